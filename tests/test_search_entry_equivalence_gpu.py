"""The top-k entry points are layers of one call (search_call in csrc/mirx_index.hip): leave-out contains deep, deep
contains masked, masked contains plain.  On one index -- 41 216 x 64 unit rows, the smallest multiple of 256 at or above
deep_min_rows(65, nq <= 64) = 41 088, where k = 10 takes FILTER, k = 65 takes DEEP with 3 queries and EXACT with 65 (their
128-query tile needs 82 176 rows) -- every containment is held to the bit: ids, fp32 values, fp64 ranking scores and the
last_stats() dicts.  Every call's route is read from last_stats() and held against tests/_route_ref.py."""
import numpy as np
import pytest
import torch

import _route_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, D = 41216, 64
ROW_BYTES = 128 * 4 + 8            # D padded to 128 floats, and the id
GATHER_MAX = 1 << 30               # MIRX_OPT_MASK_GATHER_BYTES at its default
CASES = [(nq, k) for nq in (3, 65) for k in (10, 65)]


@pytest.fixture(scope="module")
def world():
    from mirx.index import FlatIndex
    gen = torch.Generator().manual_seed(39)
    g = torch.nn.functional.normalize(torch.randn(N, D, generator=gen), dim=1)
    q = torch.nn.functional.normalize(g[:65] + 0.3 * torch.randn(65, D, generator=gen), dim=1)
    ix = FlatIndex(D, "COSINE", 0)
    ix.add(g)
    rng = np.random.default_rng(39)
    clear = torch.ones(N, dtype=torch.bool)
    clear[torch.from_numpy(rng.choice(N, 1000, replace=False))] = False
    keep = torch.zeros(N, dtype=torch.bool)
    keep[torch.from_numpy(rng.choice(N, 100, replace=False))] = True
    masks = {"ones": torch.ones(N, dtype=torch.bool), "zeros": torch.zeros(N, dtype=torch.bool), "clear1000": clear, "keep100": keep}
    assert N == (R.deep_min_rows(65, 64) + 255) // 256 * 256 and R.deep_min_rows(65, 128) > N
    return ix, q.to(DEV), masks, torch.full((N,), -1, dtype=torch.int32, device=DEV)


def _want_list(nq, k, allow_deep, n_allowed=None):
    return R.route(True, N, k, False, 0, allow_deep, n_allowed is not None, n_allowed or 0, R.query_tile(nq), ROW_BYTES, GATHER_MAX)[0]


def _run(ix, fn, nq, k, want_list):
    """both return forms of one call -> (fp32 values, fp64 scores, ids, stats), the route checked against `want_list`"""
    out = []
    for f64 in (False, True):
        s, i = fn(return_f64=f64)
        st = ix.last_stats()
        assert s.shape == i.shape == (nq, k)
        if want_list is None:
            pass                                                   # rank_top: no route, and the stats are an earlier search's
        elif want_list == R.EXACT:
            assert st["exact_answered"] == nq and st["tier1_answered"] == 0, (want_list, st)
        else:
            assert st["tier1_answered"] > 0, (want_list, st)
        assert want_list is None or st["nq"] == nq
        out.append((s, i, st))
    (s32, i32, st32), (s64, i64, st64) = out
    assert torch.equal(i32, i64) and st32 == st64
    return s32, s64, i64, st64


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64)


def _same(a, b, what, stats=True):
    """two results of _run equal to the bit, and in their stats"""
    for x, y, name in zip(a[:3], b[:3], ("fp32 values", "fp64 scores", "ids")):
        assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), (what, name)
    assert not stats or a[3] == b[3], (what, a[3], b[3])


@pytest.mark.parametrize("nq,k", CASES)
def test_each_entry_point_contains_the_one_below(world, nq, k):
    ix, q_all, masks, null_rows = world
    q = q_all[:nq]
    null_q = torch.full((nq,), -1, dtype=torch.int32)
    codes = (torch.arange(N, dtype=torch.int32, device=DEV) % 7)
    lists = {deep: _want_list(nq, k, deep) for deep in (False, True)}
    assert lists[False] == (R.FILTER if k == 10 else R.EXACT)
    assert lists[True] == (R.FILTER if k == 10 else (R.DEEP if nq == 3 else R.EXACT))

    def search(**kw):
        return lambda return_f64: ix.search(q, k, return_f64=return_f64, **kw)

    def deep(**kw):
        return lambda return_f64: ix.search_deep(q, k, return_f64=return_f64, **kw)

    def leave_out(rows, qc, **kw):
        return lambda return_f64: ix.search_leave_out(q, k, rows, qc, return_f64=return_f64, **kw)

    plain = _run(ix, search(), nq, k, lists[False])
    dp = _run(ix, deep(), nq, k, lists[True])
    if k == 10:
        _same(dp, plain, "search_deep = search")
    else:
        _same(dp, plain, "search_deep answers as search whatever the route", stats=False)
    lo_rows = _run(ix, leave_out(null_rows, codes[:nq].cpu()), nq, k, lists[True])
    _same(lo_rows, dp, "leave-out with null row codes = search_deep")
    lo_q = _run(ix, leave_out(codes, null_q), nq, k, lists[True])
    _same(lo_q, dp, "leave-out with null query codes = search_deep")

    # an all-ones mask is no mask (on the host and on the device)
    for ones in (masks["ones"], masks["ones"].to(DEV)):
        _same(_run(ix, search(allow=ones), nq, k, lists[False]), plain, "search, all ones")
        _same(_run(ix, deep(allow=ones), nq, k, lists[True]), dp, "search_deep, all ones")
        _same(_run(ix, leave_out(codes, null_q, allow=ones), nq, k, lists[True]), lo_q, "search_leave_out, all ones")

    # an all-zero mask leaves nothing, for all three
    for fn in (search(allow=masks["zeros"]), deep(allow=masks["zeros"]), leave_out(codes, null_q, allow=masks["zeros"])):
        s32, s64, ids, st = _run(ix, fn, nq, k, R.EXACT)
        assert bool((ids == -1).all()) and bool(torch.isneginf(s32).all()) and bool(torch.isneginf(s64).all())

    if k == 10:
        for name, rows_left in (("clear1000", N - 1000), ("keep100", 100)):
            m = masks[name]
            assert int(m.sum()) == rows_left
            want = _want_list(nq, k, False, rows_left)
            assert want == _want_list(nq, k, True, rows_left) == (R.FILTER if name == "clear1000" else R.EXACT)
            a = _run(ix, search(allow=m), nq, k, want)
            _same(_run(ix, deep(allow=m), nq, k, want), a, "search(allow) = search_deep(allow), " + name)
            _same(_run(ix, leave_out(codes, null_q, allow=m), nq, k, want), a, "... = search_leave_out(allow), " + name)
            allowed = torch.nonzero(m).flatten().to(DEV)
            assert bool(torch.isin(a[2], allowed).all())

    top = _run(ix, lambda return_f64: ix.rank_top(q, k, return_f64=return_f64), nq, k, None)
    top_ones = _run(ix, lambda return_f64: ix.rank_top(q, k, return_f64=return_f64, allow=masks["ones"]), nq, k, None)
    _same(top_ones, top, "rank_top = rank_top(allow = ones)", stats=False)
