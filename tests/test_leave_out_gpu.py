"""Leave-group-out search (FlatIndex.search_leave_out, mirx_index_search_leave_out).  GPU only.

Bar of every result (tests/test_search_filter_edges_gpu.py's `_check`): ids equal, fp64 ranking scores bit-identical, fp32 values
equal to the rounded fp64 value, for both return forms.  Every case is held against two references:
  (a) tests/_leave_out_ref.py, the numpy restatement of the contract over oracle.search's fp64 scores;
  (b) the parent's own masked route, once per distinct query code c: index.search(q[codes == c], k, allow=(row_codes != c)),
      or search_deep past TIER1_MAX_K.
Where a route must answer it is asserted from last_stats() under MIRX_OPT_FORCE_TAU, after a float64 host precondition that the
forced threshold leaves the guard room (tau below the k_eff-th eligible score by more than 4 eps) and the lists within capacity.

Data: one unit gallery of width 64 seeded on the device; per query i a number m_i of planted near-copies of the query that carry
the query's code, so that the query's best m_i rows are exactly the rows it leaves out."""
import os
import re

import numpy as np
import pytest
import torch

import _leave_out_ref as R
from oracle import search as OS

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-retrieval---thesis-2026_amd", "csrc")
DEV = "cuda:0"


def _constexpr(fname, name):
    with open(os.path.join(_CSRC, fname)) as f:
        m = re.search(r"constexpr\s+(?:int|int64_t)\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    assert m, (fname, name)
    return int(m.group(1))


MIN_ROWS = _constexpr("mirx_api.hip", "TIER1_MIN_ROWS")
MAX_K = _constexpr("mirx_api.hip", "TIER1_MAX_K")
CAND_CAP = _constexpr("mirx_common.h", "CAND_CAP")
DEEP_CAP = _constexpr("mirx_common.h", "DEEP_CAP")
DIM_ALIGN = _constexpr("mirx_common.h", "DIM_ALIGN")
METRICS = {"COSINE": 0, "L2": 1}
_D = 64
_N1 = MIN_ROWS + 37
_M = [0, 1, 9, 63, 64, 200]                                   # planted near-copies per query, cycled over the queries
_NQ1 = 33
_NMAX = 2 * MIN_ROWS + 257                                    # the largest gallery a case of the shared data takes


def deep_min_rows(k_eff, nq):
    target = _constexpr("mirx_common.h", "DEEP_TARGET_MUL") * k_eff + _constexpr("mirx_common.h", "DEEP_TARGET_ADD")
    tile = 64 if nq <= 64 else (128 if nq <= 128 else 256)
    return max(MIN_ROWS, target * _constexpr("mirx_common.h", "DEEP_GROUP_ROWS") // (8 // (tile // 64)))


def _ragged(rows):
    return (rows + 255) // 256 * 256 + 257


def _dimp(d):
    return (d + DIM_ALIGN - 1) // DIM_ALIGN * DIM_ALIGN


def _unit(n, d, seed):
    """unit rows seeded on the device -> float32 on the host (the oracle's input; the index gets the same bits)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, device=DEV, generator=gen), dim=1).cpu()


def _near(q, count, sigma, seed):
    """`count` unit rows near the unit vector q: cos about 1 / sqrt(1 + sigma^2 d)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    noise = torch.randn(count, q.shape[0], device=DEV, generator=gen).cpu()
    return torch.nn.functional.normalize(q[None] + sigma * noise, dim=1)


def _filter_scores(q, g, metric):
    """[nq, n] float64 in the filter's space: q.g, for L2 q.g - |g|^2 / 2"""
    s = q.double() @ g.double().t()
    if metric == 1:
        s -= 0.5 * (g.double() ** 2).sum(1)[None]
    return s


def _eps(q, g, metric):
    qn, gn = q.double().norm(dim=1), g.double().norm(dim=1).max()
    e = qn * gn * (2.0 ** -8 + 2.0 ** -18 + _dimp(g.shape[1]) * 2.0 ** -23)
    if metric == 1:
        e = e + 2.0 ** -23 * (gn * gn + qn * gn)
    return e


def _index(d, metric, g, ids=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(d, metric, 0)
    ix.add(g, ids)
    return ix


def _same(got, want, what):
    assert torch.equal(got[1], want[1]), what
    assert torch.equal(got[0], want[0]), what


def _check(ix, q, k, rcodes, qcodes, metric, g, ids=None, exclude=None, allow=None, hint=-1, ref_every=1):
    """both return forms of search_leave_out against (a) and (b) -> (stats of the fp64 call, reference ids)"""
    nq = q.shape[0]
    rc = torch.from_numpy(np.ascontiguousarray(rcodes, dtype=np.int32)).to(DEV)
    ex = None if exclude is None else torch.as_tensor(np.asarray(exclude, dtype=np.int64))
    am = None if allow is None else torch.as_tensor(np.asarray(allow, dtype=bool))
    got64 = ix.search_leave_out(q, k, rc, qcodes, exclude_ids=ex, allow=am, return_f64=True, max_left_out=hint)
    st = ix.last_stats()
    got32 = ix.search_leave_out(q, k, rc, torch.as_tensor(np.asarray(qcodes)), exclude_ids=ex, allow=am, max_left_out=hint)
    print("leave_out k=%d nq=%d hint=%d %s" % (k, nq, hint, st))
    assert st["nq"] == nq and st["tier1_answered"] + st["exact_answered"] == nq, st
    s64, i64, s32 = got64[0].cpu().numpy(), got64[1].cpu().numpy(), got32[0].cpu().numpy()
    assert torch.equal(got32[1], got64[1])
    # (a) the restatement
    sel = np.arange(0, nq, ref_every)
    r_s, r_i = R.topk(q.numpy()[sel], g.numpy(), k, rcodes, np.asarray(qcodes)[sel], metric, ids=ids,
                      exclude=None if exclude is None else np.asarray(exclude)[sel], allow=allow)
    np.testing.assert_array_equal(i64[sel], r_i)
    np.testing.assert_array_equal(s64[sel], r_s)                                      # bit-identical fp64
    np.testing.assert_array_equal(s32[sel], OS.reported_value(r_s, metric).astype(np.float32))
    # (b) the parent's masked route, per distinct query code
    find = ix.search if k + (0 if exclude is None else 1) <= MAX_K else ix.search_deep
    qc = np.asarray(qcodes)
    for c in np.unique(qc):
        rows = torch.as_tensor(np.nonzero(qc == c)[0])
        mask = np.ones(len(rcodes), dtype=bool) if c < 0 else np.asarray(rcodes) != c
        if allow is not None:
            mask = mask & np.asarray(allow, dtype=bool)
        want = find(q[rows], k, exclude_ids=None if ex is None else ex[rows], return_f64=True, allow=torch.from_numpy(mask).to(DEV))
        _same((got64[0][rows.to(DEV)], got64[1][rows.to(DEV)]), want, ("parent route, code", int(c)))
    return st, i64


# ---- shared data ----------------------------------------------------------------------------------------------------------
_cache = {}


def _world(rows=_N1):
    """-> (gallery [rows, 64], queries [33, 64], row codes, query codes, planted rows per query).  Query i has m_i = _M[i % 6]
    planted near-copies among the first MIN_ROWS rows, which carry code i; every other row carries 1000 + r % 50, or the null
    code -1 where r % 11 == 0.  Built once, at the size of the largest case; a case takes its leading rows."""
    w = _cache.get("w")
    if w is None:
        n = _NMAX
        assert rows <= n
        g = _unit(n, _D, 3801)
        q = _unit(_NQ1, _D, 3802)
        r = np.arange(n)
        codes = np.where(r % 11 == 0, -1, 1000 + r % 50).astype(np.int32)
        spots = np.random.default_rng(3803).permutation(MIN_ROWS)
        planted, at = [], 0
        for i in range(_NQ1):
            m = _M[i % len(_M)]
            rows_i = np.sort(spots[at:at + m])
            at += m
            if m:
                g[torch.as_tensor(rows_i)] = _near(q[i], m, 0.02, 3810 + i)
            codes[rows_i] = i
            planted.append(rows_i)
        # the premise: a query's best m_i rows are exactly its planted rows
        s = q.double() @ g.double().t()
        for i, rows_i in enumerate(planted):
            if len(rows_i):
                top = s[i].topk(len(rows_i)).indices.numpy()
                assert set(top.tolist()) == set(rows_i.tolist()), i
        w = _cache["w"] = (g, q, codes, np.arange(_NQ1, dtype=np.int32), planted)
    g, q, codes, qcodes, planted = w
    return g[:rows], q, codes[:rows], qcodes, planted


def _forced_tau(q, g, metric, rcodes, qcodes, k_eff, tau, cap):
    """the host precondition of a forced threshold: every query keeps more than k_eff eligible rows 4 eps above tau, and the
    rows that can pass tau number at most `cap` -> the rows that surely pass, per query"""
    s, eps = _filter_scores(q, g, metric), _eps(q, g, metric)
    elig = torch.from_numpy(np.asarray(rcodes)[None, :] != np.asarray(qcodes)[:, None])
    kth = s.masked_fill(~elig, -np.inf).topk(k_eff, dim=1).values[:, -1]
    assert (kth - 4.0 * eps > tau).all(), float((kth - 4.0 * eps).min())
    assert int((s > tau - eps[:, None]).sum(1).max()) <= cap
    return (s > tau + eps[:, None]).sum(1)


def _set_tau(ix, tau):
    from mirx import _lib as L
    ix.set_option(L.OPT_FORCE_TAU, L.FORCE_TAU_OFF if tau is None else int(np.float32(tau).view(np.uint32)))


# ---- 1. the candidate lists (tier 1) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_tier1_planted_groups(metric):
    mc, k = METRICS[metric], 10
    g, q, rcodes, qcodes, planted = _world()
    total = sum(len(p) for p in planted)
    ix = _index(_D, metric, g)
    # natural thresholds; with the true bound as the hint k_eff = 210 is past the lists and this gallery too small for the deep
    # route: the exact scan answers, with the same lists
    st, r_i = _check(ix, q, k, rcodes, qcodes, mc, g)
    assert st["tier1_answered"] > 0, st
    for i, rows_i in enumerate(planted):
        assert not np.isin(r_i[i], rows_i).any()
    st, r_i2 = _check(ix, q, k, rcodes, qcodes, mc, g, hint=max(_M))
    assert st["exact_answered"] == _NQ1, st
    np.testing.assert_array_equal(r_i2, r_i)
    # a low threshold: every query's list holds its planted rows and at least k more, and the lists answer every query
    tau = 0.36 - (0.5 if mc == 1 else 0.0)
    sure = _forced_tau(q, g, mc, rcodes, qcodes, k, tau, CAND_CAP)
    assert all(int(sure[i]) >= len(p) + k for i, p in enumerate(planted))
    _set_tau(ix, tau)
    st, _ = _check(ix, q, k, rcodes, qcodes, mc, g)
    assert st["tier1_answered"] == _NQ1 and st["exact_answered"] == 0 and st["left_out"] == total, st
    assert st["overflowed"] == 0 and st["incomplete"] == 0 and st["candidates"] >= total + k * _NQ1, st
    # a high threshold: only planted rows pass it, so no query keeps k survivors (the m = 200 queries hold 200 candidates and
    # not one survivor): the guard counts survivors, and the exact scan answers
    tau = 0.9 - (0.5 if mc == 1 else 0.0)
    s = _filter_scores(q, g, mc)
    own = torch.from_numpy(rcodes[None, :] == qcodes[:, None])
    assert float(s.masked_fill(own, -np.inf).max()) < tau - float(_eps(q, g, mc).max())
    assert float(s.masked_fill(~own, np.inf).min()) > tau + float(_eps(q, g, mc).max())
    _set_tau(ix, tau)
    st, _ = _check(ix, q, k, rcodes, qcodes, mc, g)
    assert st["exact_answered"] == _NQ1 and st["tier1_answered"] == 0 and st["candidates"] == 0 and st["left_out"] == 0, st
    assert st["incomplete"] == _NQ1 and st["overflowed"] == 0, st


# ---- 2. with excluded ids ----------------------------------------------------------------------------------------------------
def test_excluded_id_outside_and_inside_the_group():
    k = 10
    g, q, rcodes, qcodes, planted = _world()
    ids = np.arange(_N1, dtype=np.int64) * 3 + 7
    ix = _index(_D, "COSINE", g, torch.from_numpy(ids))
    s = (q.double() @ g.double().t()).numpy()
    own = rcodes[None, :] == qcodes[:, None]
    best_other = ids[np.where(own, -np.inf, s).argmax(1)]                    # the best eligible row: in another group
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, ids=ids, exclude=best_other)
    assert not (r_i == best_other[:, None]).any()
    inside = np.array([ids[p[0]] if len(p) else -1 for p in planted], dtype=np.int64)      # a row the code drops anyway
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, ids=ids, exclude=inside)
    _, plain_i = _check(ix, q, k, rcodes, qcodes, 0, g, ids=ids)
    np.testing.assert_array_equal(r_i, plain_i)                             # the same lists as without it: not counted twice
    tau = 0.36
    _forced_tau(q, g, 0, rcodes, qcodes, k + 1, tau, CAND_CAP)
    _set_tau(ix, tau)
    st, _ = _check(ix, q, k, rcodes, qcodes, 0, g, ids=ids, exclude=inside)
    assert st["tier1_answered"] == _NQ1 and st["left_out"] == sum(len(p) for p in planted), st


@pytest.mark.parametrize("k,excl,hint,deep", [(MAX_K, False, 0, False), (MAX_K - 1, True, 0, False), (10, False, MAX_K - 10, False),
                                              (MAX_K + 1, False, 0, True), (MAX_K, True, 0, True), (10, False, MAX_K - 9, True),
                                              (10, True, MAX_K - 10, True)])
def test_k_eff_across_the_tier1_deep_boundary(k, excl, hint, deep):
    """k_eff = k (+1) + hint = 64 stays on the candidate lists, 65 takes the deep route.  Told apart by capacity: tau is forced
    so that every query has more than CAND_CAP and fewer than DEEP_CAP candidates -- the lists overflow (exact scan), the deep
    route answers."""
    n = _ragged(deep_min_rows(MAX_K + 1, _NQ1))
    g, q, rcodes, qcodes, planted = _world(n)
    tau = 0.2
    sure = _forced_tau(q, g, 0, rcodes, qcodes, k + 1, tau, DEEP_CAP)
    assert int(sure.min()) > CAND_CAP + 256
    ix = _index(_D, "COSINE", g)
    _set_tau(ix, tau)
    ex = np.array([p[0] if len(p) else 5 for p in planted], dtype=np.int64) if excl else None
    st, _ = _check(ix, q, k, rcodes, qcodes, 0, g, exclude=ex, hint=hint)
    if deep:
        assert st["tier1_answered"] == _NQ1 and st["overflowed"] == 0 and st["left_out"] == sum(len(p) for p in planted), st
    else:
        assert st["overflowed"] == _NQ1 and st["exact_answered"] == _NQ1 and st["left_out"] == 0, st


# ---- 3. edge codes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,excl", [(10, False), (10, True), (MAX_K + 1, False), (MAX_K, True)])
def test_negative_query_codes_are_the_plain_search(k, excl):
    n = _ragged(deep_min_rows(MAX_K + 1, _NQ1))
    g, q, rcodes, _, planted = _world(n)
    ix = _index(_D, "COSINE", g)
    rc = torch.from_numpy(rcodes).to(DEV)
    ex = torch.as_tensor(np.array([p[0] if len(p) else 5 for p in planted])) if excl else None
    find = ix.search if k + int(excl) <= MAX_K else ix.search_deep
    for form in (False, True):
        want = find(q, k, exclude_ids=ex, return_f64=form)
        st_want = ix.last_stats()
        got = ix.search_leave_out(q, k, rc, [-1] * _NQ1, exclude_ids=ex, return_f64=form)
        st_got = ix.last_stats()
        _same(got, want, (k, excl, form))
        assert st_got == st_want and st_got["tier1_answered"] > 0 and st_got["left_out"] == 0, (st_got, st_want)
    # any negative code is the null, on either side: a row code equal to a negative query code is not dropped
    neg = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    _same(ix.search_leave_out(q, k, neg, [-5] * _NQ1, exclude_ids=ex, return_f64=True), find(q, k, exclude_ids=ex, return_f64=True),
          "negative row codes")
    st, r_i = _check(ix, q, k, np.full(n, -1, dtype=np.int32), np.arange(_NQ1, dtype=np.int32), 0, g)
    assert st["left_out"] == 0


def test_whole_gallery_in_the_group_and_fewer_than_k_eligible():
    g, q, _, _, _ = _world()
    ix = _index(_D, "COSINE", g)
    k = 10
    rcodes = np.full(_N1, 3, dtype=np.int32)
    qcodes = np.array([3] * 16 + [4] * 16 + [-1], dtype=np.int32)
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g)
    assert (r_i[:16] == -1).all() and (r_i[16:] >= 0).all()
    s, i = ix.search_leave_out(q[:16], k, torch.from_numpy(rcodes).to(DEV), qcodes[:16], return_f64=True)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    s32, _ = ix.search_leave_out(q[:16], k, torch.from_numpy(rcodes).to(DEV), qcodes[:16])
    assert bool(torch.isinf(s32).all()) and bool((s32 < 0).all())
    few = np.array([5, 777, 20000, _N1 - 1])
    rcodes[few] = -1                                                           # four rows outside the group
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g)
    assert (np.sort(r_i[:16, :4], axis=1) == few[None]).all() and (r_i[:16, 4:] == -1).all()


# ---- 4. masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_mask_route_a_bias(metric):
    """every second row of a gallery twice the filter's minimum: the filter answers under the mask's bias"""
    mc, k = METRICS[metric], 10
    n = _NMAX
    g, q, rcodes, qcodes, planted = _world(n)
    allow = np.arange(n) % 2 == 0
    ix = _index(_D, metric, g)
    st, r_i = _check(ix, q, k, rcodes, qcodes, mc, g, allow=allow)
    assert st["tier1_answered"] > 0 and st["left_out"] > 0, st
    assert (r_i % 2 == 0).all()
    with pytest.raises(ValueError):
        ix.search_leave_out(q, k, torch.from_numpy(rcodes).to(DEV), qcodes, allow=torch.ones(n - 1, dtype=torch.bool))
    s, i = ix.search_leave_out(q, k, torch.from_numpy(rcodes).to(DEV), qcodes, allow=torch.zeros(n, dtype=torch.bool), return_f64=True)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s < 0).all())
    assert ix.last_stats()["left_out"] == 0


def test_mask_route_b_gathers_the_codes_with_the_rows():
    """500 allowed rows at r = 13 j + 5 with row codes r % 7: the j-th gathered row's code is (13 j + 5) % 7, not j % 7 and not
    the code of index row j -- codes read in index order against gathered rows would drop the wrong rows.  Then the same call
    with the gather's scratch limited to 1 KiB: the in-place fallback, which reads the codes as they are."""
    from mirx import _lib as L
    g, q, _, _, _ = _world()
    k = 10
    rcodes = (np.arange(_N1) % 7).astype(np.int32)
    allow = np.zeros(_N1, dtype=bool)
    allow[13 * np.arange(500) + 5] = True
    qcodes = (np.arange(_NQ1) % 8).astype(np.int32) - 1                       # -1, 0 .. 6
    ix = _index(_D, "COSINE", g)
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, allow=allow)
    assert st["exact_answered"] == _NQ1
    for i in range(_NQ1):
        assert (r_i[i] >= 0).all() and allow[r_i[i]].all() and not (rcodes[r_i[i]] == qcodes[i]).any()
    ix.set_option(L.OPT_MASK_GATHER_BYTES, 1024)
    try:
        st2, r_i2 = _check(ix, q, k, rcodes, qcodes, 0, g, allow=allow)
    finally:
        ix.set_option(L.OPT_MASK_GATHER_BYTES, -1)
    np.testing.assert_array_equal(r_i2, r_i)
    assert st2["exact_answered"] == _NQ1


# ---- 5. the deep route -----------------------------------------------------------------------------------------------------------
def _straddle(n, nq, k):
    """per query 25 rows nearer than a group of 150 rows that carries the query's code: the group lies at ranks 26 .. 175 of the
    plain ranking, across rank k = 100"""
    g = _unit(n, _D, 3821).clone()
    q = _unit(nq, _D, 3822)
    r = np.arange(n)
    rcodes = (2000 + r % 31).astype(np.int32)
    spots = np.random.default_rng(3823).permutation(MIN_ROWS)
    groups = []
    for i in range(nq):
        front, grp = np.sort(spots[i * 175:i * 175 + 25]), np.sort(spots[i * 175 + 25:(i + 1) * 175])
        g[torch.as_tensor(front)] = _near(q[i], 25, 0.01, 3830 + i)
        g[torch.as_tensor(grp)] = _near(q[i], 150, 0.03, 3930 + i)
        rcodes[grp] = i
        groups.append((front, grp))
    s = q.double() @ g.double().t()
    for i, (front, grp) in enumerate(groups):
        top = s[i].topk(175).indices.numpy()
        assert set(top[:25].tolist()) == set(front.tolist()) and set(top[25:].tolist()) == set(grp.tolist())
    return g, q, rcodes, np.arange(nq, dtype=np.int32), groups


def test_deep_group_straddling_rank_100_and_the_hint():
    nq, k, m = 16, 100, 150
    n = _ragged(deep_min_rows(k + m, nq))
    g, q, rcodes, qcodes, groups = _straddle(n, nq, k)
    ix = _index(_D, "COSINE", g)
    outs = {}
    for hint in (-1, 0, m, 1000):
        st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, hint=hint)
        outs[hint] = (ix.search_leave_out(q, k, torch.from_numpy(rcodes).to(DEV), qcodes, return_f64=True, max_left_out=hint), st)
        for i, (front, grp) in enumerate(groups):
            assert set(r_i[i, :25].tolist()) == set(front.tolist()) and not np.isin(r_i[i], grp).any()
        if hint == 1000:
            assert st["exact_answered"] == nq and st["tier1_answered"] == 0, st          # k_eff + hint > 1024: the exact scan
    for hint in (0, m, 1000):
        _same(outs[hint][0], outs[-1][0], ("hint", hint))
    # the routes, by capacity: with tau forced to leave about 2500 candidates the deep lists answer at every hint <= 150
    tau = 0.22
    sure = _forced_tau(q, g, 0, rcodes, qcodes, k, tau, DEEP_CAP)
    assert int(sure.min()) > CAND_CAP + 256
    _set_tau(ix, tau)
    for hint in (-1, m):
        st, _ = _check(ix, q, k, rcodes, qcodes, 0, g, hint=hint)
        assert st["tier1_answered"] == nq and st["left_out"] == nq * m and st["overflowed"] == 0, st


def test_deep_k_1024():
    nq, k = 8, 1024
    n = _ragged(deep_min_rows(k, nq))
    g, q, rcodes, qcodes, groups = _straddle(n, nq, k)
    s, eps = _filter_scores(q, g, 0), _eps(q, g, 0)
    elig = torch.from_numpy(rcodes[None, :] != qcodes[:, None])
    kth = s.masked_fill(~elig, -np.inf).topk(k, dim=1).values[:, -1]
    assert int((s >= (kth - 4.0 * eps)[:, None]).sum(1).max()) <= DEEP_CAP
    ix = _index(_D, "COSINE", g)
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, hint=0)
    assert st["tier1_answered"] >= 0.9 * nq and st["left_out"] > 0, st
    for i, (front, grp) in enumerate(groups):
        assert not np.isin(r_i[i], grp).any()


def test_deep_run_of_identical_rows_half_of_them_in_the_group():
    """tau forced to 0.5 over runs of DEEP_CAP identical rows (tests/test_search_deep_gpu.py's `_runs`): a query equal to a base
    vector admits exactly its run, the list is full to the last entry, every second row of the run carries the query's code.
    The 2048 survivors tie in the filter and in fp64: the answer is the k lowest eligible ids, and only survivors are re-scored."""
    nq, k, run, d = 8, 1024, DEEP_CAP, 256
    nbase = -(-deep_min_rows(k, nq) // run)
    base = _unit(nbase, d, 3841)
    dots = (base.double() @ base.double().t()).fill_diagonal_(-1)
    assert float(dots.max()) < 0.5 - 4 * (2.0 ** -8 + 2.0 ** -18 + _dimp(d) * 2.0 ** -23)
    qi = (torch.arange(nq) * 5) % nbase
    g, q = base.repeat_interleave(run, dim=0), base[qi]
    r = np.arange(g.shape[0])
    rcodes = np.where(r % 2 == 0, r // run, -1).astype(np.int32)               # even rows: the run's number; odd rows: null
    qcodes = qi.numpy().astype(np.int32)
    ix = _index(d, "COSINE", g)
    _set_tau(ix, 0.5)
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, hint=0)
    first = (qi * run).numpy()
    np.testing.assert_array_equal(r_i, first[:, None] + 1 + 2 * np.arange(k)[None, :])
    assert st["candidates"] == nq * run and st["left_out"] == nq * run // 2 and st["reranked"] == nq * run // 2, st
    assert st["tier1_answered"] == nq and st["overflowed"] == 0 and st["incomplete"] == 0, st


@pytest.mark.parametrize("nq", [63, 64, 65, 129, 300])
def test_deep_query_counts_around_the_query_tiles(nq):
    """the query tiles of the deep route (64 / 128 / 256 queries), each at its smallest gallery; a quarter of the gallery shares
    each query's code, so a quarter of every candidate list is dropped"""
    k = 100
    n = _ragged(deep_min_rows(k, nq))
    g = _unit(n, _D, 3851)
    rows = (np.arange(nq) * 977 + 3) % n
    gen = torch.Generator().manual_seed(3852)
    q = torch.nn.functional.normalize(g[rows] + 0.5 / _D ** 0.5 * torch.randn(nq, _D, generator=gen), dim=1)
    rcodes = (np.arange(n) % 4).astype(np.int32)
    qcodes = ((np.arange(nq) % 5) - 1).astype(np.int32)                        # -1, 0, 1, 2, 3
    ix = _index(_D, "COSINE", g)
    st, r_i = _check(ix, q, k, rcodes, qcodes, 0, g, ref_every=1 if nq <= 65 else 5)
    assert st["tier1_answered"] >= 0.9 * nq and st["left_out"] > 0, st


# ---- 6. the exact tier ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("k", [10, 1000])
def test_exact_tier_small_gallery(k, metric):
    mc, n, nq = METRICS[metric], 1000, 20
    g, q = _unit(n, _D, 3861), _unit(nq, _D, 3862)
    rcodes = (np.arange(n) % 7).astype(np.int32) - 1
    qcodes = (np.arange(nq) % 9).astype(np.int32) - 1                          # -1, 0 .. 5, and 6, 7 that no row carries
    ids = np.arange(n, dtype=np.int64)[::-1].copy() * 2
    ix = _index(_D, metric, g, torch.from_numpy(ids))
    st, r_i = _check(ix, q, k, rcodes, qcodes, mc, g, ids=ids, exclude=ids[(np.arange(nq) * 37) % n])
    assert st["exact_answered"] == nq and st["left_out"] == 0, st
    if k == 1000:
        assert ((r_i == -1).sum(1) > 0).all()                                  # the excluded id at least leaves a slot empty


def test_exact_only_tier_and_a_padded_width():
    from mirx import _lib as L
    g, q, rcodes, qcodes, planted = _world()
    ix = _index(_D, "COSINE", g)
    ix.set_option(L.OPT_TIERS, L.TIER_EXACT_ONLY)
    try:
        st, r_i = _check(ix, q, 10, rcodes, qcodes, 0, g, hint=max(_M))
    finally:
        ix.set_option(L.OPT_TIERS, L.TIER_AUTO)
    assert st["exact_answered"] == _NQ1 and st["tier1_answered"] == 0 and st["left_out"] == 0, st
    d, n, nq = 100, 1500, 12
    g2, q2 = _unit(n, d, 3871), _unit(nq, d, 3872)
    rc2 = (np.arange(n) % 5).astype(np.int32)
    ix2 = _index(d, "L2", g2)
    _check(ix2, q2, 10, rc2, (np.arange(nq) % 5).astype(np.int32), 1, g2)


# ---- 7. after remove; determinism; the busy rule ---------------------------------------------------------------------------------
def test_after_remove_with_codes_in_the_new_row_order():
    k = 10
    n_big = _N1 + MIN_ROWS // 2 + 300                                          # two thirds of it still reach the filter
    g, q, rcodes, qcodes, _ = _world(n_big)
    ids = np.arange(n_big, dtype=np.int64) * 2 + 1
    ix = _index(_D, "COSINE", g, torch.from_numpy(ids))
    gone = np.arange(n_big) % 3 == 1
    assert ix.remove(torch.from_numpy(ids[gone])) == int(gone.sum())
    keep = ~gone
    assert int(keep.sum()) >= MIN_ROWS
    st, r_i = _check(ix, q, k, rcodes[keep], qcodes, 0, g[torch.from_numpy(keep)], ids=ids[keep])
    assert st["tier1_answered"] > 0 and st["left_out"] > 0, st
    assert not np.isin(r_i, ids[gone]).any()


def test_same_call_twice_and_busy_index():
    from mirx import _lib as L
    g, q, rcodes, qcodes, _ = _world()
    ix = _index(_D, "COSINE", g)
    rc = torch.from_numpy(rcodes).to(DEV)
    a = ix.search_leave_out(q, 10, rc, qcodes, return_f64=True)
    st = ix.last_stats()
    assert st["tier1_answered"] > 0 and st["left_out"] > 0, st
    b = ix.search_leave_out(q, 10, rc, qcodes, return_f64=True)
    _same(a, b, "twice")
    assert ix.last_stats() == st
    h = ix.search_begin(q, 10)
    with pytest.raises(L.MirxError, match=r"\(%d\).*mirx_index_search_end" % L.ESTATE):
        ix.search_leave_out(q, 10, rc, qcodes)
    with pytest.raises(L.MirxError, match=r"\(%d\).*mirx_index_search_end" % L.ESTATE):
        ix.search_leave_out(q, 10, rc, qcodes, allow=torch.ones(_N1, dtype=torch.bool))
    ix.search_end(h)
    _same(ix.search_leave_out(q, 10, rc, qcodes, return_f64=True), a, "after search_end")


def test_python_argument_checks():
    g, q, rcodes, qcodes, _ = _world()
    ix = _index(_D, "COSINE", g)
    rc = torch.from_numpy(rcodes).to(DEV)
    for bad in (rc.cpu(), rc.to(torch.int64), rc[:-1], rcodes, rc.reshape(1, -1)):
        with pytest.raises(ValueError):
            ix.search_leave_out(q, 10, bad, qcodes)
    with pytest.raises(ValueError):
        ix.search_leave_out(q, 10, rc, qcodes[:-1])
    with pytest.raises(ValueError):
        ix.search_leave_out(q, 10, rc, qcodes.astype(np.float32))
    for k in (0, 1025):
        with pytest.raises(ValueError):
            ix.search_leave_out(q, k, rc, qcodes)
    from mirx.index import FlatIndex
    empty = FlatIndex(_D, "COSINE", 0)
    s, i = empty.search_leave_out(q, 5, torch.empty(0, dtype=torch.int32, device=DEV), qcodes)
    assert bool((i == -1).all()) and bool(torch.isinf(s).all())
