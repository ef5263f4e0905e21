"""IVF_PQ with residual coding on the device (mirx.index.IvfResidualPqIndex, Collection.create_index({"index_type": "IVF_PQ",
"params": {"m": M, "by_residual": True}}, approximate=True)).

Every comparison is bit for bit -- residuals, bases, QQ, N2, codes, ids, fp64 ranking scores, fp32 reported values -- against
tests/_rpq_ref.py, the numpy restatement of include/mirx.h's definition on tests/_pq_ref.py and tests/_ivf_ref.py.

The scan starts every entry's sum from the base of the entry's OWN (query, probed list), so the shapes put several lists into
one wave of 64 entries (lists of 0, 1, 63, 64, 65, 120 and 257 rows) and a list boundary inside and on the edge of a work item
of mirx_ivf_pq_item_rows() = 1024 entries; a base taken from a neighbour's list, or an N2 read at the compact position instead
of the master position, changes the bits that are compared."""
import ctypes

import numpy as np
import pytest
import torch

import _ivf_ref as R
import _pq_ref as P
import _rpq_ref as RP
from _ivf_cases import SIZES, _bits, _lib, _np, _unit, forced

pytestmark = pytest.mark.gpu

F4, F8 = np.float32, np.float64


def _codebooks(rows, cent, metric, m, seed):
    """[m, 256, dim / m]: slices of 256 random rows' residuals"""
    res = RP.residuals(rows, R.assign(rows, cent, metric), cent)
    pick = np.random.default_rng(seed).choice(rows.shape[0], 256, replace=False)
    ds = rows.shape[1] // m
    return np.ascontiguousarray(np.stack([res[pick][:, j * ds:(j + 1) * ds] for j in range(m)]), dtype=F4)


def _rpq(rows, ids, cent, cb, metric, by_residual=True):
    from mirx.index import IvfResidualPqIndex
    ivf = IvfResidualPqIndex(rows.shape[1], metric, nlist=cent.shape[0], m=cb.shape[0], by_residual=by_residual)
    ivf.set_centroids(torch.from_numpy(cent))
    ivf.set_codebooks(torch.from_numpy(cb))
    ivf.add(torch.from_numpy(rows), None if ids is None else torch.from_numpy(ids))
    return ivf


def _layout(ivf, rows, ids, cent, cb, metric):
    """codes, N2 and reconstruct of the master are the restatement's of the ORIGINAL rows, list-major, insertion order inside"""
    codes, cid, lists = (_np(t) for t in ivf.codes())
    dec, did = (_np(t) for t in ivf.reconstruct())
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else ids
    assert codes.dtype == np.uint8 and codes.shape == (rows.shape[0], cb.shape[0])
    assert np.array_equal(cid, did) and sorted(cid.tolist()) == sorted(ids.tolist())
    where = {int(v): i for i, v in enumerate(ids)}
    src = np.array([where[int(v)] for v in cid], dtype=np.int64)
    want_lists = R.assign(rows, cent, metric)
    assert np.array_equal(lists, want_lists[src]) and (np.diff(lists) >= 0).all()
    for l in np.unique(lists):
        assert (np.diff(src[lists == l]) > 0).all()
    assert np.array_equal(codes, RP.encode(rows, want_lists, cent, cb)[src])
    assert np.array_equal(_bits(dec), _bits(RP.reconstruct(codes, lists, cent, cb)))
    if metric == "L2":
        assert np.array_equal(_bits(_np(ivf.norms())), _bits(RP.norms(codes, lists, cent, cb)))
    else:
        with pytest.raises(_lib().MirxError, match=r"\(-1\).*norms"):
            ivf.norms()


def _check(ivf, rows, ids, cent, cb, metric, q, k, nprobe, ex=None):
    qt = torch.from_numpy(q)
    ext = None if ex is None else torch.from_numpy(ex)
    s64, got, probes = ivf.search(qt, k, nprobe, exclude_ids=ext, return_f64=True, return_probes=True)
    val, got_v = ivf.search(qt, k, nprobe, exclude_ids=ext)
    s64, got, probes, val = _np(s64), _np(got), _np(probes), _np(val)
    assert np.array_equal(probes, R.probes(q, cent, nprobe, metric)) and probes.dtype == np.int32
    want_s, want_i = RP.search(q, rows, ids, cent, cb, k, nprobe, metric, exclude=ex)
    assert np.array_equal(got, want_i) and np.array_equal(_np(got_v), want_i)
    assert np.array_equal(_bits(s64), _bits(want_s))
    assert np.array_equal(_bits(val), _bits(P.values(want_s, metric)))
    return got, probes


# ---- the kernels, through the stand-alone calls ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [16, 2048])
def test_residuals_round_once(dim):
    from mirx.index import pq_residuals
    rng = np.random.default_rng(dim)
    n, nlist = 301, 7
    cent = rng.standard_normal((nlist, dim)).astype(F4)
    lists = rng.integers(0, nlist, n)
    rows = (cent[lists] + 1e3 + rng.standard_normal((n, dim))).astype(F4)  # off by 1e3: the subtraction rounds
    want = RP.residuals(rows, lists, cent)
    assert (want.astype(F8) != rows.astype(F8) - cent[lists].astype(F8)).any()           # the rounding shows
    got = pq_residuals(torch.from_numpy(rows).cuda(), torch.from_numpy(lists).cuda(), torch.from_numpy(cent).cuda())
    assert got.dtype == torch.float32 and np.array_equal(_bits(_np(got)), _bits(want))
    bad = lists.copy()
    bad[[0, n - 1]] = [-1, nlist]                                         # no such list: a NaN row, nothing read
    got = _np(pq_residuals(torch.from_numpy(rows).cuda(), torch.from_numpy(bad).cuda(), torch.from_numpy(cent).cuda()))
    assert np.isnan(got[[0, n - 1]]).all() and np.array_equal(_bits(got[1:n - 1]), _bits(want[1:n - 1]))
    assert pq_residuals(torch.empty((0, dim), device="cuda"), torch.empty((0,), dtype=torch.int64), torch.from_numpy(cent)).shape == (0, dim)


@pytest.mark.parametrize("dim, m", [(16, 4), (64, 16), (256, 64), (2048, 4)])
def test_bases_and_qq_equal_the_two_level_sums(dim, m):
    from mirx.index import pq_bases
    rng = np.random.default_rng(dim + m)
    nlist = 70                                                            # more slots than a round of 256 / m holds, for every m
    cent = (rng.standard_normal((nlist, dim)) + 1e3).astype(F4)
    flat = np.cumsum(cent.astype(F8) * cent.astype(F8), axis=1)[:, -1]
    assert dim == 16 or (RP.two_level(cent, cent, m) != flat).any()       # the two-level sum is not the one sequential sum
    for nq in (1, 5):
        q = (rng.standard_normal((nq, dim)) + 1e3).astype(F4)
        for nprobe in (1, 3, nlist):
            lists = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)]).astype(np.int32)
            base, qq = pq_bases(torch.from_numpy(q).cuda(), torch.from_numpy(lists).cuda(), torch.from_numpy(cent).cuda(), m)
            assert base.dtype == torch.float64 and tuple(base.shape) == (nq, nprobe) and tuple(qq.shape) == (nq,)
            assert np.array_equal(_bits(_np(base)), _bits(RP.bases(q, lists, cent, m)))
            assert np.array_equal(_bits(_np(qq)), _bits(RP.qq(q, m)))
    lists[0, 0] = -1                                                      # an unfilled probe slot: 0.0, nothing read
    base, _ = pq_bases(torch.from_numpy(q).cuda(), torch.from_numpy(lists).cuda(), torch.from_numpy(cent).cuda(), m)
    assert _np(base)[0, 0] == 0.0 and np.array_equal(_bits(_np(base)[1:]), _bits(RP.bases(q, lists, cent, m)[1:]))


# ---- the scan ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("m", [4, 8, 16, 64])
def test_forced_lists_every_list_edge(m, metric):
    L = _lib()
    lib = L.load()
    dim = 4 * m
    rows, ids, cent, base = forced(SIZES, dim, metric, 100 + m, 0.05 / dim ** 0.5)
    cb = _codebooks(rows, cent, metric, m, m)
    ivf = _rpq(rows, ids, cent, cb, metric)
    assert lib.mirx_ivf_kind(ivf._h) == L.IVF_PQ and lib.mirx_ivf_pq_m(ivf._h) == m and lib.mirx_ivf_pq_by_residual(ivf._h) == 1
    _layout(ivf, rows, ids, cent, cb, metric)
    assert ivf.list_sizes().tolist() == SIZES and len(ivf) == sum(SIZES)
    assert np.array_equal(_bits(_np(ivf.tables(torch.from_numpy(rows[:2])))), _bits(P.tables(rows[:2], cb, "IP")))
    rng = np.random.default_rng(m + 1)
    near = lambda l, n: (base[l] + 0.05 / dim ** 0.5 * rng.standard_normal((n, dim))).astype(F4)
    for nq in (1, 2, 17):                                                 # all probing list 0
        got, probes = _check(ivf, rows, ids, cent, cb, metric, near(0, nq), 10, 1)
        assert (probes == 0).all()
        assert ivf.last_stats() == {"nq": nq, "rows_scored": nq * SIZES[0], "pairs": nq, "work_items": nq, "batches": 1}
    pr = R.probes(near(0, 1), cent, 3, metric)
    b, qq = ivf.bases(torch.from_numpy(near(0, 1)), torch.from_numpy(pr.astype(np.int32)))
    assert tuple(b.shape) == (1, 3) and tuple(qq.shape) == (1,)
    # queries spread over the lists; list 1 (empty) is probed together with list 0, and the short lists share waves
    q = np.concatenate([near(0, 3)] + [near(l, 2) for l in (2, 3, 4, 5)])
    lists = R.assign(rows, cent, metric)
    ex = np.full(q.shape[0], -1, dtype=np.int64)
    ex[0] = ids[np.flatnonzero(lists == 0)[0]]                            # inside a probed list (an equal row: its twin must stay)
    ex[1] = ids[np.flatnonzero(lists == 6)[0]]                            # in a list the query does not probe
    ex[2] = 7                                                             # no row has this id
    for k in (1, 10, 300):
        got, probes = _check(ivf, rows, ids, cent, cb, metric, q, k, 2, ex)
        assert ex[0] not in got[0] and (probes[:3, :2] == [0, 1]).all()
    for nprobe in (3, 5):                                                 # 1 + 63 + 64 + 65 ...: boundaries inside one wave
        _check(ivf, rows, ids, cent, cb, metric, q, 300, nprobe, ex)
    twin = np.flatnonzero(lists == 0)[:2]
    got, _ = _check(ivf, rows, ids, cent, cb, metric, rows[twin[:1]], 300, 1)
    at = [got[0].tolist().index(int(ids[t])) for t in twin]
    assert ids[twin[1]] < ids[twin[0]] and at[1] + 1 == at[0]
    # every list probed, in two internal batches: the ranking of all rows; the budget counts 8 nprobe + 8 bytes a query more
    np_all = len(SIZES)
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, (8 * sum(SIZES) + 2048 * m + 8 * np_all + 8) * (q.shape[0] - 2))
    got, _ = _check(ivf, rows, ids, cent, cb, metric, q, 10, np_all, ex)
    assert ivf.last_stats()["batches"] == 2 and ivf.last_stats()["rows_scored"] == q.shape[0] * sum(SIZES)
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, (8 * sum(SIZES) + 2048 * m + 8 * np_all + 8) * q.shape[0])
    _check(ivf, rows, ids, cent, cb, metric, q, 10, np_all, ex)
    assert ivf.last_stats()["batches"] == 1                               # exactly the budget of all the queries: one batch
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, 0)
    far, _ = _check(ivf, rows, ids, cent, cb, metric, q, 10, 1000, ex)
    assert np.array_equal(far, got) and ivf.last_stats()["batches"] == 1
    # the answer depends on the flag: the raw form over the same codebooks gives other ids
    raw = _rpq(rows, ids, cent, cb, metric, by_residual=False)
    assert (_np(raw.codes()[0]) != _np(ivf.codes()[0])).any()
    _, raw_i = raw.search(torch.from_numpy(q), 10, len(SIZES), exclude_ids=torch.from_numpy(ex))
    assert not np.array_equal(_np(raw_i), got)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("m", [8, 16])                                    # 4-byte and 16-byte code loads
def test_compact_rows_on_the_item_edges(m, metric):
    lib = _lib().load()
    ir = lib.mirx_ivf_pq_item_rows()
    assert 2 * ir + 1 <= 3000
    sizes = [ir - 1, 1, 1, ir]
    dim = 64
    rows, ids, cent, base = forced(sizes, dim, metric, 77, 0.05 / dim ** 0.5)
    cb = _codebooks(rows, cent, metric, m, 3)
    ivf = _rpq(rows, ids, cent, cb, metric)
    assert ivf.list_sizes().tolist() == sizes
    mix = lambda w: _unit(np.asarray(w, dtype=F4)[None] @ base)            # probes in the order of the weights
    # list 0 | 0, 1 | 0, 1, 2 | 3, 0, 1, 2: ir - 1, ir, ir + 1 and 2 ir + 1 entries; a list boundary inside an item (after
    # ir - 1 entries: the item's last entry has another base) and on an item boundary (list 3's ir entries first)
    cases = [(mix([1, .5, .3, 0]), 1, [0], ir - 1), (mix([1, .5, .3, 0]), 2, [0, 1], ir), (mix([1, .5, .3, 0]), 3, [0, 1, 2], ir + 1),
             (mix([.5, .3, .2, 1]), 4, [3, 0, 1, 2], 2 * ir + 1)]
    for q, nprobe, order, entries in cases:
        got, probes = _check(ivf, rows, ids, cent, cb, metric, q, 300, nprobe)
        assert probes[0].tolist() == order
        assert ivf.last_stats() == {"nq": 1, "rows_scored": entries, "pairs": nprobe, "work_items": -(-entries // ir), "batches": 1}
    q = np.concatenate([c[0] for c in cases] * 2)                         # together: items of several queries in one launch
    _check(ivf, rows, ids, cent, cb, metric, q, 10, 4)
    assert ivf.last_stats()["work_items"] == 3 * q.shape[0]
    _check(ivf, rows, ids, cent, cb, metric, q, 10, 3)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("m", [8, 64])                                    # two workgroups per CU and 4-byte loads; one and 16-byte loads
def test_a_workgroup_walks_many_items_and_queries(m, metric):
    """the persistent loop of the scan: about 1100 queries over lists of 1023 / 1 / 1 / 1024 rows plus four empty lists, a fifth
    of the queries without entries, more than twice as many items as workgroups: a workgroup goes from item to item and from query
    to query, and every entry still starts from the base of its own (query, list)"""
    lib = _lib().load()
    ir = lib.mirx_ivf_pq_item_rows()
    dim = 4 * m
    sizes = [ir - 1, 1, 1, ir]
    rows, ids, cent, base = forced(sizes, dim, metric, 300 + m, 0.05 / dim ** 0.5)
    rng = np.random.default_rng(m)
    far = -_unit(base.sum(axis=0, keepdims=True))                         # four empty lists side by side, behind every other list
    cent = np.ascontiguousarray(np.concatenate([cent, (3 * far + 0.001 * rng.standard_normal((4, dim))).astype(F4)]), dtype=F4)
    if metric == "COSINE":
        cent[4:] = _unit(cent[4:])
    assert np.bincount(R.assign(rows, cent, metric), minlength=8).tolist() == sizes + [0, 0, 0, 0]
    cb = _codebooks(rows, cent, metric, m, 7)
    ivf = _rpq(rows, ids, cent, cb, metric)
    nq = 1100
    target = rng.integers(0, 5, nq)                                       # 4: the empty lists
    target[[0, 1, 500, 501, 502, nq - 1]] = 4                             # also first, last and consecutive
    centre = np.concatenate([base, cent[4:5]])[target]
    q = (centre + 0.05 / dim ** 0.5 * rng.standard_normal((nq, dim))).astype(F4)
    ex = np.where(rng.integers(0, 3, nq) == 0, ids[rng.integers(0, ids.size, nq)], -1).astype(np.int64)
    got, probes = _check(ivf, rows, ids, cent, cb, metric, q, 10, 4, ex)
    n_q = np.asarray(sizes + [0, 0, 0, 0])[probes].sum(axis=1)
    assert (n_q[target == 4] == 0).all() and (got[target == 4] == -1).all()
    items = -(-n_q // ir)
    assert {0, 3} <= set(items.tolist())
    st = ivf.last_stats()
    assert st == {"nq": nq, "rows_scored": int(n_q.sum()), "pairs": 4 * nq, "work_items": int(items.sum()), "batches": 1}
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    assert st["work_items"] > 2 * grid, (st["work_items"], grid)


# ---- training, state and layout ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_train_codebooks_on_residuals_equals_the_restatement(metric):
    from mirx.index import IvfResidualPqIndex
    L = _lib()
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((5, 16)).astype(F4)
    rows = (cent[rng.integers(0, 5, 600)] + 0.3 * rng.standard_normal((600, 16))).astype(F4)
    if metric == "COSINE":
        cent, rows = _unit(cent), _unit(rows)
    ivf = IvfResidualPqIndex(16, metric, nlist=5, m=4)
    with pytest.raises(L.MirxError, match=r"\(-4\).*mirx_ivf_train / _set_centroids"):    # residuals need centroids
        ivf.train_codebooks(torch.from_numpy(rows), 3)
    ivf.set_centroids(torch.from_numpy(cent))
    ivf.train_codebooks(torch.from_numpy(rows), 3)
    want = RP.train_codebooks(rows, cent, 4, 3, metric)
    assert np.array_equal(_bits(_np(ivf.codebooks)), _bits(want))
    assert not np.array_equal(want, P.train_codebooks(rows, 4, 3))        # not the raw rows' codebooks
    ivf.train_codebooks(torch.from_numpy(rows).cuda(), 3)                 # device rows, a second call: equal bytes
    assert np.array_equal(_bits(_np(ivf.codebooks)), _bits(want))
    both = IvfResidualPqIndex(16, metric, nlist=5, m=4)                   # train(): the centroids first, then the residual codebooks
    both.train(torch.from_numpy(rows), iters=4, codebook_iters=3)
    c2 = R.train(rows, 5, 4, metric)
    assert np.array_equal(_np(both.centroids), c2)
    assert np.array_equal(_bits(_np(both.codebooks)), _bits(RP.train_codebooks(rows, c2, 4, 3, metric)))


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_add_in_two_calls_remove_and_state_errors(metric):
    from mirx.index import IvfResidualPqIndex
    L = _lib()
    dim, m = 32, 8
    rows, ids, cent, base = forced(SIZES, dim, metric, 21, 0.05 / dim ** 0.5)
    n = rows.shape[0]
    cb = _codebooks(rows, cent, metric, m, 2)
    q = np.concatenate([(base[l] + F4(0.01)).astype(F4)[None] for l in (0, 3, 5, 6)])
    qt = torch.from_numpy(q)
    ivf = IvfResidualPqIndex(dim, metric, nlist=len(SIZES), m=m)
    with pytest.raises(L.MirxError, match=r"\(-4\).*centroids are not fixed"):
        ivf.add(torch.from_numpy(rows))
    ivf.set_centroids(torch.from_numpy(cent))
    with pytest.raises(L.MirxError, match=r"\(-4\).*codebooks are not fixed"):
        ivf.add(torch.from_numpy(rows))
    assert len(ivf) == 0
    ivf.set_codebooks(cb)
    ivf.add(torch.from_numpy(rows[:200]), torch.from_numpy(ids[:200]))
    ivf.add(torch.from_numpy(rows[200:]).cuda(), torch.from_numpy(ids[200:]).cuda())
    whole = _rpq(rows, ids, cent, cb, metric)                             # one call: a second build, equal bytes
    same = lambda a, b: all(np.array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8)) for x, y in zip(a, b))
    state = (lambda v: v.codes() + v.reconstruct() + (v.norms(),)) if metric == "L2" else (lambda v: v.codes() + v.reconstruct())
    assert same(state(ivf), state(whole))
    _layout(ivf, rows, ids, cent, cb, metric)
    for nprobe in (1, 3):
        assert same(ivf.search(qt, 20, nprobe, return_f64=True), whole.search(qt, 20, nprobe, return_f64=True))
    # an index that holds rows keeps its centroids and its codebooks: MIRX_ESTATE, nothing changed
    before = ivf.search(qt, 20, 3, return_f64=True)
    for call in (lambda: ivf.set_codebooks(cb + 1), lambda: ivf.train_codebooks(torch.from_numpy(rows), 1),
                 lambda: ivf.set_centroids(torch.from_numpy(np.ascontiguousarray(base[::-1]))),
                 lambda: ivf.train(torch.from_numpy(rows), iters=1)):
        with pytest.raises(L.MirxError, match=r"\(-4\).*holds rows"):
            call()
    assert same(state(ivf), state(whole)) and same(ivf.search(qt, 20, 3, return_f64=True), before)
    # remove: N2, codes and ids stay together -- the state and the answers of a fresh index over the survivors
    gone = np.concatenate([ids[5:60], ids[5:20], ids[n - 40:], [123456789]])
    assert ivf.remove(torch.from_numpy(gone)) == 55 + 40
    keep = np.ones(n, bool)
    keep[5:60] = keep[n - 40:] = False
    fresh = _rpq(rows[keep], ids[keep], cent, cb, metric)
    assert len(ivf) == n - 95 and same(state(ivf), state(fresh))
    _layout(ivf, rows[keep], ids[keep], cent, cb, metric)
    for nprobe in (1, 3, len(SIZES)):
        _check(ivf, rows[keep], ids[keep], cent, cb, metric, q, 20, nprobe)
    assert ivf.remove(torch.from_numpy(ids)) == n - 95 and len(ivf) == 0  # emptied, it takes new codebooks and centroids again
    ivf.set_codebooks(cb + 1)
    ivf.set_centroids(torch.from_numpy(np.ascontiguousarray(base[::-1])))
    assert ivf.codes()[0].shape == (0, m)
    # the flag is checked on the device side too; the getter answers -1 for another kind
    lib = L.load()
    h = ctypes.c_void_p()
    assert lib.mirx_ivf_create_pq_ex(dim, 0, 4, m, 8, 2, 0, ctypes.byref(h)) == -1 and not h.value
    from mirx.index import IvfFlatIndex, IvfPqIndex
    assert lib.mirx_ivf_pq_by_residual(IvfFlatIndex(dim, metric, nlist=4)._h) == -1
    raw = IvfPqIndex(dim, metric, nlist=4, m=m)
    assert lib.mirx_ivf_pq_by_residual(raw._h) == 0
    assert lib.mirx_ivf_get_norms(raw._h, None) == -1 and b"residual" in lib.mirx_last_error()


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_flag_off_through_the_new_call_is_the_raw_form(metric):
    from mirx.index import IvfPqIndex
    dim, m = 64, 16
    rows, ids, cent, base = forced(SIZES, dim, metric, 5, 0.05 / dim ** 0.5)
    cb = _codebooks(rows, np.zeros_like(cent), metric, m, 4)              # zero centroids: slices of the raw rows
    q = np.concatenate([(base[l] + F4(0.01)).astype(F4)[None] for l in (0, 2, 3, 6)])
    a, b = _rpq(rows, ids, cent, cb, metric, by_residual=False), _rpq(rows, ids, cent, cb, metric, by_residual=False)
    old = IvfPqIndex(dim, metric, nlist=len(SIZES), m=m)
    old.set_centroids(torch.from_numpy(cent))
    old.set_codebooks(torch.from_numpy(cb))
    old.add(torch.from_numpy(rows), torch.from_numpy(ids))
    assert _lib().load().mirx_ivf_pq_by_residual(a._h) == 0 and a.by_residual is False
    same = lambda x, y: all(np.array_equal(_np(s).view(np.uint8), _np(t).view(np.uint8)) for s, t in zip(x, y))
    assert same(a.codes(), b.codes()) and same(a.codes(), old.codes()) and same(a.reconstruct(), old.reconstruct())
    assert np.array_equal(_np(a.codes()[0])[np.argsort(_np(a.codes()[1]))], P.encode(rows, cb)[np.argsort(ids)])
    assert np.array_equal(_bits(_np(a.tables(torch.from_numpy(q)))), _bits(P.tables(q, cb, metric)))
    for nprobe in (1, 3, len(SIZES)):
        s, i = a.search(torch.from_numpy(q), 20, nprobe, return_f64=True)
        want_s, want_i = P.search(q, rows, ids, cent, cb, 20, nprobe, metric)
        assert np.array_equal(_np(i), want_i) and np.array_equal(_bits(_np(s)), _bits(want_s))
        assert same((s, i), b.search(torch.from_numpy(q), 20, nprobe, return_f64=True))
        assert same((s, i), old.search(torch.from_numpy(q), 20, nprobe, return_f64=True))


def test_collection_route():
    from mirx.retriever import Collection
    from mirx.index import IvfResidualPqIndex
    rng = np.random.default_rng(0)
    centres = _unit(rng.standard_normal((12, 32)))
    rows = _unit(centres[rng.integers(0, 12, 1200)] + 0.5 / 32 ** 0.5 * rng.standard_normal((1200, 32)).astype(F4))
    rng = np.random.default_rng(1)
    q = _unit(rows[rng.choice(1200, 12, replace=False)] + 0.05 * rng.standard_normal((12, 32)).astype(F4))
    labels = [f"c{i % 3}" for i in range(1200)]
    paths = [f"p{i}.png" for i in range(1200)]
    params = {"metric_type": "COSINE", "index_type": "IVF_PQ", "params": {"nlist": 12, "m": 8, "by_residual": True}}
    raw_params = {"metric_type": "COSINE", "index_type": "IVF_PQ", "params": {"nlist": 12, "m": 8}}
    approx, raw = Collection("arpq", 32), Collection("rrpq", 32)
    approx.create_index("embedding", params, approximate=True)
    raw.create_index("embedding", raw_params, approximate=True)
    for col in (approx, raw):
        col.insert([paths, labels, rows])
        col.load()
    assert type(approx._ivf) is IvfResidualPqIndex and approx._ivf.by_residual is True and approx._ivf.m == 8
    assert type(raw._ivf) is not IvfResidualPqIndex and raw._ivf.by_residual is False
    ivf = IvfResidualPqIndex(32, "COSINE", nlist=12, m=8, by_residual=True)
    ivf.train(torch.from_numpy(rows))
    ivf.add(torch.from_numpy(rows))
    cent, cb = _np(ivf.centroids), _np(ivf.codebooks)
    assert np.array_equal(cent, R.train(rows, 12, 10, "COSINE"))
    assert np.array_equal(_bits(cb), _bits(RP.train_codebooks(rows, cent, 8, 10, "COSINE")))
    pairs = lambda hits: [[(h.id, h.distance) for h in hs] for hs in hits]

    def direct(index, nprobe, ex=None):
        sc, ids = index.search(torch.from_numpy(q), 10, nprobe, exclude_ids=ex)
        return [[(int(i), float(v)) for i, v in zip(a, b) if i >= 0] for a, b in zip(_np(ids), _np(sc))]

    p2 = {"metric_type": "COSINE", "params": {"nprobe": 2}}
    got = pairs(approx.search(q, param=p2, limit=10))
    assert got == direct(ivf, 2)
    _check(ivf, rows, None, cent, cb, "COSINE", q, 10, 2)
    assert got != pairs(raw.search(q, param=p2, limit=10))                # not the raw form's answer
    ex = list(range(12))
    assert pairs(approx.search(q, param=p2, limit=10, exclude_ids=ex)) == direct(ivf, 2, ex)
    assert pairs(approx.search(q, limit=10)) == pairs(raw.search(q, limit=10))       # no nprobe: both exact
    # after delete and insert the lists are rebuilt with the kept centroids and the kept residual codebooks
    approx.delete("id in [0, 1, 2, 3, 4, 5, 6, 7]")
    late = _unit(q[:1] + F4(0.01))
    approx.insert([["n.png"], ["c0"], late])
    keep = np.arange(8, 1200)
    again = IvfResidualPqIndex(32, "COSINE", nlist=12, m=8)
    again.set_centroids(torch.from_numpy(cent))
    again.set_codebooks(cb)
    again.add(torch.from_numpy(np.concatenate([rows[keep], late])), torch.from_numpy(np.concatenate([keep, [1200]])))
    assert pairs(approx.search(q, param=p2, limit=10)) == direct(again, 2)
    assert type(approx._ivf) is IvfResidualPqIndex
    assert np.array_equal(_np(approx._ivf.centroids), cent) and np.array_equal(_bits(_np(approx._ivf.codebooks)), _bits(cb))
    codes, cid, lists = approx._ivf.codes()
    at = _np(cid) == 1200
    assert np.array_equal(_np(codes)[at][0], RP.encode(late, _np(lists)[at], cent, cb)[0])
