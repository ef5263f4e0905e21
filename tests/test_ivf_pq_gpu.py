"""IVF_PQ on the device (mirx.index.IvfPqIndex, Collection.create_index({"index_type": "IVF_PQ", "params": {"m": M}},
approximate=True)).

The rule: an IVF_PQ answer is the exact top-k of the ADC score over the rows of the probed lists.  Every comparison is bit for
bit -- ids, fp64 ranking scores, fp32 reported values, tables, codes, codebooks -- against tests/_pq_ref.py, the numpy
restatement on tests/_ivf_ref.py and oracle.search; the lists come from the ORIGINAL rows.

Shapes sit on the edges of the scan as built: a work item is mirx_ivf_pq_item_rows() = 1024 consecutive entries of a query's
compact score row, one per thread, so compact rows hold 1023, 1024, 1025 and 2049 entries, with a list boundary inside an item
and on an item boundary; lists hold 0, 1, 63, 64, 65 and 257 rows; m = 4, 8 (4-byte code loads) and 16, 64 (16-byte loads).
The grid is persistent (CUs x 1 or 2 workgroups, a contiguous run of items each): one case launches more than twice as many
items as workgroups, so that a workgroup walks from item to item and from query to query, over queries without entries."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _ivf_ref as R
import _pq_ref as P
from _ivf_cases import SIZES, _bits, _lib, _np, _unit, forced

pytestmark = pytest.mark.gpu

F4 = np.float32


def _codebooks(rows, m, seed):
    """[m, 256, dim / m]: slices of random rows"""
    pick = np.random.default_rng(seed).choice(rows.shape[0], 256, replace=False)
    ds = rows.shape[1] // m
    return np.ascontiguousarray(np.stack([rows[pick][:, j * ds:(j + 1) * ds] for j in range(m)]), dtype=F4)


def _pq(rows, ids, cent, cb, metric):
    from mirx.index import IvfPqIndex
    ivf = IvfPqIndex(rows.shape[1], metric, nlist=cent.shape[0], m=cb.shape[0])
    ivf.set_centroids(torch.from_numpy(cent))
    ivf.set_codebooks(torch.from_numpy(cb))
    ivf.add(torch.from_numpy(rows), None if ids is None else torch.from_numpy(ids))
    return ivf


def _layout(ivf, rows, ids, cent, cb, metric):
    """codes / reconstruct / lists of the master are the restatement's of the ORIGINAL rows, list-major, insertion order inside"""
    codes, cid, lists = (_np(t) for t in ivf.codes())
    dec, did = (_np(t) for t in ivf.reconstruct())
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else ids
    assert codes.dtype == np.uint8 and codes.shape == (rows.shape[0], cb.shape[0])
    assert np.array_equal(cid, did) and sorted(cid.tolist()) == sorted(ids.tolist())
    where = {int(v): i for i, v in enumerate(ids)}
    src = np.array([where[int(v)] for v in cid], dtype=np.int64)          # master position -> caller's row (ids are unique)
    assert np.array_equal(lists, R.assign(rows, cent, metric)[src])       # the list of every id: from the original row
    assert (np.diff(lists) >= 0).all()
    for l in np.unique(lists):
        assert (np.diff(src[lists == l]) > 0).all()
    assert np.array_equal(codes, P.encode(rows, cb)[src])
    assert np.array_equal(_bits(dec), _bits(P.decode(codes, cb)))


def _check(ivf, rows, ids, cent, cb, metric, q, k, nprobe, ex=None):
    """ivf.search(q, k, nprobe) against the restatement: ids, fp64 scores, fp32 values, probes; returns (ids, probes)"""
    qt = torch.from_numpy(q)
    ext = None if ex is None else torch.from_numpy(ex)
    s64, got, probes = ivf.search(qt, k, nprobe, exclude_ids=ext, return_f64=True, return_probes=True)
    val, got_v = ivf.search(qt, k, nprobe, exclude_ids=ext)
    s64, got, probes, val = _np(s64), _np(got), _np(probes), _np(val)
    assert np.array_equal(probes, R.probes(q, cent, nprobe, metric)) and probes.dtype == np.int32
    want_s, want_i = P.search(q, rows, ids, cent, cb, k, nprobe, metric, exclude=ex)
    assert np.array_equal(got, want_i) and np.array_equal(_np(got_v), want_i)
    assert np.array_equal(_bits(s64), _bits(want_s))
    assert np.array_equal(_bits(val), _bits(P.values(want_s, metric)))
    return got, probes


# ---- the quantiser and the tables --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("dim, m", [(16, 4), (64, 16), (256, 64), (2048, 4)])
def test_tables_equal_the_sequential_sums(dim, m, metric):
    from mirx.index import pq_tables
    rng = np.random.default_rng(dim + m)
    cb = rng.standard_normal((m, 256, dim // m)).astype(F4)
    for nq in (1, 5):
        q = (rng.standard_normal((nq, dim)) + 1e3).astype(F4)             # off by 1e3: d * d is inexact, the rounding shows
        want = P.tables(q, cb, metric)
        got = pq_tables(torch.from_numpy(q).cuda(), torch.from_numpy(cb).cuda(), metric)
        assert got.dtype == torch.float64 and tuple(got.shape) == (nq, m, 256)
        assert np.array_equal(_bits(_np(got)), _bits(want))
    if metric == "L2" and hasattr(math, "fma"):                           # a fused L2 has other bits: the restatement tells them apart
        fused = P.tables(q[-1:], cb[:1], metric, fused=math.fma)
        assert (_bits(fused) != _bits(want[-1:, :1])).any()
    assert pq_tables(torch.empty((0, dim), device="cuda"), torch.from_numpy(cb).cuda(), metric).shape == (0, m, 256)


def test_encode_ties_and_decode():
    from mirx.index import pq_encode, pq_decode
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((300, 32)).astype(F4)
    cb = _codebooks(rows, 8, 5)
    cb[2, 200] = cb[2, 17]                                                # a duplicated codeword: the lower twin wins
    cb[0, 9] = [0.001, 0, 0, 0]
    cb[0, 5] = [-0.001, 0, 0, 0]
    rows[7, :4] = 0                                                       # equidistant from codewords 5 and 9, nearest to both
    pick = np.random.default_rng(5).choice(300, 256, replace=False)
    rows[pick[17], 8:12] = cb[2, 17]                                      # exactly on the duplicated codeword
    want = P.encode(rows, cb)
    assert want[7, 0] == 5 and want[pick[17], 2] == 17 and (want[:, 2] != 200).all()
    got = pq_encode(torch.from_numpy(rows).cuda(), torch.from_numpy(cb).cuda())
    assert got.dtype == torch.uint8 and np.array_equal(_np(got), want)
    dec = pq_decode(got, torch.from_numpy(cb).cuda())
    assert np.array_equal(_bits(_np(dec)), _bits(P.decode(want, cb)))
    assert np.array_equal(_np(pq_encode(dec, torch.from_numpy(cb).cuda())), want)
    assert pq_encode(torch.empty((0, 32), device="cuda"), torch.from_numpy(cb).cuda()).shape == (0, 8)


def test_train_codebooks_equals_the_restatement():
    from mirx.index import IvfPqIndex
    rows = np.random.default_rng(9).standard_normal((600, 16)).astype(F4)
    a, b = IvfPqIndex(16, "L2", nlist=4, m=4), IvfPqIndex(16, "COSINE", nlist=4, m=4)
    with pytest.raises(_lib().MirxError, match=r"\(-4\).*codebooks are not fixed"):
        a.codebooks
    with pytest.raises(ValueError, match="256"):
        a.train_codebooks(torch.from_numpy(rows[:255]), 3)
    a.train_codebooks(torch.from_numpy(rows), 3)
    b.train_codebooks(torch.from_numpy(rows).cuda(), 3)                   # host and device rows, either metric: always L2
    want = P.train_codebooks(rows, 4, 3)
    assert np.array_equal(_bits(_np(a.codebooks)), _bits(want)) and np.array_equal(_bits(_np(b.codebooks)), _bits(want))
    a.train_codebooks(torch.from_numpy(rows), 3)                          # a second call: equal bytes
    assert np.array_equal(_bits(_np(a.codebooks)), _bits(want))
    with pytest.raises(ValueError):
        a.set_codebooks(want[:, :255])


# ---- the scan ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("m", [4, 8, 16, 64])
def test_forced_lists_every_list_edge(m, metric):
    L = _lib()
    lib = L.load()
    ir = lib.mirx_ivf_pq_item_rows()
    dim = 4 * m
    rows, ids, cent, base = forced(SIZES, dim, metric, 100 + m, 0.02)
    cb = _codebooks(rows, m, m)
    ivf = _pq(rows, ids, cent, cb, metric)
    assert lib.mirx_ivf_kind(ivf._h) == L.IVF_PQ == 2 and lib.mirx_ivf_pq_m(ivf._h) == m
    _layout(ivf, rows, ids, cent, cb, metric)
    assert ivf.list_sizes().tolist() == SIZES and len(ivf) == sum(SIZES)
    assert np.array_equal(_np(ivf.assign(torch.from_numpy(rows))), R.assign(rows, cent, metric))
    assert np.array_equal(_bits(_np(ivf.tables(torch.from_numpy(rows[:2])))), _bits(P.tables(rows[:2], cb, metric)))
    rng = np.random.default_rng(m + 1)
    near = lambda l, n: (base[l] + 0.02 * rng.standard_normal((n, dim))).astype(F4)
    sizes = np.asarray(SIZES)
    for nq in (1, 2, 17):                                                 # all probing list 0
        got, probes = _check(ivf, rows, ids, cent, cb, metric, near(0, nq), 10, 1)
        assert (probes == 0).all()
        assert ivf.last_stats() == {"nq": nq, "rows_scored": nq * SIZES[0], "pairs": nq, "work_items": nq, "batches": 1}
    # queries spread over the lists; list 1 (empty) is probed together with list 0
    q = np.concatenate([near(0, 3)] + [near(l, 2) for l in (2, 3, 4, 5)])
    lists = R.assign(rows, cent, metric)
    ex = np.full(q.shape[0], -1, dtype=np.int64)
    ex[0] = ids[np.flatnonzero(lists == 0)[0]]                            # inside a probed list (an equal row: its twin must stay)
    ex[1] = ids[np.flatnonzero(lists == 6)[0]]                            # in a list the query does not probe
    ex[2] = 7                                                             # no row has this id
    for k in (1, 10, 300):
        got, probes = _check(ivf, rows, ids, cent, cb, metric, q, k, 2, ex)
        assert ex[0] not in got[0] and (probes[:3, :2] == [0, 1]).all()
        n_q = sizes[probes].sum(axis=1)
        assert ivf.last_stats() == {"nq": q.shape[0], "rows_scored": int(n_q.sum()), "pairs": 2 * q.shape[0],
                                    "work_items": int((-(-n_q // ir)).sum()), "batches": 1}
    # the equal rows of list 0: equal scores, the lower id first
    twin = np.flatnonzero(lists == 0)[:2]
    got, _ = _check(ivf, rows, ids, cent, cb, metric, rows[twin[:1]], 300, 1)
    at = [got[0].tolist().index(int(ids[t])) for t in twin]
    assert ids[twin[1]] < ids[twin[0]] and at[1] + 1 == at[0]
    # every list probed, in two internal batches: the ADC ranking of all rows
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, (8 * sum(SIZES) + 2048 * m) * (q.shape[0] - 2))
    got, _ = _check(ivf, rows, ids, cent, cb, metric, q, 10, len(SIZES), ex)
    assert ivf.last_stats()["batches"] == 2 and ivf.last_stats()["rows_scored"] == q.shape[0] * sum(SIZES)
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, 0)
    far, _ = _check(ivf, rows, ids, cent, cb, metric, q, 10, 1000, ex)
    assert np.array_equal(far, got) and ivf.last_stats()["batches"] == 1


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("m", [8, 16])                                    # 4-byte and 16-byte code loads
def test_compact_rows_on_the_item_edges(m, metric):
    lib = _lib().load()
    ir = lib.mirx_ivf_pq_item_rows()
    assert 2 * ir + 1 <= 3000
    sizes = [ir - 1, 1, 1, ir]
    dim = 64
    rows, ids, cent, base = forced(sizes, dim, metric, 77, 0.02)
    cb = _codebooks(rows, m, 3)
    ivf = _pq(rows, ids, cent, cb, metric)
    assert ivf.list_sizes().tolist() == sizes
    mix = lambda w: _unit(np.asarray(w, dtype=F4)[None] @ base)            # probes in the order of the weights
    # list 0 | 0, 1 | 0, 1, 2 | 3, 0, 1, 2: ir - 1, ir, ir + 1 and 2 ir + 1 entries; a list boundary inside an item (after
    # ir - 1 entries) and on an item boundary (list 3's ir entries first)
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
    """The scan's grid is persistent: CUs x (1 or 2) workgroups, each taking a contiguous run of ceil(items / grid) items.  With
    more than twice as many items as workgroups a workgroup goes from item to item inside a query, from query to query (reloading
    the table behind a barrier that lanes without an entry must reach too), and over queries without entries in the middle of
    its run; runs start inside a query's items, so one query's items straddle two workgroups."""
    lib = _lib().load()
    ir = lib.mirx_ivf_pq_item_rows()
    dim = 4 * m
    sizes = [ir - 1, 1, 1, ir]
    rows, ids, cent, base = forced(sizes, dim, metric, 300 + m, 0.02)
    rng = np.random.default_rng(m)
    far = _unit(rng.standard_normal((1, dim)))                            # four empty lists, their centroids side by side
    cent = np.ascontiguousarray(np.concatenate([cent, (3 * far + 0.001 * rng.standard_normal((4, dim))).astype(F4)]), dtype=F4)
    if metric == "COSINE":
        cent[4:] = _unit(cent[4:])
    assert np.bincount(R.assign(rows, cent, metric), minlength=8).tolist() == sizes + [0, 0, 0, 0]
    cb = _codebooks(rows, m, 7)
    ivf = _pq(rows, ids, cent, cb, metric)
    nq = 1100
    target = rng.integers(0, 5, nq)                                       # 4: the empty lists
    target[[0, 1, 500, 501, 502, nq - 1]] = 4                             # also first, last and consecutive
    centre = np.concatenate([base, cent[4:5]])[target]
    q = (centre + 0.02 * rng.standard_normal((nq, dim))).astype(F4)
    ex = np.where(rng.integers(0, 3, nq) == 0, ids[rng.integers(0, ids.size, nq)], -1).astype(np.int64)
    got, probes = _check(ivf, rows, ids, cent, cb, metric, q, 10, 4, ex)
    n_q = np.asarray(sizes + [0, 0, 0, 0])[probes].sum(axis=1)
    assert (n_q[target == 4] == 0).all() and (got[target == 4] == -1).all()          # queries without entries, hence without items
    items = -(-n_q // ir)
    assert {0, 3} <= set(items.tolist())                                  # three items per query as well
    st = ivf.last_stats()
    assert st == {"nq": nq, "rows_scored": int(n_q.sum()), "pairs": 4 * nq, "work_items": int(items.sum()), "batches": 1}
    grid = 2 * torch.cuda.get_device_properties(0).multi_processor_count  # the larger of the two grids
    assert st["work_items"] > 2 * grid, (st["work_items"], grid)


# ---- state and layout --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_add_in_two_calls_remove_state_errors_and_determinism(metric):
    from mirx.index import IvfPqIndex, IvfFlatIndex, IvfSq8Index
    L = _lib()
    dim, m = 32, 8
    rows, ids, cent, base = forced(SIZES, dim, metric, 21, 0.02)
    n = rows.shape[0]
    cb = _codebooks(rows, m, 2)
    q = np.concatenate([(base[l] + F4(0.01)).astype(F4)[None] for l in (0, 3, 5, 6)])
    qt = torch.from_numpy(q)
    ivf = IvfPqIndex(dim, metric, nlist=len(SIZES), m=m)
    with pytest.raises(L.MirxError, match=r"\(-4\).*centroids are not fixed"):
        ivf.add(torch.from_numpy(rows))
    ivf.set_centroids(torch.from_numpy(cent))
    with pytest.raises(L.MirxError, match=r"\(-4\).*codebooks are not fixed"):
        ivf.add(torch.from_numpy(rows))
    assert len(ivf) == 0
    ivf.set_codebooks(cb)
    ivf.add(torch.from_numpy(rows[:200]), torch.from_numpy(ids[:200]))
    ivf.add(torch.from_numpy(rows[200:]).cuda(), torch.from_numpy(ids[200:]).cuda())
    whole = _pq(rows, ids, cent, cb, metric)                              # one call: a second build
    same = lambda a, b: all(np.array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8)) for x, y in zip(a, b))
    assert same(ivf.codes(), whole.codes()) and same(ivf.reconstruct(), whole.reconstruct())
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
    assert same(ivf.codes(), whole.codes()) and same(ivf.search(qt, 20, 3, return_f64=True), before)
    assert np.array_equal(_np(ivf.centroids), cent) and np.array_equal(_np(ivf.codebooks), cb)
    # remove: then the answer of a fresh index over the survivors
    gone = np.concatenate([ids[5:60], ids[5:20], ids[n - 40:], [123456789]])
    assert ivf.remove(torch.from_numpy(gone)) == 55 + 40
    keep = np.ones(n, bool)
    keep[5:60] = keep[n - 40:] = False
    fresh = _pq(rows[keep], ids[keep], cent, cb, metric)
    assert len(ivf) == n - 95 and same(ivf.codes(), fresh.codes())
    _layout(ivf, rows[keep], ids[keep], cent, cb, metric)
    for nprobe in (1, 3, len(SIZES)):
        _check(ivf, rows[keep], ids[keep], cent, cb, metric, q, 20, nprobe)
    # emptied, it takes new codebooks and new centroids again
    assert ivf.remove(torch.from_numpy(ids)) == n - 95 and len(ivf) == 0
    ivf.set_codebooks(cb + 1)
    ivf.set_centroids(torch.from_numpy(np.ascontiguousarray(base[::-1])))
    assert ivf.codes()[0].shape == (0, m)
    # the PQ calls on FLAT and SQ8 handles, the SQ8 calls on a PQ handle: MIRX_EINVAL
    lib = L.load()
    buf = torch.zeros(256 * dim, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    for other in (IvfFlatIndex(dim, metric, nlist=4), IvfSq8Index(dim, metric, nlist=4)):
        assert lib.mirx_ivf_pq_train(other._h, p, 256, 1, None) == -1 and lib.mirx_ivf_pq_m(other._h) == -1
        assert lib.mirx_ivf_pq_set_codebooks(other._h, p) == -1 and lib.mirx_ivf_pq_get_codebooks(other._h, p) == -1
    assert lib.mirx_ivf_sq8_train(ivf._h, p, 1, None) == -1 and lib.mirx_ivf_sq8_set_range(ivf._h, p, p) == -1
    assert lib.mirx_ivf_sq8_get_range(ivf._h, p, p) == -1


def test_collection_route():
    from mirx.retriever import Collection
    from mirx.index import IvfPqIndex
    rows = _unit(np.random.default_rng(0).standard_normal((1200, 32)))
    rng = np.random.default_rng(1)
    q = _unit(rows[rng.choice(1200, 12, replace=False)] + 0.3 * rng.standard_normal((12, 32)).astype(F4))
    labels = [f"c{i % 3}" for i in range(1200)]
    paths = [f"p{i}.png" for i in range(1200)]
    params = {"metric_type": "COSINE", "index_type": "IVF_PQ", "params": {"nlist": 12, "m": 8}}
    approx, twin, small = Collection("apq", 32), Collection("tpq", 32), Collection("spq", 32)
    approx.create_index("embedding", params, approximate=True)
    twin.create_index("embedding", {"metric_type": "COSINE", "index_type": "IVF_FLAT", "params": {"nlist": 12}}, approximate=True)
    small.create_index("embedding", params, approximate=True)
    for col in (approx, twin):
        col.insert([paths, labels, rows])
        col.load()
    assert type(approx._ivf) is IvfPqIndex and approx._ivf.m == 8
    ivf = IvfPqIndex(32, "COSINE", nlist=12, m=8)
    ivf.train(torch.from_numpy(rows))
    ivf.add(torch.from_numpy(rows))
    cent, cb = _np(ivf.centroids), _np(ivf.codebooks)
    assert np.array_equal(cent, R.train(rows, 12, 10, "COSINE")) and np.array_equal(_bits(cb), _bits(P.train_codebooks(rows, 8, 10)))
    pairs = lambda hits: [[(h.id, h.distance) for h in hs] for hs in hits]

    def direct(index, nprobe, ex=None):
        sc, ids = index.search(torch.from_numpy(q), 10, nprobe, exclude_ids=ex)
        return [[(int(i), float(v)) for i, v in zip(a, b) if i >= 0] for a, b in zip(_np(ids), _np(sc))]

    p2 = {"metric_type": "COSINE", "params": {"nprobe": 2}}
    got = pairs(approx.search(q, param=p2, limit=10))
    assert got == direct(ivf, 2)
    _check(ivf, rows, None, cent, cb, "COSINE", q, 10, 2)
    flat_got = pairs(twin.search(q, param=p2, limit=10))
    assert all([i for i, _ in a] != [i for i, _ in b] for a, b in zip(got, flat_got))       # not the IVF_FLAT twin's ids
    ex = list(range(12))
    assert pairs(approx.search(q, param=p2, limit=10, exclude_ids=ex)) == direct(ivf, 2, ex)
    # every other call stays exact, over the ORIGINAL rows: no nprobe, an expr
    assert pairs(approx.search(q, limit=10)) == pairs(twin.search(q, limit=10))
    e = 'label == "c1"'
    assert pairs(approx.search(q, param=p2, limit=10, expr=e)) == pairs(twin.search(q, limit=10, expr=e))
    # below max(nlist, 256) rows the collection stays exact
    small.insert([paths[:255], labels[:255], rows[:255]])
    small.load()
    assert small._ivf is None and small._ensure_ivf() is None
    # after delete and insert the lists are rebuilt with the kept centroids and the kept codebooks
    approx.delete("id in [0, 1, 2, 3, 4, 5, 6, 7]")
    late = (10 * q[:1]).astype(F4)
    approx.insert([["n.png"], ["c0"], late])
    keep = np.arange(8, 1200)
    again = IvfPqIndex(32, "COSINE", nlist=12, m=8)
    again.set_centroids(torch.from_numpy(cent))
    again.set_codebooks(cb)
    again.add(torch.from_numpy(np.concatenate([rows[keep], late])), torch.from_numpy(np.concatenate([keep, [1200]])))
    assert pairs(approx.search(q, param=p2, limit=10)) == direct(again, 2)
    assert np.array_equal(_np(approx._ivf.centroids), cent) and np.array_equal(_bits(_np(approx._ivf.codebooks)), _bits(cb))
    codes, cid, _ = approx._ivf.codes()
    assert np.array_equal(_np(codes)[_np(cid) == 1200][0], P.encode(late, cb)[0])
