"""IVF_SQ8 on the device (mirx.index.IvfSq8Index, Collection.create_index({"index_type": "IVF_SQ8"}, approximate=True)).

The rule: an IVF_SQ8 answer is the IVF_FLAT answer over the DECODED rows.  Every comparison is bit for bit -- ids, fp64 ranking
scores, fp32 reported values -- against FlatIndex over reconstruct()'s rows under the mask "the row's list is probed"
(tests/test_ivf_gpu.py's _check, unchanged), and the quantiser itself against tests/_sq8_ref.py, byte for byte.  The lists come
from the ORIGINAL rows: tests/_ivf_ref.py's assign on the CPU.

Shapes are tests/test_ivf_gpu.py's, on the same block edges (lists of 0, 1, 63, 64, 65, 120, 257 rows; QT - 1 .. 2 QT + 1 queries
on one list; dims 20 .. 1100: a partial last 4-code word, 1 / 2 / 4 / 8 chunks per lane, the padding)."""
import ctypes

import numpy as np
import pytest
import torch

import _ivf_ref as R
import _sq8_ref as Q
import test_ivf_gpu as T
from _ivf_cases import SIZES, _lib, _np, _unit, forced

pytestmark = pytest.mark.gpu

F4 = np.float32


def _sq8(rows, ids, cent, metric, vmin=None, scale=None):
    """an IvfSq8Index with the given centroids, the range trained on `rows` (or given), holding rows"""
    from mirx.index import IvfSq8Index
    ivf = IvfSq8Index(rows.shape[1], metric, nlist=cent.shape[0])
    ivf.set_centroids(torch.from_numpy(cent))
    if vmin is None:
        ivf.train_range(torch.from_numpy(rows))
    else:
        ivf.set_range(torch.from_numpy(vmin), torch.from_numpy(scale))
    ivf.add(torch.from_numpy(rows), None if ids is None else torch.from_numpy(ids))
    return ivf


def _oracle(ivf, rows, ids, cent, metric):
    """(flat index over the decoded rows, flat index over the centroids, the lists, all in the master's order) after checking
    that codes / reconstruct / lists are the restatement's of the ORIGINAL rows"""
    vmin, scale = (_np(t) for t in ivf.range)
    codes, cid, lists = (_np(t) for t in ivf.codes())
    dec, did = (_np(t) for t in ivf.reconstruct())
    ids = np.arange(rows.shape[0], dtype=np.int64) if ids is None else ids
    assert np.array_equal(cid, did) and sorted(cid.tolist()) == sorted(ids.tolist())
    where = {int(v): i for i, v in enumerate(ids)}
    src = np.array([where[int(v)] for v in cid], dtype=np.int64)          # master position -> caller's row
    assert np.array_equal(lists, R.assign(rows, cent, metric)[src])       # the list of every id: from the original row
    assert (np.diff(lists) >= 0).all()                                    # list-major
    for l in np.unique(lists):                                            # insertion order inside a list
        assert (np.diff(src[lists == l]) > 0).all()
    assert np.array_equal(codes, Q.encode(rows, vmin, scale)[src])
    assert np.array_equal(dec.view(np.uint32), Q.decode(codes, vmin, scale).view(np.uint32))
    return T._flat(dec, cid, metric), T._flat(cent, None, metric), lists


def _bits_differ(a, b):
    """per query: does any of its fp64 scores differ in bits"""
    return (_np(a).view(np.uint64) != _np(b).view(np.uint64)).any(axis=1)


# ---- the quantiser -------------------------------------------------------------------------------------------------------------

def test_encode_decode_at_the_rounding_edges():
    from mirx.index import sq8_encode, sq8_decode
    rng = np.random.default_rng(0)
    dim = 37                                                              # no multiple of 4: a partial last word
    vmin = rng.standard_normal(dim).astype(F4)
    scale = (np.abs(rng.standard_normal(dim)) / 255 + 1e-4).astype(F4)
    vmin[0], scale[0] = 1.0, 0.25                                         # exact in binary: t hits .5 exactly
    vmin[1], scale[1] = -3.0, 2.0 ** -10
    scale[5] = 0.0                                                        # a zero-scale column
    cs = np.arange(256, dtype=np.float64)
    mid = (vmin.astype(np.float64) + (cs[:, None] + 0.5) * scale.astype(np.float64)).astype(F4)     # at / next to a boundary
    rows = np.concatenate([mid, np.nextafter(mid, F4(-np.inf)), np.nextafter(mid, F4(np.inf)),
                           np.nextafter(np.nextafter(mid, F4(np.inf)), F4(np.inf)),
                           (vmin - 5)[None], (vmin + 300 * scale + 5)[None],                         # clamping
                           np.full((1, dim), np.nan, F4), np.full((1, dim), np.inf, F4), np.full((1, dim), -np.inf, F4),
                           rng.standard_normal((40, dim)).astype(F4)]).astype(F4)
    want = Q.encode(rows, vmin, scale)
    t0 = (rows[:256, :2].astype(np.float64) - vmin[:2]) / scale[:2]
    assert np.array_equal(t0, cs[:, None] + 0.5 + 0 * t0)                 # columns 0 and 1 really are exact ties
    assert np.array_equal(want[:256, 0], np.minimum(cs + 1, 255)) and np.array_equal(want[256:512, 0], cs)   # ties go up
    assert (want[:, 5] == 0).all() and (want[-45] == 0).all() and (want[-44][scale > 0] == 255).all()
    assert (want[-43] == 0).all() and (want[-42][scale > 0] == 255).all() and (want[-41] == 0).all()
    dv, ds = torch.from_numpy(vmin).cuda(), torch.from_numpy(scale).cuda()
    got = sq8_encode(torch.from_numpy(rows).cuda(), dv, ds)
    assert got.dtype == torch.uint8 and np.array_equal(_np(got), want)
    every = np.repeat(np.arange(256, dtype=np.uint8)[:, None], dim, axis=1)
    dec = sq8_decode(torch.from_numpy(every).cuda(), dv, ds)
    assert np.array_equal(_np(dec).view(np.uint32), Q.decode(every, vmin, scale).view(np.uint32))
    assert np.array_equal(_np(sq8_encode(dec, dv, ds)), np.where(scale == 0, 0, every))
    assert sq8_encode(torch.empty((0, dim), device="cuda"), dv, ds).shape == (0, dim)


@pytest.mark.parametrize("n, dim", [(1, 20), (700, 100), (3001, 300)])   # one row; below / above the 1024 partials
def test_train_range_equals_the_restatement(n, dim):
    from mirx.index import IvfSq8Index
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, dim)).astype(F4)
    rows[:, 3] = F4(0.5)                                                  # constant: scale 0
    rows[:, 4] = F4(-0.0)
    rows[n // 2, 4] = F4(0.0)                                             # both zeros: the stored minimum is +0
    rows[:, 6] = np.nan                                                   # a column without a number
    rows[n // 3, 7] = np.nan                                              # NaN is ignored
    a, b = IvfSq8Index(dim, "L2", nlist=4), IvfSq8Index(dim, "L2", nlist=4)
    with pytest.raises(_lib().MirxError, match=r"\(-4\).*range is not fixed"):
        a.range
    a.train_range(torch.from_numpy(rows))
    b.train_range(torch.from_numpy(rows).cuda())                          # host and device rows, two calls: equal bits
    vmin, scale = Q.train_range(rows)
    for ix in (a, b):
        gv, gs = (_np(t) for t in ix.range)
        assert np.array_equal(gv.view(np.uint32), vmin.view(np.uint32)) and np.array_equal(gs.view(np.uint32), scale.view(np.uint32))
    assert scale[3] == 0 and scale[4] == 0 and vmin[6] == 0 and scale[6] == 0 and (n == 1 or scale[7] > 0)
    a.set_range(vmin + 1, torch.from_numpy(scale * 2).cuda())             # a caller's own range, host and device
    gv, gs = (_np(t) for t in a.range)
    assert np.array_equal(gv, vmin + 1) and np.array_equal(gs, scale * 2)
    with pytest.raises(ValueError):
        a.set_range(vmin[:-1], scale)
    with pytest.raises(ValueError):
        a.train_range(torch.empty((0, dim)))


# ---- the hot path ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("dim", [20, 64, 100, 256, 300, 1024, 1100])
def test_forced_lists_every_block_edge(dim, metric):
    L = _lib()
    lib = L.load()
    qt, rb = lib.mirx_ivf_query_tile(dim), lib.mirx_ivf_row_block()
    assert rb + 1 in SIZES
    rows, ids, cent, base = forced(SIZES, dim, metric, dim, 0.02)
    ivf = _sq8(rows, ids, cent, metric)
    assert lib.mirx_ivf_kind(ivf._h) == L.IVF_SQ8
    flat, cflat, lists = _oracle(ivf, rows, ids, cent, metric)
    assert ivf.list_sizes().tolist() == SIZES and len(ivf) == sum(SIZES)
    assert np.array_equal(_np(ivf.assign(torch.from_numpy(rows))), R.assign(rows, cent, metric))
    twin = T._ivf(rows, ids, cent, metric)                                # IVF_FLAT, the same centroids: the same lists
    assert twin.list_sizes().tolist() == SIZES
    rng = np.random.default_rng(dim + 1)
    near0 = lambda m: (base[0] + 0.02 * rng.standard_normal((m, dim))).astype(F4)
    for m in (1, qt - 1, qt, qt + 1, 2 * qt + 1):        # that many queries, all probing list 0; no query probes the other lists
        if m < 1:
            continue
        got, probes = T._check(ivf, flat, cflat, lists, near0(m), 10, 1)
        assert (probes == 0).all()
        st = ivf.last_stats()
        assert st == {"nq": m, "rows_scored": m * SIZES[0], "pairs": m, "work_items": 2 * -(-m // qt), "batches": 1}
    # queries spread over the lists; list 1 (empty) is probed together with list 0
    q = np.concatenate([near0(3)] + [(base[l] + 0.02 * rng.standard_normal((2, dim))).astype(F4) for l in (2, 3, 4, 5)])
    ex = np.full(q.shape[0], -1, dtype=np.int64)
    ex[0] = ids[np.flatnonzero(R.assign(rows, cent, metric) == 0)[0]]     # inside a probed list
    ex[1] = ids[np.flatnonzero(R.assign(rows, cent, metric) == 6)[0]]     # in a list the query does not probe
    ex[2] = 7                                                             # no row has this id
    got, probes = T._check(ivf, flat, cflat, lists, q, 10, 2, ex)
    assert ex[0] not in got[0] and (probes[:3, :2] == [0, 1]).all()
    st = ivf.last_stats()
    sizes = np.asarray(SIZES)
    assert st["pairs"] == 2 * q.shape[0] and st["rows_scored"] == int(sizes[probes].sum())
    assert st["work_items"] == sum(-(-int(sizes[l]) // rb) * -(-int((probes == l).sum()) // qt) for l in range(len(SIZES)))
    # not the IVF_FLAT answer: every query's score bits differ
    qt_ = torch.from_numpy(q)
    s8 = ivf.search(qt_, 10, 2, exclude_ids=torch.from_numpy(ex), return_f64=True)[0]
    s32 = twin.search(qt_, 10, 2, exclude_ids=torch.from_numpy(ex), return_f64=True)[0]
    assert _bits_differ(s8, s32).all()
    # every list probed: the flat index's answer over the decoded rows, in two internal batches
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, 8 * sum(SIZES) * (q.shape[0] - 2))
    got, _ = T._check(ivf, flat, cflat, lists, q, 10, len(SIZES), ex)
    assert ivf.last_stats()["batches"] == 2
    e64, eid = flat.search(qt_, 10, exclude_ids=torch.from_numpy(ex), return_f64=True)
    assert np.array_equal(got, _np(eid))
    assert np.array_equal(_np(ivf.search(qt_, 10, 1000, exclude_ids=torch.from_numpy(ex), return_f64=True)[0]), _np(e64))


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("k", [1, 10, 300])
def test_k_edges_and_padding(k, metric):
    rows, ids, cent, base = forced(SIZES, 64, metric, 5, 0.02)
    ivf = _sq8(rows, ids, cent, metric)
    flat, cflat, lists = _oracle(ivf, rows, ids, cent, metric)
    rng = np.random.default_rng(6)
    q = np.concatenate([(base[l] + 0.02 * rng.standard_normal((2, 64))).astype(F4) for l in (0, 2, 3)])
    for nprobe in (1, 2, len(SIZES)):
        got, probes = T._check(ivf, flat, cflat, lists, q, k, nprobe)
        if nprobe == 1:                                   # k above the probed rows: (-1, -inf) behind them
            for i, l in enumerate((0, 0, 2, 2, 3, 3)):
                assert (got[i] >= 0).sum() == min(k, SIZES[l])


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_recipe_is_the_restatement_and_not_ivf_flat(metric):
    """tests/test_ivf_cpu.py's recipe, trained on the device: centroids, range, lists and answers are the restatement's; the
    answer is neither IVF_FLAT's nor the one an index that assigned from the decoded rows would give"""
    from mirx.index import IvfSq8Index, IvfFlatIndex
    rows = _unit(np.random.default_rng(0).standard_normal((3000, 32)))
    rng = np.random.default_rng(1)
    q = _unit(rows[rng.choice(3000, 64, replace=False)] + 0.3 * rng.standard_normal((64, 32)).astype(F4))
    ivf = IvfSq8Index(32, metric, nlist=24)
    ivf.train(torch.from_numpy(rows), iters=10)           # centroids and range from the same sample (here: every row)
    ivf.add(torch.from_numpy(rows))
    cent = _np(ivf.centroids)
    vmin, scale = (_np(t) for t in ivf.range)
    assert np.array_equal(cent, R.train(rows, 24, 10, metric))
    rv, rs = Q.train_range(rows)
    assert np.array_equal(vmin, rv) and np.array_equal(scale, rs)
    flat, cflat, lists = _oracle(ivf, rows, None, cent, metric)
    orig = R.assign(rows, cent, metric)
    moved = int((R.assign(Q.decode(Q.encode(rows, vmin, scale), vmin, scale), cent, metric) != orig).sum())
    assert moved >= 1                                     # so _oracle's list check tells the two assignments apart
    assert np.array_equal(ivf.list_sizes(), np.bincount(orig, minlength=24))
    got, _ = T._check(ivf, flat, cflat, lists, q, 10, 2)
    s_ref, i_ref = Q.search(q, rows, None, cent, vmin, scale, 10, 2, metric)
    qt = torch.from_numpy(q)
    s8 = ivf.search(qt, 10, 2, return_f64=True)[0]
    assert np.array_equal(got, i_ref) and np.array_equal(_np(s8), s_ref)
    twin = IvfFlatIndex(32, metric, nlist=24)
    twin.set_centroids(torch.from_numpy(cent))
    twin.add(torch.from_numpy(rows))
    assert _bits_differ(s8, twin.search(qt, 10, 2, return_f64=True)[0]).all()
    # nprobe = nlist: the unmasked flat search of the decoded rows
    full, _ = T._check(ivf, flat, cflat, lists, q, 10, 24)
    e64, eid = flat.search(qt, 10, return_f64=True)
    assert np.array_equal(full, _np(eid)) and np.array_equal(_np(ivf.search(qt, 10, 24, return_f64=True)[0]), _np(e64))
    assert ivf.last_stats()["rows_scored"] == 64 * 3000
    exact = _np(T._flat(rows, None, metric).search(qt, 10)[1])
    differ = sum(not np.array_equal(a, b) for a, b in zip(full, exact))
    print(f"{metric}: id lists at nprobe = nlist that differ from the exact ones over the original rows: {differ} of 64")
    assert differ >= 24, differ


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_add_in_two_calls_remove_state_errors_and_determinism(metric):
    from mirx.index import IvfSq8Index, IvfFlatIndex
    L = _lib()
    rows, ids, cent, base = forced(SIZES, 100, metric, 21, 0.02)
    n = rows.shape[0]
    vmin, scale = Q.train_range(rows)
    q = torch.from_numpy(np.concatenate([(base[l] + F4(0.01)).astype(F4)[None] for l in (0, 3, 5, 6)]))
    ivf = IvfSq8Index(100, metric, nlist=len(SIZES))
    with pytest.raises(L.MirxError, match=r"\(-4\).*centroids are not fixed"):
        ivf.add(torch.from_numpy(rows))
    ivf.set_centroids(torch.from_numpy(cent))
    with pytest.raises(L.MirxError, match=r"\(-4\).*range is not fixed"):
        ivf.add(torch.from_numpy(rows))
    assert len(ivf) == 0
    ivf.set_range(vmin, scale)
    ivf.add(torch.from_numpy(rows[:200]), torch.from_numpy(ids[:200]))
    ivf.add(torch.from_numpy(rows[200:]).cuda(), torch.from_numpy(ids[200:]).cuda())
    whole = _sq8(rows, ids, cent, metric)                 # one call, the range trained on the device: a second build
    same = lambda a, b: all(np.array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8)) for x, y in zip(a, b))
    assert same(ivf.codes(), whole.codes()) and same(ivf.reconstruct(), whole.reconstruct()) and same(ivf.range, whole.range)
    for nprobe in (1, 3):
        assert same(ivf.search(q, 20, nprobe, return_f64=True), whole.search(q, 20, nprobe, return_f64=True))
    # an index that holds rows keeps its centroids and its range: MIRX_ESTATE, nothing changed
    before = ivf.search(q, 20, 3, return_f64=True)
    for call in (lambda: ivf.set_range(vmin + 1, scale), lambda: ivf.train_range(torch.from_numpy(rows)),
                 lambda: ivf.set_centroids(torch.from_numpy(np.ascontiguousarray(base[::-1]))),
                 lambda: ivf.train(torch.from_numpy(rows), iters=1)):
        with pytest.raises(L.MirxError, match=r"\(-4\).*holds rows"):
            call()
    assert same(ivf.codes(), whole.codes()) and same(ivf.range, whole.range) and same(ivf.search(q, 20, 3, return_f64=True), before)
    assert np.array_equal(_np(ivf.centroids), cent)
    # remove: then the answer of a fresh index over the survivors, and the masked flat search of its decoded rows
    gone = np.concatenate([ids[5:60], ids[5:20], ids[n - 40:], [123456789]])
    assert ivf.remove(torch.from_numpy(gone)) == 55 + 40
    keep = np.ones(n, bool)
    keep[5:60] = keep[n - 40:] = False
    fresh = _sq8(rows[keep], ids[keep], cent, metric, vmin, scale)
    assert len(ivf) == n - 95 and same(ivf.codes(), fresh.codes())
    flat, cflat, lists = _oracle(ivf, rows[keep], ids[keep], cent, metric)
    for nprobe in (1, 3, len(SIZES)):
        T._check(ivf, flat, cflat, lists, _np(q), 20, nprobe)
    # emptied, it takes a new range and new centroids again
    assert ivf.remove(torch.from_numpy(ids)) == n - 95 and len(ivf) == 0
    ivf.set_range(vmin + 1, scale)
    ivf.set_centroids(torch.from_numpy(np.ascontiguousarray(base[::-1])))
    assert ivf.codes()[0].shape == (0, 100)
    # the SQ8 calls on an IVF_FLAT handle: MIRX_EINVAL
    plain = IvfFlatIndex(100, metric, nlist=len(SIZES))
    buf = torch.zeros(100, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    lib = L.load()
    assert lib.mirx_ivf_kind(plain._h) == L.IVF_FLAT
    assert lib.mirx_ivf_sq8_set_range(plain._h, p, p) == -1 and lib.mirx_ivf_sq8_get_range(plain._h, p, p) == -1
    assert lib.mirx_ivf_sq8_train(plain._h, p, 1, None) == -1
    assert lib.mirx_ivf_get_codes(plain._h, p, None, None) == -1 and lib.mirx_ivf_reconstruct(plain._h, p, None) == -1


def test_collection_route():
    from mirx.retriever import Collection
    from mirx.index import IvfSq8Index
    from mirx.nih import create_nih_collection
    rows = _unit(np.random.default_rng(0).standard_normal((1200, 32)))
    rng = np.random.default_rng(1)
    q = _unit(rows[rng.choice(1200, 12, replace=False)] + 0.3 * rng.standard_normal((12, 32)).astype(F4))
    labels = [f"c{i % 3}" for i in range(1200)]
    paths = [f"p{i}.png" for i in range(1200)]
    params = {"metric_type": "COSINE", "index_type": "IVF_SQ8", "params": {"nlist": 12}}
    approx, twin = Collection("a8", 32), Collection("t32", 32)
    approx.create_index("embedding", params, approximate=True)
    twin.create_index("embedding", dict(params, index_type="IVF_FLAT"), approximate=True)
    for col in (approx, twin):
        col.insert([paths, labels, rows])
        col.load()
    assert type(approx._ivf) is IvfSq8Index
    ivf = IvfSq8Index(32, "COSINE", nlist=12)
    ivf.train(torch.from_numpy(rows))
    ivf.add(torch.from_numpy(rows))
    pairs = lambda hits: [[(h.id, h.distance) for h in hs] for hs in hits]

    def direct(index, nprobe, ex=None):
        sc, ids = index.search(torch.from_numpy(q), 10, nprobe, exclude_ids=ex)
        return [[(int(i), float(v)) for i, v in zip(a, b) if i >= 0] for a, b in zip(_np(ids), _np(sc))]

    p2 = {"metric_type": "COSINE", "params": {"nprobe": 2}}
    got = pairs(approx.search(q, param=p2, limit=10))
    flat_got = pairs(twin.search(q, param=p2, limit=10))
    assert got == direct(ivf, 2)
    assert all(a != b for a, b in zip(got, flat_got))                     # not the IVF_FLAT twin's answer, for any query
    ex = list(range(12))
    assert pairs(approx.search(q, param=p2, limit=10, exclude_ids=ex)) == direct(ivf, 2, ex)
    # every other call stays exact, over the ORIGINAL rows: no nprobe, an expr
    assert pairs(approx.search(q, limit=10)) == pairs(twin.search(q, limit=10))
    e = 'label == "c1"'
    assert pairs(approx.search(q, param=p2, limit=10, expr=e)) == pairs(twin.search(q, limit=10, expr=e))
    # after delete and insert the lists are rebuilt with the kept centroids and the kept range
    cent, (vmin, scale) = _np(ivf.centroids), ivf.range
    approx.delete("id in [0, 1, 2, 3, 4, 5, 6, 7]")
    late = (10 * q[:1]).astype(F4)                                        # outside the trained range: it clamps
    approx.insert([["n.png"], ["c0"], late])
    keep = np.arange(8, 1200)
    again = IvfSq8Index(32, "COSINE", nlist=12)
    again.set_centroids(torch.from_numpy(cent))
    again.set_range(vmin, scale)
    again.add(torch.from_numpy(np.concatenate([rows[keep], late])), torch.from_numpy(np.concatenate([keep, [1200]])))
    got = pairs(approx.search(q, param=p2, limit=10))
    assert got == direct(again, 2)
    assert np.array_equal(_np(approx._ivf.centroids), cent)
    assert all(np.array_equal(_np(a), _np(b)) for a, b in zip(approx._ivf.range, (vmin, scale)))
    codes, cid, _ = approx._ivf.codes()
    outside = (late[0] < _np(vmin)) | (late[0] > rows.max(axis=0))
    assert outside.sum() >= 8                                             # 10 x a unit row leaves the range in most columns
    new = _np(codes)[_np(cid) == 1200][0]
    assert np.array_equal(new, Q.encode(late, _np(vmin), _np(scale))[0]) and set(new[outside].tolist()) <= {0, 255}
    # the wrappers hand the type through
    nih = create_nih_collection("nih_sq8", index_type="IVF_SQ8", nlist=16, approximate=True)
    assert (nih._approx_nlist, nih._approx_type) == (16, "IVF_SQ8")
