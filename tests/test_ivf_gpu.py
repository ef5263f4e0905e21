"""IVF_FLAT on the device (mirx.index.IvfFlatIndex, Collection.create_index(approximate=True)).

Every comparison is bit for bit -- ids, fp64 ranking scores, fp32 reported values -- and the oracle is never the code under
test: FlatIndex over the centroids (assignment, probes), FlatIndex.search under the mask "the row's list is probed" (the IVF
answer), FlatIndex.search itself (nprobe = nlist), and tests/_ivf_ref.py on oracle.search (training).

Shapes sit on the edges of the list scan as built: a work item is mirx_ivf_row_block() = 256 rows of a list (64 per wave) times
up to QT = mirx_ivf_query_tile(dim) queries (16 up to dim 512, 8 at 1024, 7 at 1100), so the lists hold 0, 1, 63, 64, 65 and
257 rows and QT - 1, QT, QT + 1 and 2 QT + 1 queries probe one list; dims 20 .. 1100 cover the padding and the 1 / 2 / 4 / 8
chunks per lane."""
import numpy as np
import pytest
import torch

import _ivf_ref as R
from _ivf_cases import SIZES, _lib, _np, _unit, forced

pytestmark = pytest.mark.gpu


def _flat(rows, ids, metric):
    from mirx.index import FlatIndex
    ix = FlatIndex(rows.shape[1], metric)
    ix.add(torch.from_numpy(rows), None if ids is None else torch.from_numpy(ids))
    return ix


def _ivf(rows, ids, cent, metric, nlist=None):
    from mirx.index import IvfFlatIndex
    ivf = IvfFlatIndex(rows.shape[1], metric, nlist=cent.shape[0] if nlist is None else nlist)
    ivf.set_centroids(torch.from_numpy(cent))
    ivf.add(torch.from_numpy(rows), None if ids is None else torch.from_numpy(ids))
    return ivf


def _check(ivf, flat, cflat, lists, q, k, nprobe, ex=None):
    """ivf.search(q, k, nprobe) against flat.search under each query's mask; returns (ids, probes).  Queries that probe the
    same set of lists share a mask and go to the oracle together."""
    qt = torch.from_numpy(q)
    ext = None if ex is None else torch.from_numpy(ex)
    s64, ids, probes = ivf.search(qt, k, nprobe, exclude_ids=ext, return_f64=True, return_probes=True)
    val, ids_v = ivf.search(qt, k, nprobe, exclude_ids=ext)
    s64, ids, probes, val = _np(s64), _np(ids), _np(probes), _np(val)
    assert np.array_equal(ids, _np(ids_v))
    npc = min(nprobe, ivf.nlist)
    assert probes.dtype == np.int32 and probes.shape == (q.shape[0], npc)
    assert np.array_equal(probes, _np(cflat.search(qt, npc)[1]))
    groups = {}
    for i in range(q.shape[0]):
        groups.setdefault(tuple(sorted(probes[i].tolist())), []).append(i)
    for key, members in groups.items():
        mask = torch.from_numpy(np.isin(lists, key))
        sel = torch.tensor(members)
        exs = None if ext is None else ext[sel]
        e64, eid = flat.search(qt[sel], k, exclude_ids=exs, allow=mask, return_f64=True)
        ev, _ = flat.search(qt[sel], k, exclude_ids=exs, allow=mask)
        assert np.array_equal(ids[members], _np(eid)), (key, members)
        assert np.array_equal(s64[members], _np(e64))
        assert np.array_equal(val[members], _np(ev))
    return ids, probes


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("dim", [20, 64, 100, 256, 300, 1024, 1100])
def test_forced_lists_every_block_edge(dim, metric):
    L = _lib()
    lib = L.load()
    qt, rb = lib.mirx_ivf_query_tile(dim), lib.mirx_ivf_row_block()
    assert rb + 1 in SIZES and qt == min(16, 65536 // (8 * ((dim + 127) // 128 * 128)))
    rows, ids, cent, base = forced(SIZES, dim, metric, dim, 0.02)
    flat, cflat = _flat(rows, ids, metric), _flat(cent, None, metric)
    ivf = _ivf(rows, ids, cent, metric)
    lists = _np(cflat.search(torch.from_numpy(rows), 1)[1])[:, 0]
    assert np.array_equal(_np(ivf.assign(torch.from_numpy(rows))), lists)
    assert ivf.list_sizes().tolist() == SIZES == np.bincount(lists, minlength=len(SIZES)).tolist() and len(ivf) == sum(SIZES)
    rng = np.random.default_rng(dim + 1)
    near0 = lambda m: (base[0] + 0.02 * rng.standard_normal((m, dim))).astype(np.float32)
    for m in (1, qt - 1, qt, qt + 1, 2 * qt + 1):        # that many queries, all probing list 0; no query probes the other lists
        if m < 1:
            continue
        got, probes = _check(ivf, flat, cflat, lists, near0(m), 10, 1)
        assert (probes == 0).all()
        st = ivf.last_stats()
        assert st == {"nq": m, "rows_scored": m * SIZES[0], "pairs": m, "work_items": 2 * -(-m // qt), "batches": 1}
    # queries spread over the lists; list 1 (empty) is probed together with list 0
    q = np.concatenate([near0(3)] + [(base[l] + 0.02 * rng.standard_normal((2, dim))).astype(np.float32) for l in (2, 3, 4, 5)])
    ex = np.full(q.shape[0], -1, dtype=np.int64)
    ex[0] = ids[np.flatnonzero(lists == 0)[0]]           # inside a probed list (a duplicated row: its twin must stay)
    ex[1] = ids[np.flatnonzero(lists == 6)[0]]           # in a list the query does not probe
    ex[2] = 7                                            # no row has this id
    got, probes = _check(ivf, flat, cflat, lists, q, 10, 2, ex)
    assert ex[0] not in got[0] and (probes[:3, :2] == [0, 1]).all()
    # every list probed: the flat index's answer, in two internal batches
    ivf.set_option(L.IVF_OPT_SCORE_BYTES, 8 * sum(SIZES) * (q.shape[0] - 2))
    got, _ = _check(ivf, flat, cflat, lists, q, 10, len(SIZES), ex)
    assert ivf.last_stats()["batches"] == 2
    e64, eid = flat.search(torch.from_numpy(q), 10, exclude_ids=torch.from_numpy(ex), return_f64=True)
    assert np.array_equal(got, _np(eid))
    assert np.array_equal(_np(ivf.search(torch.from_numpy(q), 10, 1000, exclude_ids=torch.from_numpy(ex), return_f64=True)[0]), _np(e64))


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
@pytest.mark.parametrize("k", [1, 10, 65, 300, 1024])
def test_k_edges_and_padding(k, metric):
    rows, ids, cent, base = forced(SIZES, 64, metric, 5, 0.02)
    flat, cflat = _flat(rows, ids, metric), _flat(cent, None, metric)
    ivf = _ivf(rows, ids, cent, metric)
    lists = _np(cflat.search(torch.from_numpy(rows), 1)[1])[:, 0]
    rng = np.random.default_rng(6)
    q = np.concatenate([(base[l] + 0.02 * rng.standard_normal((2, 64))).astype(np.float32) for l in (0, 2, 3)])
    for nprobe in (1, 2, len(SIZES)):
        got, probes = _check(ivf, flat, cflat, lists, q, k, nprobe)
        if nprobe == 1:                                   # k above the probed rows: (-1, -inf) behind them
            for i, l in enumerate((0, 0, 2, 2, 3, 3)):
                assert (got[i] >= 0).sum() == min(k, SIZES[l])


@pytest.fixture(scope="module")
def recipe():
    """3000 unit rows of dimension 32, nlist = 24, strided start, 10 iterations, 64 perturbed-row queries (the issue's recipe;
    tests/test_ivf_cpu.py checks on the restatement that it differs from the exact answer)"""
    rng = np.random.default_rng(0)
    rows = _unit(rng.standard_normal((3000, 32)))
    rng = np.random.default_rng(1)
    q = _unit(rows[rng.choice(3000, 64, replace=False)] + 0.3 * rng.standard_normal((64, 32)).astype(np.float32))
    return rows, q


def test_recipe_matches_masked_flat_and_differs_from_exact(recipe):
    from mirx.index import IvfFlatIndex
    rows, q = recipe
    ivf = IvfFlatIndex(32, "COSINE", nlist=24)
    ivf.train(torch.from_numpy(rows), iters=10)
    ivf.add(torch.from_numpy(rows))
    cent = _np(ivf.centroids)
    assert np.array_equal(cent, R.train(rows, 24, 10, "COSINE"))
    flat, cflat = _flat(rows, None, "COSINE"), _flat(cent, None, "COSINE")
    lists = _np(cflat.search(torch.from_numpy(rows), 1)[1])[:, 0]
    sizes = ivf.list_sizes()
    assert sizes.min() > 0 and sizes.sum() == 3000 and np.array_equal(sizes, np.bincount(lists, minlength=24))
    got, _ = _check(ivf, flat, cflat, lists, q, 10, 2)
    exact = _np(flat.search(torch.from_numpy(q), 10)[1])
    differ = sum(not np.array_equal(a, b) for a, b in zip(got, exact))
    print(f"lists that differ from the exact top-10 at nprobe = 2: {differ} of 64; recall@10 {R.recall(got, exact):.3f}")
    assert differ >= 48, differ                          # a build that ignores nprobe fails here
    assert np.array_equal(got, R.search(q, rows, None, cent, 10, 2, "COSINE")[1])
    full, _ = _check(ivf, flat, cflat, lists, q, 10, 24)
    assert np.array_equal(full, exact)
    assert ivf.last_stats()["rows_scored"] == 64 * 3000


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_train_equals_the_restatement(metric):
    from mirx.index import IvfFlatIndex
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((700, 20)).astype(np.float32)
    rows = _unit(rows) if metric == "COSINE" else rows
    a, b = IvfFlatIndex(20, metric, nlist=40), IvfFlatIndex(20, metric, nlist=40)
    a.train(torch.from_numpy(rows), iters=3)
    b.train(torch.from_numpy(rows).cuda(), iters=3)       # host and device rows, two calls: equal bits
    cent = _np(a.centroids)
    assert np.array_equal(cent, _np(b.centroids))
    assert np.array_equal(cent, R.train(rows, 40, 3, metric))
    # assignment and probes are FlatIndex's over the centroids
    cflat = _flat(cent, None, metric)
    assert np.array_equal(_np(a.assign(torch.from_numpy(rows))), _np(cflat.search(torch.from_numpy(rows), 1)[1])[:, 0])
    a.add(torch.from_numpy(rows))
    q = torch.from_numpy(rows[:9] + np.float32(0.01))
    for nprobe in (1, 2, 40):
        assert np.array_equal(_np(a.search(q, 5, nprobe, return_probes=True)[2]), _np(cflat.search(q, nprobe)[1]))
    # max_rows: the rows at an even stride
    c = IvfFlatIndex(20, metric, nlist=40)
    c.train(torch.from_numpy(rows), iters=2, max_rows=100)
    assert np.array_equal(_np(c.centroids), R.train(rows[(np.arange(100) * 700) // 100], 40, 2, metric))


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_one_update_step_with_an_empty_list(metric):
    from mirx.index import IvfFlatIndex
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((300, 36)).astype(np.float32)
    rows = _unit(rows) if metric == "COSINE" else rows
    pos = np.array([5, 17, 5, 250, 33, 299], dtype=np.int64)       # list 2 starts as list 0's twin: it stays empty
    ivf = IvfFlatIndex(36, metric, nlist=6)
    ivf.train(torch.from_numpy(rows), iters=1, init_positions=pos)
    start = rows[pos]
    lists = _np(_flat(start, None, metric).search(torch.from_numpy(rows), 1)[1])[:, 0]
    assert not (lists == 2).any()
    want = R.update(rows, lists, start, metric)
    got = _np(ivf.centroids)
    assert np.array_equal(got, want) and np.array_equal(got[2], rows[5])
    zero = IvfFlatIndex(36, metric, nlist=6)
    zero.train(torch.from_numpy(rows), iters=0, init_positions=pos)
    assert np.array_equal(_np(zero.centroids), start)


@pytest.mark.parametrize("metric", ["COSINE", "L2"])
def test_add_in_batches_remove_and_new_centroids(metric):
    rows, ids, cent, base = forced(SIZES, 100, metric, 21, 0.02)
    n = rows.shape[0]
    q = np.concatenate([(base[l] + np.float32(0.01)).astype(np.float32)[None] for l in (0, 3, 5, 6)])
    from mirx.index import IvfFlatIndex
    ivf = IvfFlatIndex(100, metric, nlist=len(SIZES))
    with pytest.raises(_lib().MirxError, match="centroids are not fixed"):
        ivf.add(torch.from_numpy(rows))
    ivf.set_centroids(torch.from_numpy(cent))
    ivf.add(torch.from_numpy(rows[:200]), torch.from_numpy(ids[:200]))
    ivf.add(torch.from_numpy(rows[200:]).cuda(), torch.from_numpy(ids[200:]).cuda())
    whole = _ivf(rows, ids, cent, metric)
    for nprobe in (1, 3):
        a, b = ivf.search(torch.from_numpy(q), 20, nprobe, return_f64=True), whole.search(torch.from_numpy(q), 20, nprobe, return_f64=True)
        assert np.array_equal(_np(a[0]), _np(b[0])) and np.array_equal(_np(a[1]), _np(b[1]))
    # remove: duplicates count once, absent ids are ignored; then the answer of a fresh index over the survivors
    gone = np.concatenate([ids[5:60], ids[5:20], ids[n - 40:], [123456789]])
    assert ivf.remove(torch.from_numpy(gone)) == 55 + 40
    keep = np.ones(n, bool)
    keep[5:60] = keep[n - 40:] = False
    fresh = _ivf(rows[keep], ids[keep], cent, metric)
    assert len(ivf) == len(fresh) == n - 95 and np.array_equal(ivf.list_sizes(), fresh.list_sizes())
    flat, cflat = _flat(rows[keep], ids[keep], metric), _flat(cent, None, metric)
    lists = _np(cflat.search(torch.from_numpy(rows[keep]), 1)[1])[:, 0]
    for nprobe in (1, 3, len(SIZES)):
        a, b = ivf.search(torch.from_numpy(q), 20, nprobe, return_f64=True), fresh.search(torch.from_numpy(q), 20, nprobe, return_f64=True)
        assert np.array_equal(_np(a[0]), _np(b[0])) and np.array_equal(_np(a[1]), _np(b[1]))
        _check(ivf, flat, cflat, lists, q, 20, nprobe)
    # new centroids on an index that holds rows: the rows are re-assigned
    cent2 = np.ascontiguousarray(base[::-1])
    ivf.set_centroids(torch.from_numpy(cent2))
    again = _ivf(rows[keep], ids[keep], cent2, metric)
    assert np.array_equal(ivf.list_sizes(), again.list_sizes())
    a, b = ivf.search(torch.from_numpy(q), 20, 2, return_f64=True), again.search(torch.from_numpy(q), 20, 2, return_f64=True)
    assert np.array_equal(_np(a[0]), _np(b[0])) and np.array_equal(_np(a[1]), _np(b[1]))
    # auto ids go on past the largest one handed out, as FlatIndex's
    auto = IvfFlatIndex(100, metric, nlist=len(SIZES))
    auto.set_centroids(torch.from_numpy(cent))
    auto.add(torch.from_numpy(rows[:10]))
    assert auto.remove([8, 9]) == 2
    auto.add(torch.from_numpy(rows[10:12]))
    got = _np(auto.search(torch.from_numpy(rows[:1]), 12, len(SIZES))[1])[0]
    assert sorted(got[got >= 0].tolist()) == [0, 1, 2, 3, 4, 5, 6, 7, 10, 11]


def test_collection_route(recipe):
    from mirx.retriever import Collection
    from mirx.index import IvfFlatIndex
    rows, q = recipe
    rows, q = rows[:1200], q[:12]
    labels = [f"c{i % 3}" for i in range(1200)]
    paths = [f"p{i}.png" for i in range(1200)]
    params = {"metric_type": "COSINE", "index_type": "IVF_FLAT", "params": {"nlist": 12}}
    approx, twin = Collection("a", 32), Collection("t", 32)
    approx.create_index("embedding", params, approximate=True)
    twin.create_index("embedding", params)
    for col in (approx, twin):
        col.insert([paths, labels, rows])
        col.load()
    ivf = IvfFlatIndex(32, "COSINE", nlist=12)
    ivf.train(torch.from_numpy(rows))
    ivf.add(torch.from_numpy(rows))
    pairs = lambda hits: [[(h.id, h.distance) for h in hs] for hs in hits]

    def direct(index, nprobe, ex=None):
        sc, ids = index.search(torch.from_numpy(q), 10, nprobe, exclude_ids=ex)
        return [[(int(i), float(v)) for i, v in zip(a, b) if i >= 0] for a, b in zip(_np(ids), _np(sc))]

    p2 = {"metric_type": "COSINE", "params": {"nprobe": 2}}
    exact = pairs(twin.search(q, param=p2, limit=10))
    assert exact == pairs(twin.search(q, limit=10)) == pairs(twin.search(q, param={"nprobe": 12}, limit=10))
    got = pairs(approx.search(q, param=p2, limit=10))
    assert got == direct(ivf, 2) and got != exact
    assert pairs(approx.search(q, param={"nprobe": 2}, limit=10)) == got                  # the key at the top level
    ex = list(range(12))
    assert pairs(approx.search(q, param=p2, limit=10, exclude_ids=ex)) == direct(ivf, 2, ex)
    assert pairs(approx.search(q, param={"params": {"nprobe": 12}}, limit=10)) == exact  # every list probed
    # every other call stays exact: no nprobe, an expr, grouping, a radius
    assert pairs(approx.search(q, limit=10)) == exact
    assert pairs(approx.search(q, param={"params": {"ef": 64}}, limit=10)) == exact
    e = 'label == "c1"'
    assert pairs(approx.search(q, param=p2, limit=10, expr=e)) == pairs(twin.search(q, limit=10, expr=e))
    assert pairs(approx.search(q, param=p2, limit=4, group_by_field="label")) == pairs(twin.search(q, limit=4, group_by_field="label"))
    pr = {"params": {"nprobe": 2, "radius": 0.2}}
    assert pairs(approx.search(q, param=pr, limit=10)) == pairs(twin.search(q, param=pr, limit=10))
    # after delete and insert the lists are rebuilt with the kept centroids
    cent = _np(ivf.centroids)
    approx.delete("id in [0, 1, 2, 3, 4, 5, 6, 7]")
    approx.insert([["n.png"], ["c0"], q[:1]])
    keep = np.arange(8, 1200)
    again = IvfFlatIndex(32, "COSINE", nlist=12)
    again.set_centroids(torch.from_numpy(cent))
    again.add(torch.from_numpy(np.concatenate([rows[keep], q[:1]])), torch.from_numpy(np.concatenate([keep, [1200]])))
    got = pairs(approx.search(q, param=p2, limit=10))
    assert got == direct(again, 2) and got[0][0][0] == 1200
    assert np.array_equal(_np(approx._ivf.centroids), cent)
    # fewer rows than lists: nothing to train on, the exact routes answer
    small = Collection("s", 32)
    small.create_index("embedding", {"index_type": "IVF_FLAT", "params": {"nlist": 64}}, approximate=True)
    small.insert([paths[:20], labels[:20], rows[:20]])
    small.load()
    other = Collection("o", 32)
    other.insert([paths[:20], labels[:20], rows[:20]])
    assert pairs(small.search(q, param=p2, limit=5)) == pairs(other.search(q, limit=5))
