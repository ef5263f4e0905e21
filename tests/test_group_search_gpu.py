"""FlatIndex.search_grouped, Collection.search(group_by_field=) and MilvusRetriever.search(group_by=) end to end against the
contract (tests/_group_ref.py).  GPU only; no tolerance: ids, group codes and score bits are compared with ==.

The reference ranking of a query is built in numpy from oracle.search.scores (the fp64 lane-tree scores, inputs padded with
zero columns to a multiple of 4 as the index pads them): the eligible rows ordered by (score descending, id ascending), then
walked by _group_ref.  Every route must return exactly that."""
import functools

import numpy as np
import pytest
import torch

import _group_ref as R
from oracle import search as OS

pytestmark = pytest.mark.gpu
METRICS = ("COSINE", "L2")
N, D, NQ = 2000, 32, 6


def _mc(metric):
    return OS.METRIC_IP if metric == "COSINE" else OS.METRIC_NEG_L2


def _pad4(x):
    return torch.nn.functional.pad(x, (0, -x.shape[1] % 4))


@functools.lru_cache(maxsize=None)
def _data(n, d, metric, seed=3):
    """(gallery [n, d], queries [NQ, d] near gallery rows 0, 1, .. so that the own id matters, oracle scores [NQ, n])"""
    g = torch.Generator().manual_seed(seed + n)
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    if metric == "L2":
        x = x * (0.5 + torch.rand(n, 1, generator=g))
    x[n // 2] = x[n // 2 + 1]                                              # one pair of equal rows: a score tie in every query
    q = (x[:NQ] + 0.3 * torch.randn(NQ, d, generator=g)).contiguous()
    s = OS.scores(_pad4(q).numpy(), _pad4(x).numpy(), _mc(metric))
    return x.contiguous(), q, s


def _codes(n, n_groups, skewed, seed=0):
    """balanced: code = a random permutation of row % n_groups; skewed: group 0 owns 90 % of the rows"""
    rng = np.random.default_rng(seed + n_groups)
    if skewed and n_groups > 1:
        codes = np.where(rng.random(n) < 0.9, 0, 1 + rng.integers(0, n_groups - 1, n))
        codes[:n_groups] = np.arange(n_groups)
    else:
        codes = rng.permutation(np.arange(n) % n_groups)
    return codes.astype(np.int64)


def _index(x, metric, ids=None):
    from mirx.index import FlatIndex
    ix = FlatIndex(x.shape[1], metric, 0)
    ix.add(x, ids)
    return ix


def _expected(s, ids, codes, limit, gs, mask=None, exclude=None):
    """the contract for every query: (ids [nq, limit, gs], fp64 scores, codes [nq, limit]) as numpy arrays"""
    out = []
    for i in range(s.shape[0]):
        elig = np.ones(len(ids), bool) if mask is None else mask.copy()
        if exclude is not None:
            elig &= ids != exclude[i]
        order = R.ranking_of(ids, s[i], elig)
        e_ids, e_sc, e_codes, _ = R.tensors(order, ids[order], s[i][order], codes, limit, gs)
        out.append((e_ids, e_sc, e_codes))
    return [np.stack([o[j] for o in out]) for j in range(3)]


def _assert_equal(got, want, metric, what):
    ids, s64, codes = (t.cpu().numpy() for t in got)
    assert np.array_equal(ids, want[0]), what
    assert np.array_equal(codes, want[2]), what
    assert np.array_equal(s64.view(np.int64), want[1].view(np.int64)), what


def _reported(s64, metric):
    return OS.reported_value(s64, _mc(metric)).astype(np.float32)


def _run(ix, q, codes, limit, gs, want, metric, route="auto", **kw):
    got = ix.search_grouped(q, codes, limit, gs, return_f64=True, route=route, **kw)
    _assert_equal(got, want, metric, (route, limit, gs, sorted(kw)))
    st = ix.group_last_stats()
    nq = q.shape[0]
    assert st["nq"] == nq and st["route"] == route
    if route == "direct":
        assert st["direct"] == nq and st["walk"] == st["fill"] == st["deepen"] == 0
    elif route == "deepen":
        assert st["deepen"] == nq and st["direct"] == st["walk"] == st["fill"] == 0 and st["passes"] >= 1
    elif route == "walk":
        assert st["direct"] == 0 and st["walk"] + st["fill"] + st["deepen"] == nq
    return st


@pytest.mark.parametrize("skewed", [False, True])
@pytest.mark.parametrize("n_groups", [1, 3, 16, 17, 500, N])
@pytest.mark.parametrize("metric", METRICS)
def test_search_grouped_against_the_contract(metric, n_groups, skewed):
    from mirx.index import GROUP_DIRECT_MAX
    x, q, s = _data(N, D, metric)
    ids = np.arange(N, dtype=np.int64)
    codes = _codes(N, n_groups, skewed)
    ix = _index(x, metric)
    mask = np.random.default_rng(n_groups).random(N) < 0.5
    own = ids[:NQ].copy()                                                   # query i sits next to row i
    for limit in (1, 3, 10, min(n_groups + 5, 1024)):
        for gs in (1, 3):
            for kw_np in ({}, {"allow": mask}, {"exclude_ids": own}, {"allow": mask, "exclude_ids": own}):
                want = _expected(s, ids, codes, limit, gs, kw_np.get("allow"), kw_np.get("exclude_ids"))
                kw = {k: torch.from_numpy(v) for k, v in kw_np.items()}
                st = _run(ix, q, codes, limit, gs, want, metric, **kw)
                live = len(set(codes[mask].tolist())) if "allow" in kw else n_groups
                assert st["groups"] == live
                assert (st["direct"] == NQ) == (live <= GROUP_DIRECT_MAX)
                # every route, the same tensors (one masked search per group is only affordable for a few hundred groups)
                if (limit, gs) in ((3, 3), (10, 1)) or (limit > 10 and gs == 1 and not kw):
                    direct = limit == 3 and (n_groups <= 17 or (n_groups <= 500 and not kw))
                    for route in ("walk", "deepen") + (("direct",) if direct else ()):
                        _run(ix, q, codes, limit, gs, want, metric, route=route, **kw)
    # the fp32 form: search()'s reported values
    want = _expected(s, ids, codes, 3, 3, mask, own)
    got = ix.search_grouped(q, torch.from_numpy(codes), 3, 3, exclude_ids=own, allow=mask)
    assert got[1].dtype == torch.float32 and np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(got[1].cpu().numpy().view(np.int32), _reported(want[1], metric).view(np.int32))


@pytest.mark.parametrize("metric", METRICS)
def test_search_grouped_after_remove_and_with_sparse_ids(metric):
    """ids that are not 0 .. n-1: after remove() of a tenth of the rows, and with user ids around 2^40 in no order"""
    x, q, s = _data(N, D, metric)
    rng = np.random.default_rng(11)
    gone = np.sort(rng.permutation(N)[:N // 10])
    keep = np.setdiff1d(np.arange(N), gone)
    ix = _index(x, metric)
    assert ix.ids().tolist() == list(range(N))
    assert ix.remove(torch.from_numpy(gone)) == len(gone)
    assert ix.ids().cpu().numpy().tolist() == keep.tolist()
    sparse = (2 ** 40 + rng.permutation(10 * N)[:N] * 977).astype(np.int64)
    ix2 = _index(x, metric, torch.from_numpy(sparse))
    for n_groups in (17, 500):
        codes = _codes(N, n_groups, False)
        mask = rng.random(N) < 0.5
        for limit, gs in ((3, 3), (10, 1), (n_groups + 5, 2)):
            for route in ("auto", "walk", "deepen"):
                want = _expected(s[:, keep], keep, codes[keep], limit, gs, mask[keep], keep[[0, 1, 2, 3, 4, 5]])
                _run(ix, q, codes[keep], limit, gs, want, metric, route=route, allow=mask[keep], exclude_ids=keep[:NQ])
                want = _expected(s, sparse, codes, limit, gs, mask, sparse[:NQ])
                _run(ix2, q, codes, limit, gs, want, metric, route=route, allow=mask, exclude_ids=sparse[:NQ])
    want = _expected(s, sparse, _codes(N, 3, True), 3, 2)
    _run(ix2, q, _codes(N, 3, True), 3, 2, want, metric, route="direct")
    # sparse CODES (far above the row count) come back as given
    codes = _codes(N, 40, False) * 10 ** 9 + 5
    want = _expected(s, sparse, codes, 10, 2)
    _run(ix2, q, codes, 10, 2, want, metric)


def test_search_grouped_refuses_what_the_contract_refuses():
    x, q, _ = _data(N, D, "COSINE")
    ix = _index(x[:50], "COSINE")
    codes = np.arange(50) % 4
    for bad in (codes[:49], np.concatenate([codes, [0]]), codes.astype(np.float32), codes - 1, codes.astype(bool)):
        with pytest.raises(ValueError):
            ix.search_grouped(q, bad, 3)
    for limit, gs in ((0, 1), (1025, 1), (3, 0), (3, 65), (1024, 17)):
        with pytest.raises(ValueError):
            ix.search_grouped(q, codes, limit, gs)
    with pytest.raises(ValueError, match="route"):
        ix.search_grouped(q, codes, 3, route="fast")
    with pytest.raises(ValueError):
        ix.search_grouped(q, codes, 3, allow=np.ones(49, bool))
    # a repeated id
    twice = _index(x[:50], "COSINE", torch.cat([torch.arange(49), torch.tensor([7])]))
    with pytest.raises(ValueError, match="repeats"):
        twice.search_grouped(q, codes, 3)
    # an empty index, an all-zero mask, no query: empty answers of the right shapes
    from mirx.index import FlatIndex
    ids, sc, gc = FlatIndex(D, "COSINE", 0).search_grouped(q, np.zeros(0, np.int64), 3, 2)
    assert ids.shape == (NQ, 3, 2) and (ids == -1).all() and torch.isinf(sc).all() and (gc == -1).all()
    ids, sc, gc = ix.search_grouped(q, codes, 3, 2, allow=np.zeros(50, bool))
    assert (ids == -1).all() and (sc == float("-inf")).all() and (gc == -1).all()
    ids, sc, gc = ix.search_grouped(q[:0], codes, 3, 2)
    assert ids.shape == (0, 3, 2) and gc.shape == (0, 3)


@pytest.mark.parametrize("metric", METRICS)
def test_search_grouped_large_gallery_takes_the_filter_prefix_and_the_fill(metric):
    """40 000 x 64 (above TIER1_MIN_ROWS: the first prefix comes from the filter GEMM), ~5000 groups of 8, limit 10: the walk
    answers group_size 1 from the first prefix, group_size 3 goes through the fill, neither through rank_top"""
    n, d = 40000, 64
    x, q, s = _data(n, d, metric)
    ids = np.arange(n, dtype=np.int64)
    codes = _codes(n, 5000, False)
    ix = _index(x, metric)
    want = _expected(s, ids, codes, 10, 1)
    st = _run(ix, q, codes, 10, 1, want, metric)
    assert st["walk"] == NQ and st["fill"] == 0 and st["deepen"] == 0 and st["passes"] == 1 and st["max_depth"] == 64
    assert ix.last_stats()["tier1_answered"] > 0
    want = _expected(s, ids, codes, 10, 3)
    st = _run(ix, q, codes, 10, 3, want, metric)
    assert st["deepen"] == 0 and st["fill"] > 0 and st["walk"] + st["fill"] == NQ and st["passes"] == 1
    own = ids[:NQ].copy()
    want = _expected(s, ids, codes, 10, 3, None, own)
    st = _run(ix, q, codes, 10, 3, want, metric, exclude_ids=own)
    assert st["deepen"] == 0 and st["max_depth"] == 63


def _labels(n):
    return [("COVID-19", "Normal", "Pneumonia")[(i * 7 + i // 5) % 3] for i in range(n)]


def _patients(n):
    return [1000 + (i * 13) % 41 for i in range(n)]


def _collection_checks(col, metric):
    """Collection.search(group_by_field=) == FlatIndex.search_grouped on codes the test derives from the column itself"""
    index = col.index
    live = col.live_ids()
    q = torch.nn.functional.normalize(torch.randn(3, col.dim, generator=torch.Generator().manual_seed(5)), dim=1)
    for field, limit, gs in (("label", 3, 1), ("label", 2, 4), ("patient", 10, 3), ("patient", 50, 1)):
        values = col.field(field)
        distinct = sorted(set(values))
        codes = np.array([distinct.index(v) for v in values], dtype=np.int64)
        for expr, ex in ((None, None), ('label != "Normal"', None), ("patient >= 1010", [int(live[3]), int(live[0]), -1])):
            allow = None if expr is None else col.expr_mask(expr)
            ids, sc, gc = index.search_grouped(q, codes, limit, gs, exclude_ids=ex, allow=allow)
            ids, sc, gc = ids.cpu().numpy(), sc.cpu().numpy(), gc.cpu().numpy()
            res = col.search(q, limit=limit, group_by_field=field, group_size=gs, expr=expr, exclude_ids=ex,
                             output_fields=["image_path"], strict_group_size=(gs != 4))
            for i in range(3):
                flat = [(int(a), float(v)) for a, v in zip(ids[i].ravel(), sc[i].ravel()) if a >= 0]
                assert [(h.id, h.distance if metric == "COSINE" else -h.distance) for h in res[i]] == flat, (field, expr)
                assert len(flat) > 0
                # group after group: the group field of the hits follows the codes, and the entity carries it
                want_groups = [distinct[c] for c, row in zip(gc[i], ids[i]) for a in row if a >= 0]
                assert [h.entity.get(field) for h in res[i]] == want_groups
                assert all(h.entity.get(field) == values[int(np.searchsorted(live, h.id))] for h in res[i])
                assert all(h.entity.get("image_path") == f"img/{h.id}.png" for h in res[i])
                if expr == 'label != "Normal"':
                    assert all(col.entity(h.id)["label"] != "Normal" for h in res[i])
                if ex is not None:
                    assert ex[i] not in [h.id for h in res[i]]


@pytest.mark.parametrize("metric", METRICS)
def test_collection_grouping_search(metric):
    from mirx.retriever import Collection
    n, dim = 600, 16
    emb = _data(n, dim, metric)[0]
    col = Collection("c", dim, metric_type=metric, extra_fields=("patient",))
    col.insert([[f"img/{i}.png" for i in range(n)], _labels(n), emb, _patients(n)])
    _collection_checks(col, metric)
    col.delete("id in [0, 5, 17, 300]")
    _collection_checks(col, metric)
    # the nearest case of every diagnosis: three hits, three labels
    hits = col.search(emb[:1], limit=3, group_by_field="label")[0]
    assert sorted(h.entity.get("label") for h in hits) == ["COVID-19", "Normal", "Pneumonia"]
    with pytest.raises(ValueError, match="patient"):
        col.search(emb[:1], limit=3, group_by_field="study")
    with pytest.raises(ValueError, match="range"):
        col.search(emb[:1], limit=3, group_by_field="label", param={"params": {"radius": 0.1}})


def test_persistent_collection_grouping_search(tmp_path):
    from mirx.retriever import Collection
    from mirx.store import Store
    n, dim = 600, 16
    emb = _data(n, dim, "COSINE")[0]
    schema = ["id", "image_path", "label", "embedding", "patient"]
    col = Collection.from_stored(Store(tmp_path / "db").create("c", dim, "COSINE", schema))
    col.insert([[f"img/{i}.png" for i in range(n)], _labels(n), emb, _patients(n)])
    col.delete("id in [7, 150]")
    col.flush()
    again = Collection.from_stored(Store(tmp_path / "db").open("c"))
    assert again._index is None                                             # loads on first use
    _collection_checks(again, "COSINE")
    again.release()
    _collection_checks(again, "COSINE")                                     # the codes are uploaded again after a release


def test_retriever_group_by_on_a_stand_in_model():
    from mirx.retriever import MilvusManager, MilvusRetriever

    class _Model(torch.nn.Module):
        device = torch.device("cuda:0")

        def forward(self, x):
            return x.reshape(x.shape[0], -1)[:, :512] + 0.25

    n, dim = 200, 512
    emb = _data(n, dim, "COSINE")[0]
    mgr = MilvusManager(dataset="covid")
    col = mgr.create_collection("dinov2")
    col.insert([[f"img/{i}.png" for i in range(n)], _labels(n), emb])
    r = MilvusRetriever(mgr, "dinov2", _Model(), lambda img: img)
    img = torch.randn(3, 16, 16, generator=torch.Generator().manual_seed(1))
    plain, _ = r.search(img, top_k=3)
    assert [set(d) for d in plain] == [{"id", "image_path", "label", "distance", "similarity"}] * 3
    grouped, emb_q = r.search(img, top_k=3, group_by="label", group_size=2)
    assert len(grouped) == 6 and [d["group"] for d in grouped] == [d["label"] for d in grouped]
    assert grouped[0]["id"] == plain[0]["id"] and grouped[0]["distance"] == plain[0]["distance"]
    assert grouped[0]["group"] == grouped[1]["group"] != grouped[2]["group"] == grouped[3]["group"]
    want = col.search(emb_q, limit=3, group_by_field="label", group_size=2)[0]
    assert [d["id"] for d in grouped] == [h.id for h in want]
    batch = r.batch_search([img, img], top_k=3, group_by="label", group_size=2)
    assert [[d["id"] for d in b] for b in batch] == [[d["id"] for d in grouped]] * 2
    assert all("group" not in d for b in r.batch_search([img], top_k=3) for d in b)
