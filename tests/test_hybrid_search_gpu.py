"""Hybrid search end to end on the GPU: hybrid_search / MilvusManager.hybrid_search against the float64 restatement
(tests/_fuse_ref.py) applied to the collections' OWN search() results -- the lists a caller would fuse by hand.

Three small collections with overlapping but unequal image_path sets, different ids for the same path and three metrics.
RRF and the COSINE / raw weighted forms: the same documents in the same order with the same fp64 score bits.  Forms that go
through atan (an IP or L2 request under norm_score=True): the same documents, scores within 1e-12, on data whose non-tied
adjacent scores are at least 1e-9 apart in the restatement (asserted)."""
import numpy as np
import pytest
import torch

import _fuse_ref as R

pytestmark = pytest.mark.gpu


def _rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def world():
    """a: COSINE, 300 rows of dim 16, paths 0..299; b: L2, 250 rows of dim 8, paths 100..349 in another order; c: IP, 200 rows
    of dim 64, every third path of 0..599.  The same path has a different id in each."""
    from mirx.retriever import Collection
    rng = np.random.default_rng(35)
    a = Collection("a", 16, metric_type="COSINE")
    b = Collection("b", 8, metric_type="L2")
    c = Collection("c", 64, metric_type="IP", extra_fields=("patient",))
    pa = [f"img/{i}.png" for i in range(300)]
    pb = [f"img/{i}.png" for i in rng.permutation(np.arange(100, 350))]
    pc = [f"img/{i}.png" for i in range(0, 600, 3)]
    a.insert([pa, [f"l{i % 4}" for i in range(300)], _rows(rng, 300, 16)])
    b.insert([pb, [f"l{i % 3}" for i in range(250)], 2.0 * _rows(rng, 250, 8)])
    c.insert([pc, ["l"] * 200, 1.5 * _rows(rng, 200, 64), list(range(200))])
    q = {"a": _rows(rng, 5, 16), "b": 2.0 * _rows(rng, 5, 8), "c": 1.5 * _rows(rng, 5, 64)}
    return {"a": a, "b": b, "c": c}, q


def _expected(cols, reqs, ranker_form, limit, exclude_keys=None, join_field="image_path"):
    """the restatement over the collections' own search() results: per query [(key, score)]"""
    distinct = []
    for r in reqs:
        if not any(cols[r.anns_field] is d for d in distinct):
            distinct.append(cols[r.anns_field])
    code_of = R.join_order([d.field(join_field) for d in distinct])
    lists = []
    for r in reqs:
        col = cols[r.anns_field]
        ex = None
        if exclude_keys is not None:
            by_key = dict(zip(col.field(join_field), col.live_ids().tolist()))
            ex = torch.tensor([by_key.get(k, -1) for k in exclude_keys], dtype=torch.int64)
        lists.append(col.search(r.data, limit=r.limit, expr=r.expr, param=r.param, exclude_ids=ex, output_fields=[join_field]))
    nq = len(lists[0])
    key = lambda h: h.entity.get(join_field)
    out = [R.fuse_by_key([l[qi] for l in lists], code_of, ranker_form, limit, key=key) for qi in range(nq)]
    return out, code_of, lists


def _check(cols, reqs, rerank, limit, exact=True, manager=None, **kw):
    from mirx.retriever import hybrid_search
    form = rerank.kernel_form([cols[r.anns_field].metric_type for r in reqs])
    exp, code_of, lists = _expected(cols, reqs, form, limit, exclude_keys=kw.get("exclude_keys"))
    got = manager.hybrid_search(reqs, rerank, limit, **kw) if manager is not None else hybrid_search(cols, reqs, rerank, limit, **kw)
    assert len(got) == len(exp)
    if not exact:
        gap = min(min([a[1] - b[1] for a, b in zip(e, e[1:]) if a[1] != b[1]], default=np.inf) for e in exp)
        print(f"smallest non-tied adjacent gap of the restatement: {gap:.3e}")
        assert gap >= 1e-9, gap
    worst = 0.0
    for hits, e in zip(got, exp):
        assert [h.entity.get("image_path") for h in hits] == [k for k, _ in e]
        assert all(type(h.distance) is float for h in hits)
        if exact:
            assert [h.distance.hex() for h in hits] == [s.hex() for _, s in e]
        else:
            worst = max([worst] + [abs(h.distance - s) for h, (_, s) in zip(hits, e)])
    if not exact:
        print(f"largest |device - restatement| of a fused score: {worst:.3e}")
        assert worst <= 1e-12, worst
    # id and entity: the document's row in the first requested collection that holds it
    distinct = []
    for r in reqs:
        if not any(cols[r.anns_field] is d for d in distinct):
            distinct.append(cols[r.anns_field])
    for hits in got:
        for h in hits:
            path = h.entity.get("image_path")
            owner = next(d for d in distinct if path in d.field("image_path"))
            assert owner.entity(h.id)["image_path"] == path
    return got, exp, lists


def _reqs(q, spec):
    from mirx.retriever import AnnSearchRequest
    return [AnnSearchRequest(q[name], name, limit=limit, **kw) for name, limit, kw in spec]


def test_rrf_over_three_collections_with_mixed_metrics(world):
    from mirx.retriever import RRFRanker
    cols, q = world
    reqs = _reqs(q, [("a", 40, {}), ("b", 17, {}), ("c", 64, {})])
    got, exp, lists = _check(cols, reqs, RRFRanker(), 10)
    assert all(len(h) == 10 for h in got)
    got, exp, _ = _check(cols, reqs, RRFRanker(k=1), 200)                         # more than the documents the lists hold
    assert all(len(h) == len(e) < 121 for h, e in zip(got, exp))                 # shared documents were joined
    assert any(a[1] == b[1] for e in exp for a, b in zip(e, e[1:]))              # ties, resolved by first appearance of the key
    # every list is the collection's own search(): a request alone returns that list, in order
    one, _, lists = _check(cols, reqs[1:2], RRFRanker(), 17)
    assert [[h.id for h in hits] for hits in one] == [[h.id for h in hits] for hits in lists[0]]


def test_weighted_rankers(world):
    from mirx.retriever import WeightedRanker
    cols, q = world
    ac = _reqs(q, [("a", 40, {}), ("c", 64, {})])
    _check(cols, ac, WeightedRanker(0.7, 0.3, norm_score=False), 25)              # raw similarities: bit-exact
    _check(cols, _reqs(q, [("a", 40, {}), ("a", 9, {})]), WeightedRanker(0.6, 0.4), 30)   # COSINE alone: bit-exact
    abc = _reqs(q, [("a", 40, {}), ("b", 17, {}), ("c", 64, {})])
    _check(cols, abc, WeightedRanker(0.5, 0.3, 0.2), 20, exact=False)             # IP and L2 go through atan


def test_one_gallery_several_query_vectors(world):
    """the same collection in two requests with different queries: documents found by both add two terms"""
    from mirx.retriever import AnnSearchRequest, RRFRanker
    cols, q = world
    reqs = [AnnSearchRequest(q["a"], "a", limit=30), AnnSearchRequest(q["a"][::-1].copy(), "a", limit=30),
            AnnSearchRequest(q["b"], "b", limit=12)]
    got, exp, _ = _check(cols, reqs, RRFRanker(), 1024)
    assert all(len(h) <= 72 for h in got)
    assert got[2][0].distance >= 1.0 / 61.0 + 1.0 / 61.0                         # query 2 is its own mirror image: the same list twice


def test_expr_param_and_limits_beyond_the_rows(world):
    from mirx.retriever import RRFRanker, WeightedRanker
    cols, q = world
    reqs = _reqs(q, [("a", 40, {"expr": 'label in ["l1", "l3"]'}), ("b", 4000, {}), ("c", 50, {"expr": "patient < 20"})])
    got, exp, lists = _check(cols, reqs, RRFRanker(), 300)
    assert all(len(l) == 250 for l in lists[1]) and all(len(l) == 20 for l in lists[2])    # b: every row; c: the 20 rows it allows
    # a radius (the request's own search() cuts its list at it), alone and with a range_filter
    for param in ({"params": {"radius": 0.3}}, {"radius": 0.3, "range_filter": 0.45, "nprobe": 8}):
        reqs = _reqs(q, [("a", 60, {"param": param}), ("c", 64, {})])
        got, exp, lists = _check(cols, reqs, WeightedRanker(1.0, 0.5, norm_score=False), 100)
        assert any(0 < len(l) < 60 for l in lists[0])


def test_exclude_keys(world):
    from mirx.retriever import RRFRanker
    cols, q = world
    # the queries ARE gallery rows of a; their documents rank first in a's list unless excluded
    own = [f"img/{i}.png" for i in (120, 3, 299, 150, 101)]                        # 3 is held by a and c only, 299 by a and b
    qa = np.stack([cols["a"].index.rows(cols["a"].position(i), 1)[0][0].cpu().numpy() for i in (120, 3, 299, 150, 101)])
    reqs = _reqs({"a": qa, "b": q["b"], "c": q["c"]}, [("a", 20, {}), ("b", 250, {}), ("c", 200, {})])
    plain, _, _ = _check(cols, reqs, RRFRanker(), 1024)
    got, _, _ = _check(cols, reqs, RRFRanker(), 1024, exclude_keys=own)
    for qi, key in enumerate(own):
        assert key in [h.entity.get("image_path") for h in plain[qi]]
        assert key not in [h.entity.get("image_path") for h in got[qi]]          # gone from every list, b's and c's full rankings too
    # a key nobody holds, and None, exclude nothing
    same, _, _ = _check(cols, reqs, RRFRanker(), 1024, exclude_keys=["img/none.png", None, "img/none.png", None, None])
    assert [[(h.id, h.distance) for h in hits] for hits in same] == [[(h.id, h.distance) for h in hits] for hits in plain]


def test_output_fields_and_join_field(world):
    from mirx.retriever import RRFRanker, hybrid_search
    cols, q = world
    reqs = _reqs(q, [("c", 30, {}), ("a", 30, {})])
    hits = hybrid_search(cols, reqs, RRFRanker(), 5, output_fields=["label", "patient"])[0]
    for h in hits:
        path = h.entity.get("image_path")                                        # always carried
        if path in cols["c"].field("image_path"):                                # c is asked first: its row, its fields
            assert cols["c"].entity(h.id) == {"image_path": path, "label": "l", "patient": h.entity.get("patient")}
        else:
            assert h.entity.get("patient") is None and h.entity.get("label") == cols["a"].entity(h.id)["label"]
    by_list = hybrid_search([cols["c"], cols["a"]], reqs, RRFRanker(), 5)         # one collection per request instead of a mapping
    assert [(h.id, h.distance) for h in by_list[0]] == [(h.id, h.distance) for h in hits]


def test_deleted_row_empty_collection_and_the_join_table_cache():
    from mirx.retriever import AnnSearchRequest, Collection, RRFRanker, WeightedRanker, _join_table
    rng = np.random.default_rng(36)
    a, b, empty = Collection("a", 8), Collection("b", 8, metric_type="IP"), Collection("e", 8)
    a.insert([[f"p{i}" for i in range(70)], ["l"] * 70, _rows(rng, 70, 8)])
    b.insert([[f"p{i}" for i in range(69, 29, -1)], ["l"] * 40, _rows(rng, 40, 8)])
    cols = {"a": a, "b": b, "e": empty}
    q = _rows(rng, 3, 8)
    reqs = [AnnSearchRequest(q, "e", limit=5), AnnSearchRequest(q, "a", limit=70), AnnSearchRequest(q, "b", limit=40)]
    got, _, lists = _check(cols, reqs, RRFRanker(), 100)
    assert lists[0] == [[], [], []] and all(len(h) == 70 for h in got)
    table = _join_table([empty, a, b], "image_path")
    dev = [table.device_codes(1, a.index.device), table.device_codes(2, b.index.device)]
    _check(cols, reqs, WeightedRanker(0.2, 0.5, 0.5, norm_score=False), 100)
    assert _join_table([empty, a, b], "image_path") is table                     # built once per state of the collections ..
    assert table.device_codes(1, a.index.device) is dev[0] and table.device_codes(2, b.index.device) is dev[1]   # .. uploaded once
    # p40 leaves a: the document lives on in b, under b's id
    assert a.delete('image_path == "p40"').delete_count == 1
    got, _, _ = _check(cols, reqs, RRFRanker(), 100)
    assert _join_table([empty, a, b], "image_path") is not table
    p40 = [h for h in got[0] if h.entity.get("image_path") == "p40"]
    assert len(p40) == 1 and p40[0].id == 29 and all(len(h) == 70 for h in got)
    assert b.delete('image_path == "p40"').delete_count == 1                     # and now nobody holds it
    got, _, _ = _check(cols, reqs, RRFRanker(), 100)
    assert all(len(h) == 69 and "p40" not in [x.entity.get("image_path") for x in h] for h in got)
    # only empty collections: nothing to find, no kernel to run
    assert _check({"e": empty}, reqs[:1], RRFRanker(), 10)[0] == [[], [], []]


def test_manager_hybrid_search_on_persistent_collections_reopened_from_disk(tmp_path):
    from mirx.retriever import AnnSearchRequest, MilvusManager, RRFRanker, WeightedRanker
    rng = np.random.default_rng(37)
    mgr = MilvusManager(uri=str(tmp_path))
    assert mgr.connect()
    cv, dn = mgr.create_collection("convnextv2"), mgr.create_collection("dinov2")
    paths = [f"isic/{i}.jpg" for i in range(260)]
    cv.insert([paths[:200], ["m"] * 200, _rows(rng, 200, 1024)])
    dn.insert([paths[60:][::-1], ["m"] * 200, _rows(rng, 200, 512)])
    dn.delete('image_path in ["isic/100.jpg", "isic/259.jpg"]')
    cv.flush(), dn.flush()
    q1, q2 = _rows(rng, 4, 1024), _rows(rng, 4, 512)
    reqs = [AnnSearchRequest(q1, "convnextv2", limit=100), AnnSearchRequest(q2, "dinov2", limit=100, expr='image_path != "isic/61.jpg"')]

    again = MilvusManager(uri=str(tmp_path))
    assert again.connect()
    again.load_collection("convnextv2"), again.load_collection("dinov2")
    assert again.collections["dinov2"].num_entities == 198
    for rerank in (RRFRanker(), WeightedRanker(0.5, 0.5), WeightedRanker(1.0, 0.25, norm_score=False)):
        got, _, _ = _check(again.collections, reqs, rerank, 10, manager=again, exclude_keys=["isic/5.jpg", None, "isic/258.jpg", "x"])
        assert all(len(h) == 10 for h in got)
        live, _, _ = _check(mgr.collections, reqs, rerank, 10, manager=mgr, exclude_keys=["isic/5.jpg", None, "isic/258.jpg", "x"])
        assert [[(h.id, h.distance) for h in x] for x in live] == [[(h.id, h.distance) for h in x] for x in got]
    with pytest.raises(ValueError, match="medsiglip not loaded"):
        again.hybrid_search(reqs + [AnnSearchRequest(q2, "medsiglip")], RRFRanker(), 10)
