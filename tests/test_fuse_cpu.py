"""Hybrid search, the parts that need no GPU: the rankers' and requests' argument checks, the bounds, the join codes
(first-appearance order, a collection used twice, deleted rows, a repeated key), the float64 restatement (tests/_fuse_ref.py)
on hand-worked cases, and mirx_fuse_ranked's MIRX_EINVAL paths (before any HIP call)."""
import ctypes
import math

import numpy as np
import pytest

import _fuse_ref as R


# ---- rankers and requests ----------------------------------------------------------------------------------------------
def test_rrf_ranker_validates_k():
    from mirx.retriever import RRFRanker
    assert RRFRanker().k == 60.0 and RRFRanker(1).kernel_form(["COSINE", "L2"]) == ("rrf", 1.0)
    assert RRFRanker(16383.5).k == 16383.5 and RRFRanker(np.float32(0.5)).k == 0.5
    for k in (0, -1, 16384, 1e9, float("nan"), float("inf"), "60", None, True):
        with pytest.raises(ValueError, match="k must be"):
            RRFRanker(k)


def test_weighted_ranker_validates_weights_and_metrics():
    from mirx.retriever import WeightedRanker
    w = WeightedRanker(0.5, 0.3, 0.2)
    assert w.kernel_form(["IP", "L2", "COSINE"]) == ("weighted", [0.5, 0.3, 0.2], ["IP", "L2", "COSINE"])
    assert WeightedRanker(0, 1).kernel_form(["COSINE", "COSINE"])[1] == [0.0, 1.0]
    raw = WeightedRanker(0.5, 0.5, norm_score=False)
    assert raw.kernel_form(["COSINE", "IP"]) == ("weighted", [0.5, 0.5], ["RAW", "RAW"])
    with pytest.raises(ValueError, match="L2"):
        raw.kernel_form(["COSINE", "L2"])
    for weights in ((), (1.5,), (-0.1, 0.5), (float("nan"),), ("0.5",), (None,), (True,)):
        with pytest.raises(ValueError, match="weight"):
            WeightedRanker(*weights)
    for metrics in (["COSINE"], ["COSINE", "IP", "L2", "L2"]):
        with pytest.raises(ValueError, match="3 weights"):
            w.kernel_form(metrics)
    with pytest.raises(ValueError, match="metric"):
        w.kernel_form(["COSINE", "IP", "HAMMING"])


def test_ann_search_request_validates_its_arguments():
    from mirx.retriever import AnnSearchRequest
    r = AnnSearchRequest(np.zeros((2, 8), np.float32), "dinov2", limit=np.int64(7), expr='label == "a"', param={"nprobe": 4})
    assert (r.anns_field, r.limit, r.expr, r.param) == ("dinov2", 7, 'label == "a"', {"nprobe": 4})
    assert AnnSearchRequest([0.0] * 8, "x").limit == 10
    for limit in (0, -2, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="limit"):
            AnnSearchRequest([0.0] * 8, "x", limit=limit)
    with pytest.raises(ValueError, match="param"):
        AnnSearchRequest([0.0] * 8, "x", param=[("nprobe", 4)])
    with pytest.raises(ValueError, match="expr"):
        AnnSearchRequest([0.0] * 8, "x", expr=5)


def test_fuse_bounds():
    from mirx.index import fuse_bounds
    assert fuse_bounds([10, 20], 5) == ([10, 20], 5)
    assert fuse_bounds([4096], 1024) == ([4096], 1024) and fuse_bounds([512] * 8, np.int64(1)) == ([512] * 8, 1)
    with pytest.raises(ValueError, match="4096"):
        fuse_bounds([4096, 1], 10)
    with pytest.raises(ValueError, match="4096"):
        fuse_bounds([513] + [512] * 7, 10)
    with pytest.raises(ValueError, match="1024"):
        fuse_bounds([10], 1025)
    with pytest.raises(ValueError, match="1024"):
        fuse_bounds([10], 0)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        fuse_bounds([1] * 9, 1)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        fuse_bounds([], 1)
    with pytest.raises(ValueError, match="at least 1"):
        fuse_bounds([5, 0], 1)
    for segments, limit in [([2.0], 1), ([True], 1), (["3"], 1), ([3], 2.5), ([3], None), (7, 1)]:
        with pytest.raises(ValueError):
            fuse_bounds(segments, limit)


def test_fuse_ranker_kernel_forms():
    from mirx.index import fuse_ranker
    from mirx import _lib as L
    assert fuse_ranker(("rrf", 60), 3) == (L.FUSE_RRF, 60.0, None, None)
    assert fuse_ranker(("weighted", [0.5, 1], ["L2", "RAW"]), 2) == (L.FUSE_WEIGHTED, 0.0, [0.5, 1.0], [3, 0])
    for bad, n in [(("rrf", 0), 1), (("rrf", 16384), 1), (("rrf",), 1), (("borda", 1), 1), (None, 1), (("weighted", [0.5], ["IP"]), 2),
                   (("weighted", [0.5, 2.0], ["IP", "IP"]), 2), (("weighted", [0.5], ["JACCARD"]), 1), (("weighted", [0.5]), 1)]:
        with pytest.raises(ValueError):
            fuse_ranker(bad, n)


# ---- hybrid_search's own checks (empty in-memory collections: no device is touched) -----------------------------------------
def _empty(name="a", metric="COSINE", **kw):
    from mirx.retriever import Collection
    return Collection(name, 8, metric_type=metric, **kw)


def test_hybrid_search_validates_before_any_search():
    from mirx.retriever import AnnSearchRequest, MilvusManager, RRFRanker, WeightedRanker, hybrid_search
    a, b = _empty("a"), _empty("b", "L2")
    q = np.zeros((3, 8), np.float32)
    ra, rb = AnnSearchRequest(q, "a", limit=5), AnnSearchRequest(q, "b", limit=7)
    cols = {"a": a, "b": b}
    assert hybrid_search(cols, [ra, rb], RRFRanker(), 4) == [[], [], []]
    assert hybrid_search([a, b], [ra, rb], WeightedRanker(0.5, 0.5), 4) == [[], [], []]
    assert hybrid_search(cols, [ra, ra, ra], RRFRanker(), 1024) == [[], [], []]                 # one collection, three requests
    with pytest.raises(ValueError, match="1024"):
        hybrid_search(cols, [ra, rb], RRFRanker(), 1025)
    with pytest.raises(ValueError, match="4096"):
        hybrid_search(cols, [AnnSearchRequest(q, "a", limit=4000), rb, AnnSearchRequest(q, "a", limit=90)], RRFRanker(), 4)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        hybrid_search(cols, [ra] * 9, RRFRanker(), 4)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        hybrid_search(cols, [], RRFRanker(), 4)
    with pytest.raises(ValueError, match="group_by_field"):
        hybrid_search(cols, [ra, rb], RRFRanker(), 4, group_by_field="label")
    with pytest.raises(ValueError, match="group_by_field"):
        hybrid_search(cols, [AnnSearchRequest(q, "a", param={"group_by_field": "label"}), rb], RRFRanker(), 4)
    with pytest.raises(ValueError, match="not loaded"):
        hybrid_search(cols, [ra, AnnSearchRequest(q, "c")], RRFRanker(), 4)
    with pytest.raises(ValueError, match="collections for"):
        hybrid_search([a], [ra, rb], RRFRanker(), 4)
    with pytest.raises(ValueError, match="2 weights"):
        hybrid_search(cols, [ra], WeightedRanker(0.5, 0.5), 4)
    with pytest.raises(ValueError, match="L2"):
        hybrid_search(cols, [ra, rb], WeightedRanker(0.5, 0.5, norm_score=False), 4)
    with pytest.raises(ValueError, match="rerank"):
        hybrid_search(cols, [ra, rb], "rrf", 4)
    with pytest.raises(ValueError, match="AnnSearchRequest"):
        hybrid_search(cols, [ra, {"data": q}], RRFRanker(), 4)
    with pytest.raises(ValueError, match="same number of queries"):
        hybrid_search(cols, [ra, AnnSearchRequest(q[:2], "b")], RRFRanker(), 4)
    with pytest.raises(ValueError, match="exclude_keys"):
        hybrid_search(cols, [ra, rb], RRFRanker(), 4, exclude_keys=["x"])
    with pytest.raises(ValueError, match="join_field"):
        hybrid_search(cols, [ra, rb], RRFRanker(), 4, join_field="patient")
    mgr = MilvusManager()
    mgr.collections = {"convnextv2": a, "dinov2": b}
    reqs = [AnnSearchRequest(q, "convnextv2"), AnnSearchRequest(q, "dinov2")]
    assert mgr.hybrid_search(reqs, RRFRanker(), 10) == [[], [], []]
    with pytest.raises(ValueError, match="densenet121 not loaded"):
        mgr.hybrid_search(reqs + [AnnSearchRequest(q, "densenet121")], RRFRanker(), 10)


# ---- join codes ------------------------------------------------------------------------------------------------------------
def test_join_codes_first_appearance_order():
    from mirx.retriever import join_codes
    codes, owners, id_of = join_codes([("a", ["x", "y", "z"], [10, 11, 12]), ("b", ["w", "y", "x", "v"], [0, 1, 2, 3])])
    assert [c.tolist() for c in codes] == [[0, 1, 2], [3, 1, 0, 4]] and all(c.dtype == np.int64 for c in codes)
    assert owners == [(0, 10), (0, 11), (0, 12), (1, 0), (1, 3)]                 # the row that introduced each document
    assert id_of == [{"x": 10, "y": 11, "z": 12}, {"w": 0, "y": 1, "x": 2, "v": 3}]
    assert R.join_order([["x", "y", "z"], ["w", "y", "x", "v"]]) == {"x": 0, "y": 1, "z": 2, "w": 3, "v": 4}
    codes, owners, id_of = join_codes([("a", [], [])])
    assert codes[0].shape == (0,) and owners == [] and id_of == [{}]


def test_join_codes_refuse_a_repeated_key():
    from mirx.retriever import join_codes
    with pytest.raises(ValueError, match="'y' repeats among the live rows of b"):
        join_codes([("a", ["x", "y"], [0, 1]), ("b", ["y", "z", "y"], [0, 1, 2])])
    join_codes([("a", ["x", "y"], [0, 1]), ("b", ["y", "z"], [0, 1])])           # across collections a key may repeat: it is the join


def _stored_pair(tmp_path):
    """two persistent collections (never loaded: no device) with overlapping paths and different ids"""
    from mirx.retriever import MilvusManager
    mgr = MilvusManager(uri=str(tmp_path))
    a, b = mgr.create_collection("dinov2"), mgr.create_collection("medsiglip")
    pa = [f"img/{i}.png" for i in range(6)]
    pb = [f"img/{i}.png" for i in (7, 4, 2, 9)]
    a.insert([pa, ["l"] * 6, np.zeros((6, 512), np.float32)])
    b.insert([pb, ["l"] * 4, np.zeros((4, 512), np.float32)])
    return mgr, a, b


def test_join_table_follows_deletions_and_is_built_once_per_state(tmp_path):
    from mirx.retriever import _join_table
    _, a, b = _stored_pair(tmp_path)
    t = _join_table([a, b], "image_path")
    assert [c.tolist() for c in t.codes] == [[0, 1, 2, 3, 4, 5], [6, 4, 2, 7]]
    assert t.owners[6] == (1, 0) and t.owners[4] == (0, 4) and t.id_of[1]["img/2.png"] == 2
    assert _join_table([a, b], "image_path") is t                                # same state: the same table
    assert _join_table([b, a], "image_path") is not t                            # the request order decides the codes
    assert [c.tolist() for c in _join_table([b, a], "image_path").codes] == [[0, 1, 2, 3], [4, 5, 2, 6, 1, 7]]
    a.delete('image_path in ["img/1.png", "img/4.png"]')                         # a deleted row takes no code and frees its key
    t2 = _join_table([a, b], "image_path")
    assert t2 is not t and [c.tolist() for c in t2.codes] == [[0, 1, 2, 3], [4, 5, 1, 6]]
    assert t2.owners[5] == (1, 1) and "img/4.png" not in t2.id_of[0]
    b.insert([["img/1.png"], ["l"], np.zeros((1, 512), np.float32)])             # a change of the SECOND collection drops it too
    t3 = _join_table([a, b], "image_path")
    assert t3 is not t2 and t3.codes[1].tolist() == [4, 5, 1, 6, 7]
    assert _join_table([a, b], "image_path") is t3
    b.insert([["img/9.png"], ["l"], np.zeros((1, 512), np.float32)])
    with pytest.raises(ValueError, match="img/9.png.*repeats"):
        _join_table([a, b], "image_path")
    b.delete("id == 3")                                                          # the earlier img/9.png: one live row per key again
    assert _join_table([a, b], "image_path").codes[1].tolist() == [4, 5, 1, 6, 7]


def test_join_table_of_a_collection_used_twice(tmp_path):
    """hybrid_search joins the DISTINCT collections: a collection that serves two requests is scanned once, and both requests
    (never loaded here: the join is host work) find the table of that state"""
    from mirx.retriever import _join_table
    _, a, b = _stored_pair(tmp_path)
    t = _join_table([a], "image_path")
    assert len(t.codes) == 1 and t.codes[0].tolist() == list(range(6)) and t.owners == [(0, i) for i in range(6)]
    assert _join_table([a], "image_path") is t and _join_table([a, b], "image_path") is not t
    with pytest.raises(ValueError, match="repeats"):
        _join_table([a], "label")                                                # every row carries label "l": not a join key


# ---- the restatement, by hand --------------------------------------------------------------------------------------------
def test_restatement_rrf_by_hand():
    lists = [[(0, 0.9), (1, 0.8)], [(1, 0.7), (2, 0.6)]]
    got = R.fuse_query(lists, ("rrf", 60), 10)
    assert got == [(1, 1.0 / 62.0 + 1.0 / 61.0, 0, 1), (0, 1.0 / 61.0, 0, 0), (2, 1.0 / 62.0, 1, 1)]
    assert R.fuse_query(lists, ("rrf", 60), 1) == got[:1]
    # equal ranks in disjoint lists tie: the lower code wins, whatever the request order
    assert [c for c, *_ in R.fuse_query([[(5, 0.1), (3, 0.0)], [(4, 0.9), (1, 0.8)]], ("rrf", 60), 10)] == [4, 5, 1, 3]
    # an empty slot keeps its rank; a wholly empty list adds nothing
    assert R.fuse_query([[(-1, 0.0), (7, 0.5)], [(-1, 0.0)]], ("rrf", 1), 10) == [(7, 1.0 / 3.0, 0, 1)]
    assert R.fuse_query([[(-1, 0.0)]], ("rrf", 1), 10) == []
    # R = 1: the list itself, in order
    assert [c for c, *_ in R.fuse_query([[(9, 0.1), (2, 0.5), (4, 0.3)]], ("rrf", 60), 10)] == [9, 2, 4]
    assert R.fuse_query([[(9, 0.1), (12, 0.5)]], ("rrf", 60), 10, n_codes=10) == [(9, 1.0 / 61.0, 0, 0)]


def test_restatement_weighted_by_hand():
    cos = ("weighted", [0.5, 0.25], ["COSINE", "COSINE"])
    got = R.fuse_query([[(0, 1.0), (1, 0.0)], [(1, 1.0), (2, -1.0)]], cos, 10)
    assert got == [(0, 0.5, 0, 0), (1, 0.5, 0, 1), (2, 0.0, 1, 1)]                          # 0.5 * 1 = 0.25 + 0.25: tie by code
    ip = R.fuse_query([[(0, 1.0)], [(0, -1.0)]], ("weighted", [1.0, 1.0], ["IP", "IP"]), 10)
    assert ip[0][1] == (0.5 + math.atan(1.0) / math.pi) + (0.5 + math.atan(-1.0) / math.pi) and abs(ip[0][1] - 1.0) < 1e-15
    l2 = R.fuse_query([[(3, 0.0), (4, 1.0)]], ("weighted", [1.0], ["L2"]), 10)
    assert l2[0][:2] == (3, 1.0) and abs(l2[1][1] - 0.5) < 1e-15                             # distance 0 -> 1, distance 1 -> 1/2
    raw = R.fuse_query([[(0, 0.5)], [(0, 0.25), (1, 0.75)]], ("weighted", [1.0, 0.5], ["RAW", "RAW"]), 10)
    assert raw == [(0, 0.625, 0, 0), (1, 0.375, 1, 1)]
    # separate multiply and add: the product is rounded before it is added
    w, d1, d2 = 0.1, float(np.float32(0.3)), float(np.float32(0.7))
    two = R.fuse_query([[(0, d1)], [(0, d2)]], ("weighted", [w, w], ["RAW", "RAW"]), 1)[0][1]
    assert two == (0.0 + w * d1) + w * d2
    assert R.min_gap([got]) == 0.5 and R.min_gap([[]]) == math.inf


def test_restatement_tensor_form_and_first_found():
    codes = np.array([[3, 1, -1, 1, 2], [0, -1, -1, 0, -1]])
    dist = np.zeros(codes.shape, np.float32)
    res = R.fuse(codes, dist, [3, 2], ("rrf", 2), 2)
    assert [r[:1] + r[2:] for r in res[0]] == [(1, 0, 1), (3, 0, 0)] and res[0][0][1] == 1.0 / 4.0 + 1.0 / 3.0
    assert res[1] == [(0, 1.0 / 3.0 + 1.0 / 3.0, 0, 0)]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_fuse_ranked_refuses_bad_arguments_without_gpu():
    import mirx._lib as L
    lib = L.load()
    E = -1                                                                     # MIRX_EINVAL
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(offsets=(0, 3, 5), ranker=L.FUSE_RRF, k=60.0, weights=None, norms=None, limit=4, nq=1, stride=5, n_codes=9, codes=p,
             dist=p, out=p, n_requests=None):
        n = len(offsets) - 1 if n_requests is None else n_requests
        off = (ctypes.c_int32 * len(offsets))(*offsets) if offsets is not None else None
        w = (ctypes.c_double * len(weights))(*weights) if weights is not None else None
        nm = (ctypes.c_int32 * len(norms))(*norms) if norms is not None else None
        return lib.mirx_fuse_ranked(codes, dist, nq, stride, n_codes, off, n, ranker, k, w, nm, limit, out, out, out, out, out, None)

    def refused(why, **kw):
        assert call(**kw) == E, kw
        assert b"fuse_ranked" in lib.mirx_last_error() and why in lib.mirx_last_error(), lib.mirx_last_error()

    refused(b"n_requests", offsets=(0,), n_requests=0)
    refused(b"n_requests", offsets=tuple(range(10)))
    refused(b"limit", limit=0)
    refused(b"limit", limit=1025)
    refused(b"segment_offsets", offsets=None, n_requests=2)
    refused(b"start at 0", offsets=(1, 3, 5))
    refused(b"ascend", offsets=(0, 3, 3))
    refused(b"ascend", offsets=(0, 3, 2))
    refused(b"4096", offsets=(0, 4000, 4097), stride=4097)
    refused(b"bad sizes", stride=4)
    refused(b"bad sizes", nq=-1)
    refused(b"bad sizes", nq=2 ** 31)
    refused(b"n_codes", n_codes=-1)
    refused(b"n_codes", n_codes=2 ** 31)
    refused(b"unknown ranker", ranker=2)
    for k in (0.0, -1.0, 16384.0, float("nan"), float("inf")):
        refused(b"rrf_k", k=k)
    refused(b"weights and norms", ranker=L.FUSE_WEIGHTED)
    refused(b"weights and norms", ranker=L.FUSE_WEIGHTED, weights=(0.5, 0.5))
    refused(b"weight must be", ranker=L.FUSE_WEIGHTED, weights=(0.5, 1.5), norms=(1, 1))
    refused(b"weight must be", ranker=L.FUSE_WEIGHTED, weights=(float("nan"), 0.5), norms=(1, 1))
    refused(b"unknown norm", ranker=L.FUSE_WEIGHTED, weights=(0.5, 0.5), norms=(1, 4))
    refused(b"needs distances", ranker=L.FUSE_WEIGHTED, weights=(0.5, 0.5), norms=(1, 2), dist=None)
    refused(b"null codes", codes=None)
    refused(b"null output", out=None)
    # nothing to do is no error and touches no device
    assert call(nq=0, codes=None, dist=None, out=None) == 0
    assert call(nq=0, offsets=(0, 4096), stride=4096, limit=1024) == 0
    assert (L.FUSE_MAX_REQUESTS, L.FUSE_MAX_ENTRIES, L.FUSE_MAX_LIMIT) == (8, 4096, 1024)
