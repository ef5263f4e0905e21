"""Leave-group-out search (mirx_index_search_leave_out), the parts that need no GPU: the ctypes signature, the entry
point's refusals before any device call, the Python signatures, Collection.search's argument checks on an empty in-memory
collection, MilvusRetriever's result dicts, and the numpy restatement the GPU tests compare against (tests/_leave_out_ref.py)
against oracle.search.topk on the filtered gallery."""
import ctypes
import inspect

import numpy as np
import pytest

import _leave_out_ref as R
from oracle import search as OS

EINVAL = -1


def test_ctypes_signature():
    import mirx._lib as L
    res, args = L.SYMBOLS["mirx_index_search_leave_out"]
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert res is ctypes.c_int
    assert args == [vp, vp, i64, ctypes.c_int, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    fn = L.load().mirx_index_search_leave_out
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    assert "left_out" == L.SearchStats._fields_[-1][0] and ctypes.sizeof(L.SearchStats) == 8 * 8
    assert L.load().mirx_version() == 305


def test_entry_point_refuses_bad_arguments_before_any_device_call():
    import mirx._lib as L
    lib = L.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(ix=None, q=p, nq=1, k=10, ex=None, allow=None, rc=p, qc=p, hint=-1, val=p, f64=None, ids=p):
        return lib.mirx_index_search_leave_out(ix, q, nq, k, ex, allow, rc, qc, hint, val, f64, ids, None)

    for k in (0, -1, 1025):
        assert call(k=k) == EINVAL and b"[1, 1024]" in lib.mirx_last_error()
    assert call(rc=None) == EINVAL and b"null codes" in lib.mirx_last_error()
    assert call(qc=None) == EINVAL and b"null codes" in lib.mirx_last_error()
    assert call(q=None) == EINVAL and b"null buffer" in lib.mirx_last_error()
    assert call(ids=None) == EINVAL and b"null buffer" in lib.mirx_last_error()
    assert call(val=None, f64=None) == EINVAL and b"null buffer" in lib.mirx_last_error()
    assert call(nq=-1) == EINVAL and b"nq" in lib.mirx_last_error()
    assert call(hint=-2) == EINVAL and b"max_left_out" in lib.mirx_last_error()
    for kw in ({}, {"val": None, "f64": p}, {"hint": 0}, {"hint": 5000}, {"k": 1}, {"k": 1024}):
        assert call(**kw) == EINVAL and b"null index" in lib.mirx_last_error()     # every other argument passed the checks


def test_flatindex_search_leave_out_signature():
    from mirx.index import FlatIndex
    sig = inspect.signature(FlatIndex.search_leave_out)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", inspect.Parameter.empty), ("q", inspect.Parameter.empty), ("k", inspect.Parameter.empty),
        ("row_codes", inspect.Parameter.empty), ("query_codes", inspect.Parameter.empty), ("exclude_ids", None), ("allow", None),
        ("return_f64", False), ("max_left_out", -1)]


def test_collection_and_retriever_signatures_are_additive():
    from mirx.retriever import Collection, MilvusRetriever
    from mirx import nih, adapter
    s = inspect.signature(Collection.search).parameters
    assert list(s)[-2:] == ["leave_out_field", "leave_out_values"] and s["leave_out_field"].default is None
    assert s["leave_out_values"].default is None
    for fn in (MilvusRetriever.search, MilvusRetriever.batch_search):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "leave_out" and p["leave_out"].default is None
    assert list(inspect.signature(nih.search_collection).parameters) == ["collection", "query_vector", "top_k", "nprobe"]
    assert "exclude_self" in inspect.signature(adapter.MilvusCollectionAdapter.search_by_embeddings).parameters


def _empty_collection():
    from mirx.retriever import Collection
    return Collection("c", 8, extra_fields=("patient",))


def test_collection_search_validates_leave_out_arguments_on_an_empty_collection():
    col = _empty_collection()
    q = np.zeros((2, 8), dtype=np.float32)
    # valid arguments: empty lists, no device touched
    assert col.search(q, limit=3, leave_out_field="patient", leave_out_values=[7, None]) == [[], []]
    assert col.search(q, limit=1024, leave_out_field="image_path", leave_out_values=["a.png", "b.png"]) == [[], []]
    assert col.search(q, limit=3, leave_out_field="label", leave_out_values=(None, None), expr="label == 1",
                      exclude_ids=[0, 1]) == [[], []]
    assert col.search(q, limit=3, leave_out_field="patient", leave_out_values=["p1", "p2"],
                      param={"params": {"nprobe": 10}}) == [[], []]
    with pytest.raises(ValueError, match="image_path.*label.*patient"):
        col.search(q, limit=3, leave_out_field="diagnosis", leave_out_values=[1, 2])           # an unknown field
    with pytest.raises(ValueError, match="scalar field"):
        col.search(q, limit=3, leave_out_field="embedding", leave_out_values=[1, 2])
    with pytest.raises(ValueError, match="one value"):
        col.search(q, limit=3, leave_out_field="patient", leave_out_values=[1])                # not the query count
    with pytest.raises(ValueError, match="one value"):
        col.search(q, limit=3, leave_out_field="patient", leave_out_values=[1, 2, 3])
    with pytest.raises(ValueError, match="sequence"):
        col.search(q, limit=3, leave_out_field="patient", leave_out_values="ab")
    with pytest.raises(ValueError, match="come together"):
        col.search(q, limit=3, leave_out_field="patient")
    with pytest.raises(ValueError, match="come together"):
        col.search(q, limit=3, leave_out_values=[1, 2])
    for bad in ([1, True], [[1], 2], [1, {"a": 1}], [b"x", 1]):
        with pytest.raises(ValueError, match="type mismatch"):
            col.search(q, limit=3, leave_out_field="patient", leave_out_values=bad)            # no literal of the column's type
    with pytest.raises(ValueError, match="type mismatch"):
        col.search(q, limit=3, leave_out_field="image_path", leave_out_values=[3, "a.png"])    # image_path holds strings
    with pytest.raises(ValueError, match="1024"):
        col.search(q, limit=1025, leave_out_field="patient", leave_out_values=[1, 2])
    with pytest.raises(ValueError, match="limit"):
        col.search(q, limit=0, leave_out_field="patient", leave_out_values=[1, 2])
    with pytest.raises(ValueError, match="group_by_field"):
        col.search(q, limit=3, leave_out_field="patient", leave_out_values=[1, 2], group_by_field="label")
    for param in ({"params": {"radius": 0.5}}, {"radius": 0.5, "range_filter": 0.9}):
        with pytest.raises(ValueError, match="radius"):
            col.search(q, limit=3, leave_out_field="patient", leave_out_values=[1, 2], param=param)


def test_column_type_is_the_held_values_type():
    """with rows in the host columns (a persistent collection's metadata needs no device) the literal must be of their kind"""
    col = _empty_collection()
    col._meta["patient"].extend([3, 4])
    col._meta["label"].extend(["a", "b"])
    q = np.zeros((1, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="type mismatch.*patient holds int"):
        col._leave_out_check("patient", ["3"], 1, 10, None, None)
    with pytest.raises(ValueError, match="type mismatch.*label holds str"):
        col._leave_out_check("label", [3], 1, 10, None, None)
    col._leave_out_check("patient", [3], 1, 10, None, None)
    col._leave_out_check("patient", [np.int64(3)], 1, 10, None, None)
    col._leave_out_check("label", [None], 1, 10, None, None)


def test_retriever_dicts_with_leave_out_on_a_stub(monkeypatch):
    """search() / batch_search() hand Collection.search the leave-out keywords only when asked, and the dicts keep their keys"""
    import torch
    from mirx.retriever import Hit, MilvusRetriever

    seen = []

    class _Col:
        metric_type = "COSINE"

        def search(self, **kw):
            seen.append(kw)
            nq = kw["data"].shape[0]
            return [[Hit(1, 0.5, {"image_path": "p", "label": "l"})] for _ in range(nq)]

    class _Model(torch.nn.Module):
        def forward(self, x):
            return x.reshape(x.shape[0], -1)[:, :4] + 1.0

    r = MilvusRetriever(None, "densenet121", _Model(), lambda img: torch.zeros(3, 2, 2))
    r.collection = _Col()
    monkeypatch.setattr(r, "_device", lambda: torch.device("cpu"))
    keys = ["id", "image_path", "label", "distance", "similarity"]
    res, _ = r.search(object(), top_k=3)
    assert "leave_out_field" not in seen[-1] and "leave_out_values" not in seen[-1] and list(res[0]) == keys
    res, _ = r.search(object(), top_k=3, leave_out=("patient", 17))
    assert seen[-1]["leave_out_field"] == "patient" and seen[-1]["leave_out_values"] == [17] and list(res[0]) == keys
    res, _ = r.search(object(), top_k=3, leave_out=("image_path", None))
    assert seen[-1]["leave_out_values"] == [None]
    res = r.batch_search([object(), object()], top_k=3)
    assert "leave_out_field" not in seen[-1] and list(res[1][0]) == keys
    res = r.batch_search([object(), object()], top_k=3, leave_out=("patient", [17, None]), expr="label == 'l'")
    assert seen[-1]["leave_out_field"] == "patient" and seen[-1]["leave_out_values"] == [17, None]
    assert seen[-1]["expr"] == "label == 'l'" and list(res[0][0]) == keys
    with pytest.raises(ValueError, match="pair"):
        r.search(object(), top_k=3, leave_out="patient")


@pytest.mark.parametrize("metric", [0, 1])
def test_restatement_equals_the_oracle_on_the_filtered_gallery(metric):
    """200 rows, ties planted (duplicate rows), ids out of row order, null codes on both sides, an excluded id inside and outside
    the left-out group, a mask, and k past the eligible rows: per query the restatement equals oracle.search.topk over the
    gallery with the ineligible rows taken out."""
    rng = np.random.default_rng(38 + metric)
    n, d, nq, k = 200, 64, 12, 30
    g = rng.standard_normal((n, d)).astype(np.float32)
    g[50:60] = g[40:50]                                            # exact ties, decided by id
    ids = (rng.permutation(n) * 3 + 5).astype(np.int64)
    codes = rng.integers(-1, 6, n).astype(np.int32)
    codes[:180][codes[:180] == 5] = 4
    codes[180:] = 5                                                # a small group: 20 rows
    q = g[rng.integers(0, n, nq)] + 0.1 * rng.standard_normal((nq, d)).astype(np.float32)
    qcodes = np.array([0, 1, 2, 3, 4, 5, -1, -1, 0, 1, 77, 5], dtype=np.int32)
    exclude = ids[rng.integers(0, n, nq)].copy()
    exclude[0] = ids[np.nonzero(codes == 0)[0][0]]                 # inside the left-out group
    exclude[6] = -1
    allow = rng.random(n) < 0.7
    for ex, am, kk in ((None, None, k), (exclude, None, k), (None, allow, k), (exclude, allow, 190)):
        got_s, got_i = R.topk(q, g, kk, codes, qcodes, metric, ids=ids, exclude=ex, allow=am)
        for i in range(nq):
            ok = R.eligible(codes, int(qcodes[i]), ids, None if ex is None else int(ex[i]), am)
            m = int(ok.sum())
            want_s, want_i = OS.topk(q[i:i + 1], g[ok], min(kk, m), metric=metric, ids=ids[ok])
            np.testing.assert_array_equal(got_i[i, :min(kk, m)], want_i[0])
            np.testing.assert_array_equal(got_s[i, :min(kk, m)], want_s[0])
            assert (got_i[i, m:] == -1).all() and np.isneginf(got_s[i, m:]).all()
            assert not np.isin(got_i[i], ids[~ok]).any()
        assert (got_i[10] != -1).sum() == min(kk, int(R.eligible(codes, -1, ids, None if ex is None else int(ex[10]), am).sum()))
