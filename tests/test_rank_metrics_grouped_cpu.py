"""Leave-group-out evaluation, the parts that need no GPU: the float64 restatement (tests/_rank_metrics_ref.py)
against the reference's recorded outputs (tests/golden/grouped_300.json), the groups= numpy paths of the four metric functions
against the restatement, groups=None against the ungrouped call, the ctypes signatures and the refusals of the two new entry
points before any device call, and evaluate()'s args.groups reaching the streaming core."""
import ctypes
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

import _rank_metrics_ref as R

EINVAL = -1
KAPPAS = [1, 5, 10]


@pytest.fixture(scope="module")
def gold(golden_dir):
    with open(os.path.join(golden_dir, "grouped_300.json")) as fh:
        g = json.load(fh)
    g["embeds"] = np.asarray(g["embeds"], dtype=np.int64)
    g["labels"] = np.asarray(g["labels"], dtype=np.int64)
    g["groups"] = np.asarray(g["groups"], dtype=np.int32)
    g["ranks"] = R.self_ranking(g["embeds"], "l2")                    # [N, N] rows per query, self last
    g["res"] = R.metrics(g["ranks"], g["labels"], g["labels"], g["kappas"], gallery_codes=g["groups"], query_codes=g["groups"])
    return g


def test_fixture_is_what_its_generator_describes(gold):
    assert gold["n"] == 300 and gold["kappas"] == KAPPAS
    np.testing.assert_array_equal(gold["labels"], np.arange(300) % 3)
    np.testing.assert_array_equal(gold["groups"], R.group_sizes_1_to_8(300, gold["seed"]))
    sizes = np.bincount(gold["groups"])
    assert set(sizes.tolist()) == set(range(1, 9))


def test_restatement_equals_the_reference_on_group_compacted_lists(gold):
    mAP, aps, pr, prs = R.map_from(gold["res"], KAPPAS)
    np.testing.assert_allclose(aps, np.asarray(gold["aps"]), rtol=0, atol=1e-12)
    np.testing.assert_allclose(prs, np.asarray(gold["prs"]), rtol=0, atol=1e-12)
    assert mAP == pytest.approx(float(np.mean(gold["aps"])), abs=1e-12)
    assert not np.isnan(aps).any()


def test_compute_map_groups_numpy_path(gold):
    from mirx.metrics import compute_map
    want = R.map_from(gold["res"], KAPPAS)
    got = compute_map(gold["ranks"].T, gold["labels"], KAPPAS, groups=gold["groups"])
    assert got[0] == pytest.approx(want[0], abs=1e-12)
    for a, b in zip(got[1:], want[1:]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12)
    # groups may be strings: equal values are one group
    names = np.array([f"patient-{c:03d}" for c in gold["groups"]])
    again = compute_map(gold["ranks"].T, gold["labels"], KAPPAS, groups=names)
    assert again[0] == got[0] and np.array_equal(again[1], got[1]) and np.array_equal(again[3], got[3])


def test_groups_none_is_the_ungrouped_call(gold):
    from mirx import metrics as M
    ranks, labels = gold["ranks"], gold["labels"]
    a, b = M.compute_map(ranks.T, labels, KAPPAS), M.compute_map(ranks.T, labels, KAPPAS, groups=None)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    heads = ranks[:, :20]
    a = M.retrieval_accuracy(None, labels, topk=KAPPAS, topk_ids=heads)
    b = M.retrieval_accuracy(None, labels, topk=KAPPAS, topk_ids=heads, groups=None)
    assert np.array_equal(torch.stack(a).numpy(), torch.stack(b).numpy())
    assert M.compute_classification_metrics(labels, None, [1, 5, 20], ranks=heads.T) == \
        M.compute_classification_metrics(labels, None, [1, 5, 20], ranks=heads.T, groups=None)
    multi = np.eye(3, dtype=np.float32)[labels]
    assert M.compute_map_multilabel(None, multi, 0.5, ranks=ranks.T) == M.compute_map_multilabel(None, multi, 0.5, ranks=ranks.T, groups=None)
    for fn, name in ((M.compute_map, "groups"), (M.compute_map_multilabel, "groups"), (M.retrieval_accuracy, "groups"),
                     (M.compute_classification_metrics, "groups")):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == name and p[name].default is None


def test_all_distinct_groups_equal_self_dropped(gold):
    from mirx.metrics import compute_map
    n = 300
    got = compute_map(gold["ranks"].T, gold["labels"], KAPPAS, groups=np.arange(n))
    res = R.metrics(gold["ranks"], gold["labels"], gold["labels"], KAPPAS, query_ids=np.arange(n), drop_self=True)
    want = R.map_from(res, KAPPAS)
    assert got[0] == pytest.approx(want[0], abs=1e-12)
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[3], want[3], rtol=0, atol=1e-12)
    # and the restatement's own two roads agree exactly
    by_code = R.metrics(gold["ranks"], gold["labels"], gold["labels"], KAPPAS, gallery_codes=np.arange(n), query_codes=np.arange(n))
    for k in res:
        np.testing.assert_array_equal(res[k], by_code[k])


def test_retrieval_accuracy_and_classification_groups(gold):
    from mirx.metrics import compute_classification_metrics, majority_vote, retrieval_accuracy
    labels, groups, ranks = gold["labels"], gold["groups"], gold["ranks"]
    n = 300
    hit = (gold["res"]["cnt"] > 0).sum(axis=0)
    want = [np.float32(np.float32(h) * np.float32(100.0 / n)) for h in hit]
    got = retrieval_accuracy(None, labels, topk=KAPPAS, topk_ids=ranks, groups=groups)
    assert [float(g) for g in got] == [float(w) for w in want]
    # from a score matrix (higher = more similar), the reference's call: -inf on the diagonal puts the query last
    e = gold["embeds"].astype(np.float64)
    scores = -((e[:, None, :] - e[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(scores, -np.inf)
    got = retrieval_accuracy(scores, labels, topk=KAPPAS, groups=groups)
    assert [float(g) for g in got] == [float(w) for w in want]
    ks = [1, 5, 20]
    got = compute_classification_metrics(labels, None, ks, ranks=ranks.T, groups=groups)
    for k in ks:
        pred = np.array([majority_vote(labels[ranks[i][groups[ranks[i]] != groups[i]][:k]]) for i in range(n)])
        assert got[k]["accuracy"] == pytest.approx(100.0 * np.count_nonzero(pred == labels) / n, abs=1e-9)
    # an empty slot (id -1, FlatIndex.search_leave_out past the eligible rows) is not a vote
    heads = np.concatenate([ranks[:, :3], np.full((n, 2), -1)], axis=1)
    a = compute_classification_metrics(labels, None, [5], ranks=heads.T, groups=np.arange(n))
    b = compute_classification_metrics(labels, None, [3], ranks=ranks[:, :3].T)
    assert a[5] == b[3]


def test_multilabel_groups_numpy_path(gold):
    from mirx.metrics import _label_bitmasks, compute_map_multilabel
    rng = np.random.default_rng(5)
    n = 120
    multi = (rng.random((n, 14)) < 0.2).astype(np.float32)
    emb = rng.standard_normal((n, 6))
    ranks = R.self_ranking(emb, "ip")
    groups = R.group_sizes_1_to_8(n, 3)
    masks = _label_bitmasks(multi)
    for thr in (0.25, 0.5):
        res = R.metrics(ranks, masks, masks, (), query_ids=np.arange(n), gallery_codes=groups, query_codes=groups, jaccard=thr,
                        standard_ap=True)
        aps = res["ap"][~np.isnan(res["ap"])]
        assert compute_map_multilabel(None, multi, thr, ranks=ranks.T, groups=groups) == pytest.approx(aps.mean(), abs=1e-12)
        assert np.isnan(res["ap"]).any() or thr == 0.25                # the set has queries left without a relevant image


def test_a_query_whose_whole_class_is_its_group_is_skipped():
    from mirx.metrics import compute_map
    labels = np.array([0, 0, 0, 1, 1, 2, 2, 2])
    groups = np.array([7, 7, 7, 1, 2, 3, 4, 4])                       # class 0 is one group: its queries have nothing left
    ranks = R.self_ranking(np.arange(8, dtype=np.float64)[:, None] * np.array([[1.0, 0.5]]), "l2")
    mAP, aps, pr, prs = compute_map(ranks.T, labels, [1, 2], groups=groups)
    assert np.isnan(aps[:3]).all() and not np.isnan(aps[3:]).any() and np.isnan(prs[:3]).all()
    assert mAP == pytest.approx(np.mean(aps[3:]), abs=1e-15)
    res = R.metrics(ranks, labels, labels, [1, 2], gallery_codes=groups, query_codes=groups)
    assert int(np.isnan(res["ap"]).sum()) == 3 and (res["nrel"][:3] == 0).all() and (res["maxpos"][:3] == 0).all()
    np.testing.assert_allclose(aps[3:], res["ap"][3:], rtol=0, atol=1e-15)
    allnan = compute_map(ranks.T, labels, [1], groups=np.zeros(8, dtype=int))   # one group holds everything
    assert np.isnan(allnan[0]) and np.isnan(allnan[1]).all()
    with pytest.raises(ValueError, match="one value per image"):
        compute_map(ranks.T, labels, [1], groups=[1, 2, 3])


def test_ctypes_signatures():
    import mirx._lib as L
    vp, i64, i, d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    kp = ctypes.POINTER(ctypes.c_int32)
    base = L.SYMBOLS["mirx_rank_metrics"][1]
    res, args = L.SYMBOLS["mirx_rank_metrics_grouped"]
    assert res is i and args == base[:14] + [vp, vp] + base[14:]       # the two code arrays sit in front of the outputs
    assert args == [vp, i64, i64, i64, vp, i64, vp, vp, i, i, d, i, kp, i, vp, vp, vp, vp, vp, vp, vp]
    res, args = L.SYMBOLS["mirx_index_rank_metrics"]
    assert res is i and args == [vp, vp, i64, vp, i, vp, vp, vp, vp, i, d, i, kp, i, vp, vp, vp, vp, vp]
    lib = L.load()
    for name in ("mirx_rank_metrics_grouped", "mirx_index_rank_metrics"):
        fn = getattr(lib, name)
        assert fn.restype is i and list(fn.argtypes) == L.SYMBOLS[name][1]
    assert lib.mirx_version() == 305


def test_python_signatures():
    from mirx import evaluate as E, nih
    from mirx.index import FlatIndex
    from mirx.metrics import rank_metrics_device
    from mirx.retriever import Collection
    E_ = inspect.Parameter.empty
    sig = inspect.signature(FlatIndex.rank_metrics)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("self", E_), ("q", E_), ("row_labels", E_), ("query_labels", E_), ("kappas", ()), ("exclude_ids", None), ("self_kind", 0),
        ("row_codes", None), ("query_codes", None), ("jaccard_threshold", None), ("standard_ap", False)]
    p = inspect.signature(rank_metrics_device).parameters
    assert list(p)[-2:] == ["gallery_codes", "query_codes"] and p["gallery_codes"].default is None and p["query_codes"].default is None
    sig = inspect.signature(E.evaluate_embeddings)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("embeds", E_), ("labels", E_), ("groups", None), ("metric", "cdist"), ("kappas", (1, 5, 10)), ("k_values", (1, 5, 10, 15, 20))]
    p = inspect.signature(nih.evaluate_map).parameters
    assert list(p) == ["model", "data_loader", "device", "jaccard_threshold", "groups"] and p["groups"].default is None
    sig = inspect.signature(Collection.self_metrics)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[:5]] == [
        ("self", E_), ("label_field", "label"), ("kappas", (1, 5, 10)), ("leave_out_field", None), ("standard_ap", False)]
    assert E.FULL_RANKING_MAX_IMAGES == 65536


def test_grouped_entry_refuses_bad_arguments_before_any_device_call():
    import mirx._lib as L
    lib = L.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    k3 = (ctypes.c_int32 * 9)(1, 5, 10, 1, 1, 1, 1, 1, 1)

    def call(ranks=p, nq=1, n=4, stride=4, gl=p, nl=4, ql=p, qi=None, drop=0, rel=0, thr=0.0, apk=0, kap=k3, nk=3, gc=p, qc=p,
             ap=p, cnt=p, nrel=p, maxpos=p):
        return lib.mirx_rank_metrics_grouped(ranks, nq, n, stride, gl, nl, ql, qi, drop, rel, thr, apk, kap, nk, gc, qc, ap, cnt,
                                             nrel, maxpos, None)

    assert call(gc=None) == EINVAL and b"null codes" in lib.mirx_last_error()
    assert call(qc=None) == EINVAL and b"null codes" in lib.mirx_last_error()
    assert call(nk=9) == EINVAL and b"nk <= 8" in lib.mirx_last_error()
    assert call(nk=-1) == EINVAL
    assert call(kap=(ctypes.c_int32 * 3)(1, 0, 2)) == EINVAL and b"kappa" in lib.mirx_last_error()
    assert call(ranks=None) == EINVAL and b"null buffer" in lib.mirx_last_error()
    assert call(ap=None) == EINVAL and b"null buffer" in lib.mirx_last_error()
    assert call(cnt=None) == EINVAL
    assert call(stride=3) == EINVAL and b"bad sizes" in lib.mirx_last_error()
    assert call(nq=-1) == EINVAL and call(n=-1, stride=-1) == EINVAL and call(nl=-1) == EINVAL
    assert call(rel=2) == EINVAL and b"bad kind" in lib.mirx_last_error()
    assert call(apk=-1) == EINVAL and b"bad kind" in lib.mirx_last_error()
    assert b"rank_metrics_grouped" in lib.mirx_last_error()
    assert call(nq=0, ranks=None, gl=None, ql=None, ap=None, nrel=None, maxpos=None, nk=0, cnt=None) == 0   # nothing to do, nothing launched


def test_index_entry_refuses_bad_arguments_before_any_device_call():
    import mirx._lib as L
    lib = L.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    k3 = (ctypes.c_int32 * 9)(1, 5, 10, 1, 1, 1, 1, 1, 1)

    def call(ix=None, q=p, nq=1, ex=None, kind=0, rl=p, ql=p, rc=None, qc=None, rel=0, thr=0.0, apk=0, kap=k3, nk=3, ap=p, cnt=p,
             nrel=p, maxpos=p):
        return lib.mirx_index_rank_metrics(ix, q, nq, ex, kind, rl, ql, rc, qc, rel, thr, apk, kap, nk, ap, cnt, nrel, maxpos, None)

    assert call(rc=p) == EINVAL and b"both or neither" in lib.mirx_last_error()
    assert call(qc=p) == EINVAL and b"both or neither" in lib.mirx_last_error()
    for kind in (-1, 3):
        assert call(kind=kind) == EINVAL and b"self_kind" in lib.mirx_last_error()
    for kind in (1, 2):
        assert call(kind=kind) == EINVAL and b"need exclude_ids" in lib.mirx_last_error()
    assert call(nk=9) == EINVAL and b"nk <= 8" in lib.mirx_last_error()
    assert call(kap=(ctypes.c_int32 * 3)(0, 1, 2)) == EINVAL and b"kappa" in lib.mirx_last_error()
    assert call(nq=-1) == EINVAL and b"nq" in lib.mirx_last_error()
    assert call(q=None) == EINVAL and b"null buffer" in lib.mirx_last_error()
    assert call(ql=None) == EINVAL and call(ap=None) == EINVAL and call(nrel=None) == EINVAL and call(maxpos=None) == EINVAL
    assert call(cnt=None) == EINVAL
    assert call(rel=2) == EINVAL and call(apk=2) == EINVAL
    for kw in ({}, {"rc": p, "qc": p}, {"kind": 1, "ex": p}, {"kind": 2, "ex": p, "rc": p, "qc": p}, {"nk": 0, "cnt": None}, {"nk": 8},
               {"rel": 1, "apk": 1, "thr": 0.4}):
        assert call(**kw) == EINVAL and b"null index" in lib.mirx_last_error()     # every other argument passed the checks


def test_self_metrics_refuses_unknown_fields_without_a_device():
    from mirx.retriever import Collection
    col = Collection("c", 8, extra_fields=("patient",))
    with pytest.raises(ValueError, match="label_field 'diagnosis'.*image_path.*label.*patient"):
        col.self_metrics(label_field="diagnosis")
    with pytest.raises(ValueError, match="leave_out_field 'study'"):
        col.self_metrics(leave_out_field="study")
    with pytest.raises(ValueError, match="scalar field"):
        col.self_metrics(label_field="embedding")
    with pytest.raises(ValueError, match="kappas"):
        col.self_metrics(kappas=range(1, 10))
    with pytest.raises(ValueError, match="kappas"):
        col.self_metrics(kappas=(0,))
    out = col.self_metrics(leave_out_field="patient")                  # an empty collection: nothing to evaluate, no device
    assert out["n_queries"] == 0 and out["n_skipped"] == 0 and np.isnan(out["mAP"])


class _Lookup(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, idx):
        return self.table[idx]


def test_evaluate_hands_args_groups_to_the_streaming_core(monkeypatch, tmp_path, capsys):
    """FlatIndex has no CPU path, so the core is replaced: evaluate() must call it with the embeddings, the labels and
    args.groups, return its numbers with ranks = None and keep the .npz's metric fields."""
    from mirx import evaluate as E
    seen = {}

    def core(embeds, labels, groups=None, metric="cdist", kappas=(1, 5, 10), k_values=(1, 5, 10, 15, 20)):
        seen.update(embeds=embeds, labels=labels, groups=groups, metric=metric, kappas=list(kappas), k_values=list(k_values))
        cls = {k: {"accuracy": 50.0 + k} for k in k_values}
        return {"acc": np.array([10, 20, 30], dtype=np.float32), "mAP": 0.25, "pr": np.array([0.1, 0.2, 0.3]), "classification": cls,
                "n_queries": embeds.shape[0], "n_skipped": 2}

    def no_ranking(*a, **k):
        raise AssertionError("the [N, N] ranking must not be built")

    monkeypatch.setattr(E, "evaluate_embeddings", core)
    monkeypatch.setattr(E, "rank_self", no_ranking)
    monkeypatch.setattr(E, "_print_classification", lambda *a: None)
    monkeypatch.setattr(E, "FULL_RANKING_MAX_IMAGES", 10)
    emb = torch.randn(30, 4)
    labels = torch.arange(30) % 3
    groups = [f"p{i // 2}" for i in range(30)]
    loader = [(torch.arange(i, i + 10), labels[i:i + 10]) for i in range(0, 30, 10)]
    args = types.SimpleNamespace(save_dir=str(tmp_path), resume="ckpt/model_y.pth", groups=groups)
    res = E.evaluate(_Lookup(emb), loader, torch.device("cpu"), args)
    assert seen["groups"] is groups and seen["metric"] == "cdist" and seen["kappas"] == [1, 5, 10]
    assert seen["k_values"] == [1, 5, 10, 15, 20] and torch.equal(seen["embeds"], emb)
    np.testing.assert_array_equal(seen["labels"], labels.numpy())
    assert res["ranks"] is None and res["mAP"] == 0.25 and res["n_skipped"] == 2
    out = np.load(tmp_path / "model_y.npz")
    assert set(out.files) == {"embeds", "labels", "kappas", "acc", "mAP", "pr", "classification_k_values", "classification_k1",
                              "classification_k5", "classification_k10", "classification_k15", "classification_k20"}
    assert ">> mAP: 25.00%" in capsys.readouterr().out
    # no groups, but more images than the [N, N] ranking is built for: the same road, groups = None
    args = types.SimpleNamespace(save_dir=None, resume="x")
    res = E.evaluate(_Lookup(emb), loader, torch.device("cpu"), args)
    assert seen["groups"] is None and res["ranks"] is None
