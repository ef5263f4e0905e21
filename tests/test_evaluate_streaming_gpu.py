"""The streaming evaluation drivers on the MI355X: evaluate_embeddings against evaluate()'s numbers and against the
reference's recorded leave-group-out outputs, evaluate() / evaluate_multilabels() / nih.evaluate_map() on the streaming road with
and without groups, and Collection.self_metrics against evaluate_embeddings on the same rows."""
import json
import os
import types

import numpy as np
import pytest
import torch

import _rank_metrics_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KAPPAS = [1, 5, 10]
KS = [1, 5, 10, 15, 20]


class _Lookup(torch.nn.Module):
    def __init__(self, table, as_dict=False):
        super().__init__()
        self.register_buffer("table", table)
        self.as_dict = as_dict

    def forward(self, idx):
        return {"embedding": self.table[idx]} if self.as_dict else self.table[idx]


def _loader(labels, step=64):
    n = labels.shape[0]
    return [(torch.arange(i, min(i + step, n)), labels[i:i + step]) for i in range(0, n, step)]


@pytest.fixture(scope="module")
def covidx(golden_dir):
    z = np.load(os.path.join(golden_dir, "evaluate_covidx300_d64.npz"))
    emb, labels = torch.as_tensor(z["embeds"]), torch.as_tensor(z["labels"])
    from mirx.evaluate import evaluate
    args = types.SimpleNamespace(save_dir=None, resume="x")
    parent = evaluate(_Lookup(emb).cuda(), _loader(labels), DEV, args)            # the [N, N] road, as before
    return emb, labels, parent


@pytest.fixture(scope="module")
def gold(golden_dir):
    with open(os.path.join(golden_dir, "grouped_300.json")) as fh:
        g = json.load(fh)
    g["embeds"] = np.asarray(g["embeds"], dtype=np.int64)             # integers: every distance is exact, ties go by id
    g["labels"] = np.asarray(g["labels"], dtype=np.int64)
    g["groups"] = np.asarray(g["groups"], dtype=np.int32)
    return g


def _same_numbers(got, want, what=""):
    assert got["mAP"] == pytest.approx(want["mAP"], abs=1e-12), what
    np.testing.assert_allclose(got["pr"], want["pr"], rtol=0, atol=1e-12, err_msg=what)
    np.testing.assert_array_equal(got["acc"], want["acc"], err_msg=what)           # integer-derived: exactly
    assert got["classification"] == want["classification"], what


def test_evaluate_embeddings_without_groups_is_evaluate(covidx):
    from mirx.evaluate import evaluate_embeddings
    emb, labels, parent = covidx
    got = evaluate_embeddings(emb.cuda(), labels)
    _same_numbers(got, parent)
    assert got["n_queries"] == 300 and got["n_skipped"] == 0
    assert got["acc"].dtype == np.float32 and list(got["classification"]) == KS


def test_evaluate_takes_the_streaming_road_past_the_cap(covidx, monkeypatch, tmp_path):
    from mirx import evaluate as E
    emb, labels, parent = covidx
    monkeypatch.setattr(E, "FULL_RANKING_MAX_IMAGES", 100)
    args = types.SimpleNamespace(save_dir=str(tmp_path), resume="ckpt/model_s.pth")
    got = E.evaluate(_Lookup(emb).cuda(), _loader(labels), DEV, args)
    assert got["ranks"] is None and got["n_skipped"] == 0
    _same_numbers(got, parent)
    out = np.load(tmp_path / "model_s.npz")
    assert "dists" not in out.files and float(out["mAP"]) == got["mAP"]
    np.testing.assert_array_equal(out["classification_k20"], np.array(list(parent["classification"][20].values())))


def test_with_groups_equals_the_reference_on_compacted_lists(gold, monkeypatch, tmp_path):
    from mirx import evaluate as E
    from mirx.metrics import majority_vote
    emb = torch.as_tensor(gold["embeds"], dtype=torch.float32)
    labels, groups = gold["labels"], gold["groups"]
    got = E.evaluate_embeddings(emb.cuda(), labels, groups=[f"patient {c}" for c in groups])
    aps, prs = np.asarray(gold["aps"]), np.asarray(gold["prs"])       # recorded from the reference's compute_ap / compute_map
    assert got["mAP"] == pytest.approx(aps.mean(), abs=1e-12)
    np.testing.assert_allclose(got["pr"], prs.mean(axis=0), rtol=0, atol=1e-12)
    assert got["n_skipped"] == 0
    ranks = R.self_ranking(gold["embeds"], "l2")
    kept = [ranks[i][groups[ranks[i]] != groups[i]] for i in range(300)]
    for j, kap in enumerate(KAPPAS):
        hits = sum(bool((labels[kept[i][:kap]] == labels[i]).any()) for i in range(300))
        assert got["acc"][j] == np.float32(np.float32(hits) * np.float32(100.0 / 300))
    for k in KS:
        pred = np.array([majority_vote(labels[kept[i][:k]]) for i in range(300)])
        assert got["classification"][k]["accuracy"] == pytest.approx(100.0 * np.count_nonzero(pred == labels) / 300, abs=1e-9)
    # evaluate() with args.groups: the same numbers, no ranking, the .npz without groups' trace but with dists (N <= the cap)
    args = types.SimpleNamespace(save_dir=str(tmp_path), resume="ckpt/model_g.pth", groups=groups)
    res = E.evaluate(_Lookup(emb).cuda(), _loader(torch.as_tensor(labels)), DEV, args)
    assert res["ranks"] is None
    _same_numbers(res, got)
    out = np.load(tmp_path / "model_g.npz")
    assert out["dists"].shape == (300, 300) and np.isposinf(np.diag(out["dists"])).all()
    e = gold["embeds"].astype(np.float64)
    np.testing.assert_allclose(out["dists"][0, 1:], np.sqrt(((e[0] - e[1:]) ** 2).sum(-1)), rtol=1e-6)


def _multilabel_world():
    rng = np.random.default_rng(7)
    n = 240
    labels = (rng.random((n, 14)) < 0.15).astype(np.float32)
    emb = labels @ rng.standard_normal((14, 24)).astype(np.float32) + 0.7 * rng.standard_normal((n, 24)).astype(np.float32)
    return torch.as_tensor(emb), torch.as_tensor(labels), R.group_sizes_1_to_8(n, 11)


def test_evaluate_multilabels_streaming(monkeypatch, capsys):
    from mirx import evaluate as E
    from mirx.metrics import _label_bitmasks, compute_map_multilabel
    emb, labels, groups = _multilabel_world()
    model, loader = _Lookup(emb).cuda(), _loader(labels)
    args = types.SimpleNamespace(save_dir=None)
    parent = E.evaluate_multilabels(model, loader, DEV, args)         # the [N, N] road
    monkeypatch.setattr(E, "FULL_RANKING_MAX_IMAGES", 100)
    got = E.evaluate_multilabels(model, loader, DEV, args)            # the same numbers without the ranking
    for t in (0.25, 0.5):
        assert got["mAP"][t] == pytest.approx(parent["mAP"][t], abs=1e-12)
    assert got["precision"] == parent["precision"] and got["recall"] == parent["recall"]
    # with groups: the walk over rank_all's ranking, and heads computed here from that ranking
    args = types.SimpleNamespace(save_dir=None, groups=groups)
    got = E.evaluate_multilabels(model, loader, DEV, args)
    norm = torch.nn.functional.normalize(emb.cuda().float(), p=2, dim=1)
    ranks, _ = E.rank_self(norm, "cosine")
    for t in (0.25, 0.5):
        want = compute_map_multilabel(None, labels, threshold=t, ranks=ranks.t(), groups=groups)
        assert got["mAP"][t] == pytest.approx(float(want), abs=1e-12)
        masks = _label_bitmasks(labels)
        res = R.metrics(ranks.cpu().numpy(), masks, masks, (), query_ids=np.arange(240), gallery_codes=groups, query_codes=groups,
                        jaccard=t, standard_ap=True)
        assert got["mAP"][t] == pytest.approx(np.nanmean(res["ap"]), abs=1e-12)
    r, lab = ranks.cpu().numpy(), labels.numpy()
    for k in KS:
        cnt = np.array([int(((lab[r[i][groups[r[i]] != groups[i]][:k]] * lab[i]).sum(axis=1) > 0).sum()) for i in range(240)])
        assert got["precision"][k] == pytest.approx(float((cnt / k).sum() / 240 * 100), abs=1e-9)
        assert got["recall"][k] == pytest.approx(float((cnt > 0).sum() / 240 * 100), abs=1e-9)
    assert "VinDr-CXR Retrieval Results" in capsys.readouterr().out


def test_nih_evaluate_map_with_and_without_groups():
    from mirx import nih
    from mirx.index import FlatIndex
    from mirx.metrics import _label_bitmasks, rank_metrics_device
    emb, labels, groups = _multilabel_world()
    model, loader = _Lookup(emb, as_dict=True).cuda(), _loader(labels)
    got = nih.evaluate_map(model, loader, DEV, 0.4)
    # the branch this call had before: rank_all, then the walk over the [N, N] ranking
    unit = torch.nn.functional.normalize(emb.cuda().float(), dim=1)
    ix = FlatIndex(24, "IP", 0)
    ix.add(unit)
    ranks = ix.rank_all(unit, exclude_ids=torch.arange(240))
    masks = _label_bitmasks(labels)
    ap = rank_metrics_device(ranks, masks, masks, (), jaccard_threshold=0.4, standard_ap=True)["ap"].cpu().numpy()
    assert got == pytest.approx(float(np.mean(ap[~np.isnan(ap)]) * 100.0), abs=1e-10)
    grouped = nih.evaluate_map(model, loader, DEV, 0.4, groups=groups)
    res = R.metrics(ranks.cpu().numpy(), masks, masks, (), gallery_codes=groups, query_codes=groups, jaccard=0.4, standard_ap=True)
    assert grouped == pytest.approx(float(np.nanmean(res["ap"]) * 100.0), abs=1e-10)
    assert grouped != got


def _collection_world(gold):
    emb = gold["embeds"].astype(np.float32)
    emb = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    return emb.astype(np.float32), gold["labels"], gold["groups"]


def _self_metrics_equal(col, emb, labels, groups, label_field="label"):
    from mirx.evaluate import evaluate_embeddings
    for field, g in ((None, None), ("patient", groups)):
        got = col.self_metrics(label_field=label_field, kappas=KAPPAS, leave_out_field=field, chunk_rows=128)
        want = evaluate_embeddings(torch.as_tensor(emb).cuda(), labels, groups=g, metric="cosine", kappas=KAPPAS)
        assert got["mAP"] == pytest.approx(want["mAP"], abs=1e-12), field
        np.testing.assert_allclose(got["pr"], want["pr"], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(got["acc"], want["acc"])
        assert got["n_queries"] == len(labels) and got["n_skipped"] == want["n_skipped"]
    return got


def test_collection_self_metrics_int_and_string_fields_delete_and_compact(gold):
    from mirx.retriever import Collection
    emb, labels, groups = _collection_world(gold)
    n = 300
    col = Collection("self_metrics", emb.shape[1], extra_fields=("patient", "finding"))
    col.insert([[f"img/{i}.png" for i in range(n)], [int(v) for v in labels], emb, [f"P{c:03d}" for c in groups],
                [("normal", "pneumonia", "covid")[v] for v in labels]])
    grouped = _self_metrics_equal(col, emb, labels, groups)                        # int labels, string groups
    by_name = col.self_metrics(label_field="finding", kappas=KAPPAS, leave_out_field="patient")       # string labels
    assert by_name["mAP"] == grouped["mAP"] and np.array_equal(by_name["pr"], grouped["pr"])
    # every row its own group == the row itself taken out; the standard AP road runs and skips nobody
    std = col.self_metrics(kappas=KAPPAS, leave_out_field="image_path", standard_ap=True)
    std2 = col.self_metrics(kappas=KAPPAS, standard_ap=True)
    assert std["mAP"] == std2["mAP"] and std["n_skipped"] == 0 and 0.3 < std["mAP"] < 1.0
    gone = list(range(5, n, 7))
    col.delete(f"id in {gone}")
    keep = np.setdiff1d(np.arange(n), gone)
    after = _self_metrics_equal(col, emb[keep], labels[keep], groups[keep])
    col.compact()
    again = col.self_metrics(kappas=KAPPAS, leave_out_field="patient", chunk_rows=128)
    assert again["mAP"] == after["mAP"] and np.array_equal(again["acc"], after["acc"])


def test_collection_self_metrics_on_a_reopened_file_backed_collection(gold, tmp_path):
    from mirx.retriever import Collection
    from mirx.store import Store
    emb, labels, groups = _collection_world(gold)
    n = 300
    schema = ("id", "image_path", "label", "embedding", "patient")
    col = Collection.from_stored(Store(tmp_path / "db").create("studies", emb.shape[1], "COSINE", schema=schema))
    col.insert([[f"img/{i}.png" for i in range(n)], [int(v) for v in labels], emb, [int(c) for c in groups]])   # int groups
    col.delete("id in [3, 150, 299]")
    col.flush()
    keep = np.setdiff1d(np.arange(n), [3, 150, 299])
    again = Collection.from_stored(Store(tmp_path / "db").open("studies", emb.shape[1], "COSINE", schema=schema))
    assert again._index is None                                       # the evaluation loads the rows itself
    _self_metrics_equal(again, emb[keep], labels[keep], groups[keep])
