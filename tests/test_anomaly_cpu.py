"""mirx.anomaly without a GPU: the numpy path against the goldens recorded from the reference's anomaly.py and scikit-learn
(tests/golden/make_golden_anomaly.py), against the float64 restatement (tests/_anomaly_ref.py), the error cases, the ABI's
limits and the .npz of evaluate() with a stand-in model.  Measures agree to 1e-12, the project's bound for reports."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _anomaly_ref as R  # noqa: E402

TOL = 1e-12


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "anomaly_ref.json")) as fh:
        return json.load(fh)


def _stack(case):
    pos, neg = np.array(case["pos"]), np.array(case["neg"])
    return np.concatenate((pos, neg)), np.r_[np.ones(pos.size, bool), np.zeros(neg.size, bool)]


def test_golden_covers_the_cases_and_the_versions(golden):
    assert golden["sklearn"] == "1.7.2" and golden["recall_level"] == 0.95
    for name in ["s300", "quant8", "all_equal", "one_positive", "one_negative", "n2"] + [f"tie_p{p}" for p in (1, 10, 19, 20, 21)]:
        assert name in golden["cases"], name
    assert len(golden["cases"]["s300"]["pos"]) == 100 and len(golden["cases"]["s300"]["neg"]) == 200
    assert len(golden["cases"]["quant8"]["pos"]) == 60 and len(golden["cases"]["quant8"]["neg"]) == 140
    assert len(set(golden["cases"]["quant8"]["pos"] + golden["cases"]["quant8"]["neg"])) == 8
    assert abs(golden["cases"]["quant8"]["auroc"] - 4071 / 8400) < TOL
    # the recall-level tie: FPR 0.44 at every P
    for p, a in zip((1, 10, 19, 20, 21), (0.56, 0.816, 0.8147368421052632, 0.815, 0.8157142857142858)):
        c = golden["cases"][f"tie_p{p}"]
        assert abs(c["fpr"] - 0.44) < TOL and abs(c["auroc"] - a) < TOL
    # the defect of the reference's line 64, recorded and not matched
    d = golden["line64_defect"]
    assert d["auroc"] is None and d["aupr"] == 0.0 and abs(d["fpr"] - 1 / d["n"]) < TOL and d["warnings"] == 3


def test_get_measures_matches_the_reference(golden):
    import mirx.anomaly as A
    for name, c in golden["cases"].items():
        auroc, aupr, fpr = A.get_measures(c["pos"], c["neg"])
        assert not A.last_native
        for got, key in ((auroc, "auroc"), (aupr, "aupr"), (fpr, "fpr")):
            assert abs(got - c[key]) <= TOL, (name, key, got, c[key])
        sc, pos = _stack(c)
        assert abs(A.fpr_and_fdr_at_recall(pos.astype(np.int32), sc) - c["fpr"]) <= TOL, name
        # and the float64 restatement agrees with the reference too
        m = R.measures(sc, pos)
        for key in ("auroc", "aupr", "fpr"):
            assert abs(m[key] - c[key]) <= TOL, (name, key)


def test_compact_arrays_equal_the_restatement(golden):
    import mirx.anomaly as A
    for name, c in golden["cases"].items():
        sc, pos = _stack(c)
        got, ref = A.binary_metrics(sc, pos), R.measures(sc, pos)
        for key in ("thresholds", "tps", "fps"):
            assert np.array_equal(got[key], ref[key]), (name, key)
        assert got["tps"].dtype == np.int64 and got["fps"].dtype == np.int64 and got["thresholds"].dtype == np.float64
        # any order of equal scores gives the same arrays
        perm = np.random.default_rng(3).permutation(sc.size)
        again = A.binary_metrics(sc[perm], pos[perm])
        for key in ("thresholds", "tps", "fps"):
            assert np.array_equal(again[key], ref[key]), (name, key)
        assert again["auroc"] == got["auroc"] and again["fpr"] == got["fpr"] and abs(again["aupr"] - got["aupr"]) <= TOL


def test_curves_match_scikit_learn(golden):
    import mirx.anomaly as A
    for name in ("s300", "quant8"):
        c = golden["cases"][name]
        sc, pos = _stack(c)
        m = A.binary_metrics(sc, pos)
        fpr, tpr, thr = A.roc_curve(m["thresholds"], m["tps"], m["fps"])
        assert thr[0] == np.inf and np.array_equal(thr[1:], np.array(c["roc"]["thresholds"]))
        assert fpr.shape == np.shape(c["roc"]["fpr"]) and np.abs(fpr - c["roc"]["fpr"]).max() <= TOL
        assert np.abs(tpr - c["roc"]["tpr"]).max() <= TOL
        prec, rec, thr2 = A.precision_recall_curve(m["thresholds"], m["tps"], m["fps"])
        assert prec.shape == np.shape(c["pr"]["precision"]) and np.abs(prec - c["pr"]["precision"]).max() <= TOL
        assert np.abs(rec - c["pr"]["recall"]).max() <= TOL and np.array_equal(thr2, np.array(c["pr"]["thresholds"]))
        for a, b in zip(R.roc_curve(m["thresholds"], m["tps"], m["fps"]), (fpr, tpr, thr)):
            assert np.array_equal(a, b)
        for a, b in zip(R.precision_recall_curve(m["thresholds"], m["tps"], m["fps"]), (prec, rec, thr2)):
            assert np.array_equal(a, b)
    full = A.roc_curve(m["thresholds"], m["tps"], m["fps"], drop_intermediate=False)
    assert len(full[0]) == len(m["tps"]) + 1


def test_segments_are_independent(golden):
    import mirx.anomaly as A
    c = golden["cases"]["quant8"]
    sc, pos = _stack(c)
    rng = np.random.default_rng(1)
    S = np.stack([sc, rng.permutation(sc), rng.random(sc.size)])
    Pm = np.stack([pos, rng.permutation(pos), pos])
    m = A.binary_metrics(S, Pm)
    for i in range(3):
        one = A.binary_metrics(S[i], Pm[i])
        assert one["auroc"] == m["auroc"][i] and one["aupr"] == m["aupr"][i] and one["fpr"] == m["fpr"][i]
        assert np.array_equal(one["tps"], m["tps"][i])


def test_error_cases():
    import mirx.anomaly as A
    with pytest.raises(ValueError):
        A.get_measures([], [0.1, 0.2])
    with pytest.raises(ValueError):
        A.get_measures([0.3], [])
    with pytest.raises(ValueError, match="NaN or infinite"):
        A.binary_metrics([0.1, np.nan, 0.3], [1, 0, 0])
    with pytest.raises(ValueError, match="NaN or infinite"):
        A.binary_metrics([0.1, np.inf, 0.3], [1, 0, 0])
    with pytest.raises(ValueError, match="without positives"):
        A.binary_metrics([0.1, 0.2], [0, 0])
    with pytest.raises(ValueError, match="without positives"):
        A.binary_metrics([0.1, 0.2], [1, 1])
    with pytest.raises(ValueError):
        A.binary_metrics([0.1, 0.2], [1, 0], recall_level=1.5)
    with pytest.raises(ValueError, match="without rows"):
        A.class_centroids(np.ones((4, 3), np.float32), [0, 0, 0, 0], (0, 1))
    with pytest.raises(ValueError, match="largest distance is 0"):
        A.centroid_scores(np.ones((4, 3), np.float32), np.ones((1, 3)))
    with pytest.raises(ValueError, match="not binary"):
        A.fpr_and_fdr_at_recall(np.array([0, 1, 2]), np.array([0.1, 0.2, 0.3]))
    assert np.array_equal(A.stable_cumsum(np.array([[1, 2], [3, 4]], dtype=np.int8)), [1.0, 3.0, 6.0, 10.0])
    assert A.stable_cumsum([]).size == 0
    # a running sum that loses what pairwise summation keeps
    drift = np.r_[1e16, np.ones(4096)]
    assert A.stable_cumsum(drift)[-1] == 1e16                    # inside the default tolerances
    with pytest.raises(RuntimeError):
        A.stable_cumsum(drift, rtol=0.0, atol=1.0)
    for ok in ([0, 1, 1], [-1, 1], [1, 1], [0, 0]):
        if len(set(ok)) == 2:
            A.fpr_and_fdr_at_recall(np.array(ok), np.arange(len(ok)) * 0.1)


def test_printed_reports_match_the_reference(golden, capsys):
    """The four printers write, byte for byte, what the reference's wrote for the same arguments (recorded in the golden)."""
    import mirx.anomaly as A
    c, g = golden["cases"], golden["printed"]
    pq, nq = np.array(c["quant8"]["pos"]), np.array(c["quant8"]["neg"])
    pt, nt = np.array(c["tie_p10"]["pos"]), np.array(c["tie_p10"]["neg"])
    calls = {"show_performance": lambda: A.show_performance(pq, nq),
             "show_performance_named": lambda: A.show_performance(pq, nq, method_name="Centroid", recall_level=0.9),
             "print_measures": lambda: A.print_measures(*g["print_measures"]["args"]),
             "print_measures_named": lambda: A.print_measures(*g["print_measures_named"]["args"]),
             "print_measures_with_std": lambda: A.print_measures_with_std(*g["print_measures_with_std"]["args"]),
             "show_performance_comparison": lambda: A.show_performance_comparison(pt, nt, pq, nq)}
    assert sorted(calls) == sorted(g)
    capsys.readouterr()
    for name, fn in calls.items():
        fn()
        assert capsys.readouterr().out == g[name]["out"], name


def test_reference_names_and_signatures():
    import inspect
    import mirx.anomaly as A
    assert A.recall_level_default == 0.95
    sig = {n: list(inspect.signature(getattr(A, n)).parameters) for n in
           ("stable_cumsum", "fpr_and_fdr_at_recall", "get_measures", "show_performance", "print_measures",
            "print_measures_with_std", "show_performance_comparison", "evaluate")}
    assert sig["stable_cumsum"] == ["arr", "rtol", "atol"]
    assert sig["fpr_and_fdr_at_recall"] == ["y_true", "y_score", "recall_level", "pos_label"]
    assert sig["get_measures"] == ["_pos", "_neg", "recall_level"]
    assert sig["show_performance"] == ["pos", "neg", "method_name", "recall_level"]
    assert sig["print_measures"] == ["auroc", "aupr", "fpr", "method_name", "recall_level"]
    assert sig["print_measures_with_std"] == ["aurocs", "auprs", "fprs", "method_name", "recall_level"]
    assert sig["show_performance_comparison"] == ["pos_base", "neg_base", "pos_ours", "neg_ours", "baseline_name", "method_name",
                                                  "recall_level"]
    assert sig["evaluate"] == ["model", "train_loader", "test_loader", "device", "args"]
    src = open(A.__file__).read()
    assert "sklearn" not in src.replace("scikit-learn", "")          # the numpy path imports no scikit-learn


def test_centroids_and_scores_numpy_path():
    import mirx.anomaly as A
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((50, 9)).astype(np.float32)
    labels = rng.integers(0, 4, 50)
    cent, counts = A.class_centroids(rows, labels, (0, 1, 3), return_counts=True)
    ref, rc = R.centroids(rows, labels, (0, 1, 3))
    assert cent.dtype == np.float64 and np.array_equal(counts, rc) and np.abs(cent - ref).max() <= 1e-15
    d, nearest = A.centroid_scores(rows, cent)
    rd, rn = R.min_dist(rows, ref)
    assert d.max() == 1.0 and np.abs(d - rd / rd.max()).max() <= 1e-14 and np.array_equal(nearest, rn)
    # the lowest class wins a tie
    two = np.stack([cent[0], cent[0]])
    assert not A.centroid_scores(rows, two)[1].any()


def test_abi_limits_without_a_gpu():
    from mirx import _lib as L
    lib = L.load()
    assert lib.mirx_class_centroids_workspace_bytes(0, 8, 2) == -1 and b"n must be" in lib.mirx_last_error()
    assert lib.mirx_class_centroids_workspace_bytes(10, 16385, 2) == -1 and b"d must be" in lib.mirx_last_error()
    assert lib.mirx_class_centroids_workspace_bytes(10, 8, 65) == -1 and b"k must be" in lib.mirx_last_error()
    assert lib.mirx_class_centroids_workspace_bytes(300, 64, 2) > 0
    assert lib.mirx_binary_rank_metrics_workspace_bytes(0, 10) == -1 and lib.mirx_binary_rank_metrics_workspace_bytes(1, 0) == -1
    assert lib.mirx_binary_rank_metrics_workspace_bytes(1, (1 << 30) + 1) == -1
    assert lib.mirx_binary_rank_metrics_workspace_bytes(65536, 4) == -1
    assert lib.mirx_binary_rank_metrics_workspace_bytes(3, 4097) >= 3 * 4097 * 24
    assert lib.mirx_class_centroids(None, 10, 8, None, None, 2, None, 0, None, None, None, None) == -1
    assert b"null" in lib.mirx_last_error()
    assert lib.mirx_centroid_min_dist(None, 10, 8, None, 0, None, None, None, None) == -1 and b"k must be" in lib.mirx_last_error()
    assert lib.mirx_binary_rank_metrics(None, None, 1, 4, None, 2.0, None, 0, None, None, None, None, None, None, None, None,
                                        None) == -1
    assert b"recall_level" in lib.mirx_last_error()


def test_evaluate_npz_fields_with_a_standin_model(tmp_path, capsys):
    import mirx.anomaly as A
    model, train, test = R.standin()
    args = types.SimpleNamespace(save_dir=str(tmp_path / "results"), resume="runs/standin.pth")
    res = A.evaluate(model, train, test, torch.device("cpu"), args)
    assert not A.last_native
    out = capsys.readouterr().out
    assert "FPR95:" in out and "AUROC:" in out and "AUPR:" in out
    z = np.load(os.path.join(args.save_dir, "standin.npz"))
    assert sorted(z.files) == sorted(["auroc", "aupr", "fpr", "tpr", "prec", "recall", "roc_fpr"])
    assert z["fpr"].shape == () and z["auroc"].shape == () and z["roc_fpr"].shape == z["tpr"].shape
    assert z["prec"].shape == z["recall"].shape
    # the same embeddings through the float64 restatement
    with torch.no_grad():
        tr = torch.cat([model(x) for x, _ in train]).numpy()
        te = torch.cat([model(x) for x, _ in test]).numpy()
    ref = R.chain(tr, np.concatenate([y for _, y in train]), te, np.concatenate([y for _, y in test]))
    for key in ("auroc", "aupr", "fpr"):
        assert abs(float(z[key]) - ref[key]) <= TOL, key
    assert np.abs(res["dists"] - ref["dists"]).max() <= 1e-14
    f, t, _ = R.roc_curve(ref["thresholds"], ref["tps"], ref["fps"])
    assert np.array_equal(z["roc_fpr"], f) and np.array_equal(z["tpr"], t)
    p, r, _ = R.precision_recall_curve(ref["thresholds"], ref["tps"], ref["fps"])
    assert np.array_equal(z["prec"], p) and np.array_equal(z["recall"], r)
    # without save_dir nothing is written
    A.evaluate(model, train, test, torch.device("cpu"), types.SimpleNamespace(save_dir=None, resume=""))
