"""mirx.anomaly on the MI355X: mirx_binary_rank_metrics, mirx_class_centroids and mirx_centroid_min_dist (k_anomaly.hip)
against the float64 restatement of tests/_anomaly_ref.py, the goldens of the reference through the device, and evaluate() end to
end.  Sizes sit on either side of the lane (64) and RANK_TILE (4096) boundaries and of the kernels' path switches (16-byte /
4-byte row loads, centroids in LDS / through L2, more than four classes, class accumulators past 64 KiB of LDS)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _anomaly_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-12
TILE = 4096


def _check_segment(got, ref, what):
    for key in ("thresholds", "tps", "fps"):
        assert np.array_equal(got[key], ref[key]), (what, key)
    for key in ("auroc", "aupr", "fpr"):
        assert abs(got[key] - ref[key]) <= TOL, (what, key, got[key], ref[key])


def _score_sets(n, rng):
    """name -> (scores, positive); both classes present in every set."""
    half = rng.random(n) < 0.4
    half[0], half[-1] = True, False
    sets = {"continuous": (rng.random(n), half),
            "eight_valued": (np.round(7 * rng.random(n)) / 7, half),
            "all_equal": (np.full(n, 0.375), half)}
    # a tie group across the tile boundary of the SORTED segment (n > TILE), else across the middle: `above` scores are larger
    above = TILE - 150 if n > TILE else n // 3
    s = rng.random(n) * 0.4
    s[:above] += 0.6
    s[above:above + max(1, min(300, n - above - 1))] = 0.5
    perm = rng.permutation(n)
    sets["tie_straddles_tile"] = (s[perm], half)
    one = np.zeros(n, bool)
    one[rng.integers(n)] = True
    sets["one_positive"] = (rng.random(n), one)
    sets["one_negative"] = (np.round(15 * rng.random(n)) / 15, ~one)
    return sets


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5])
def test_metric_kernel_equals_the_restatement(n):
    import mirx.anomaly as A
    rng = np.random.default_rng(100 + n)
    for name, (sc, pos) in _score_sets(n, rng).items():
        got = A.binary_metrics(torch.from_numpy(sc).to(DEV), torch.from_numpy(pos).to(DEV))
        assert A.last_native
        _check_segment(got, R.measures(sc, pos), (n, name))


def test_three_segments_equal_three_single_calls_bit_for_bit():
    import mirx.anomaly as A
    n = 4097
    rng = np.random.default_rng(7)
    sets = _score_sets(n, rng)
    names = ["continuous", "eight_valued", "tie_straddles_tile"]
    S = torch.from_numpy(np.stack([sets[k][0] for k in names])).to(DEV)
    P = torch.from_numpy(np.stack([sets[k][1] for k in names])).to(DEV)
    m = A.binary_metrics(S, P)
    for i, name in enumerate(names):
        one = A.binary_metrics(S[i], P[i])
        for key in ("auroc", "aupr", "fpr"):
            assert np.float64(one[key]).tobytes() == np.float64(m[key][i]).tobytes(), (name, key)
        for key in ("thresholds", "tps", "fps"):
            assert one[key].tobytes() == m[key][i].tobytes(), (name, key)
        _check_segment(one, R.measures(*sets[name]), name)


def test_golden_cases_through_the_device(golden_dir):
    import mirx.anomaly as A
    with open(os.path.join(golden_dir, "anomaly_ref.json")) as fh:
        golden = json.load(fh)
    for name, c in golden["cases"].items():
        pos, neg = torch.tensor(c["pos"], dtype=torch.float64, device=DEV), torch.tensor(c["neg"], dtype=torch.float64, device=DEV)
        auroc, aupr, fpr = A.get_measures(pos, neg)
        assert A.last_native
        for got, key in ((auroc, "auroc"), (aupr, "aupr"), (fpr, "fpr")):
            assert abs(got - c[key]) <= TOL, (name, key, got, c[key])
        if "roc" in c:
            m = A.binary_metrics(torch.cat((pos, neg)), torch.arange(pos.numel() + neg.numel(), device=DEV) < pos.numel())
            f, t, thr = A.roc_curve(m["thresholds"], m["tps"], m["fps"])
            assert np.array_equal(thr[1:], np.array(c["roc"]["thresholds"]))
            assert np.abs(f - c["roc"]["fpr"]).max() <= TOL and np.abs(t - c["roc"]["tpr"]).max() <= TOL
            p, r, thr2 = A.precision_recall_curve(m["thresholds"], m["tps"], m["fps"])
            assert np.abs(p - c["pr"]["precision"]).max() <= TOL and np.abs(r - c["pr"]["recall"]).max() <= TOL
            assert np.array_equal(thr2, np.array(c["pr"]["thresholds"]))


def test_flag_cases_are_value_errors():
    """Ordinary inputs answered with ValueError; the calls complete and the next call works."""
    import mirx.anomaly as A
    t = lambda v, dt=torch.float64: torch.tensor(v, dtype=dt, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="NaN or infinite"):
        A.binary_metrics(t([0.1, float("nan"), 0.3]), t([1, 0, 0], torch.uint8))
    with pytest.raises(ValueError, match="NaN or infinite"):
        A.binary_metrics(t([0.1, float("inf"), 0.3]), t([1, 0, 0], torch.uint8))
    with pytest.raises(ValueError, match="without positives"):
        A.binary_metrics(t([0.1, 0.2, 0.3]), t([0, 0, 0], torch.uint8))
    with pytest.raises(ValueError, match="without positives"):
        A.binary_metrics(t([0.1, 0.2, 0.3]), t([1, 1, 1], torch.uint8))
    with pytest.raises(ValueError, match="largest distance is 0"):
        A.binary_metrics(t([0.0, 0.0, 0.0]), t([1, 0, 0], torch.uint8), _norm=t([0.0]))
    rows = torch.ones(4, 8, device=DEV)
    with pytest.raises(ValueError, match="largest distance is 0"):
        A.centroid_scores(rows, torch.ones(1, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="without rows"):
        A.class_centroids(rows, torch.zeros(4, dtype=torch.int64), (0, 1))
    with pytest.raises(ValueError):
        A.get_measures(t([]), t([0.1]))
    m = A.binary_metrics(t([0.9, 0.1]), t([1, 0], torch.uint8))
    assert m["auroc"] == 1.0 and m["fpr"] == 0.0


def _labelled_rows(n, d, rng):
    rows = (rng.standard_normal((n, d)) + 0.25).astype(np.float32)
    labels = rng.choice([0, 1, 2, 7], size=n, p=[0.5, 0.3, 0.15, 0.05])     # unequal classes; 7 is in no class
    labels[0] = 0
    if n >= 5:
        labels[labels == 2] = 0
        labels[[1, 2, 3, 4]] = [1, 2, 7, 0]                                  # class 2: exactly one row
    return rows, labels


def _centroid_case(rows, labels, classes):
    """Runs the device chain and checks it against the restatement; the bounds of the issue, stated here:
    each distance lies within (N_c + D + 8) * 2^-52 relative of the float64 restatement, N_c the largest class count -- the
    worst case of two fp64 sums (N_c terms for the centroid, D for the squared distance) taken in another order, plus the
    division, the subtraction, the square root and the final rounding -- and the error is no larger than e_ref, the error
    of the reference's own arithmetic (a float32 mean) on the same inputs."""
    import mirx.anomaly as A
    n, d = rows.shape
    x, y = torch.from_numpy(rows).to(DEV), torch.from_numpy(labels).to(DEV)
    cent, counts = A.class_centroids(x, y, classes, return_counts=True)
    assert A.last_native and cent.dtype == torch.float64
    again = A.class_centroids(x, y, classes)
    assert cent.cpu().numpy().tobytes() == again.cpu().numpy().tobytes(), "centroids differ between two calls"
    ref_c, ref_n = R.centroids(rows, labels, classes)
    assert np.array_equal(counts.cpu().numpy(), ref_n)
    dist, nearest, mx = A._min_dist_device(x, cent)
    dist, nearest = dist.cpu().numpy(), nearest.cpu().numpy()
    ref_d, ref_a = R.min_dist(rows, ref_c)
    assert float(mx.item()) == dist.max()
    den = np.where(ref_d > 0, ref_d, 1.0)
    err = float((np.abs(dist - ref_d) / den).max())
    own_d, _ = R.min_dist(rows, R.reference_centroids(rows, labels, classes))
    e_ref = float((np.abs(own_d - ref_d) / den).max())
    bound = (int(ref_n.max()) + d + 8) * 2.0 ** -52
    print(f"N={n} D={d} K={len(classes)}: err={err:.3e} bound={bound:.3e} e_ref={e_ref:.3e}")
    assert err <= bound, (err, bound)
    assert err <= e_ref, (err, e_ref)
    # a nearest class may differ only where the restatement's two best distances tie within the bound
    assert np.array_equal(nearest, ref_a)
    if dist.max() > 0:
        normed, near2 = A.centroid_scores(x, cent)
        assert np.array_equal(normed.cpu().numpy(), dist / dist.max()) and np.array_equal(near2.cpu().numpy(), nearest)


@pytest.mark.parametrize("d", [1, 7, 64, 1000, 1024, 2048])
@pytest.mark.parametrize("n", [1, 5, 300, 4097])
def test_centroids_and_distances(n, d):
    rng = np.random.default_rng(1000 * n + d)
    rows, labels = _labelled_rows(n, d, rng)
    for classes in ((0,), (0, 1), (0, 1, 2)):
        if n == 1 and len(classes) > 1:
            continue                                   # one row fills one class
        _centroid_case(rows, labels, classes)


def test_centroid_paths_past_the_lds_budgets():
    """K = 5 at D = 2048: more than four classes (two class groups) and 80 KiB of centroids (read through L2); K = 33: the
    chunk's class accumulators take more than 64 KiB of LDS."""
    rng = np.random.default_rng(11)
    rows = (rng.standard_normal((300, 2048)) + 0.25).astype(np.float32)
    _centroid_case(rows, np.arange(300) % 6, (0, 1, 2, 3, 4))
    rows = rng.standard_normal((300, 7)).astype(np.float32)
    _centroid_case(rows, np.arange(300) % 34, tuple(range(33)))


def test_tie_goes_to_the_lowest_class():
    import mirx.anomaly as A
    rng = np.random.default_rng(12)
    rows = torch.from_numpy(rng.standard_normal((65, 24)).astype(np.float32)).to(DEV)
    c = torch.from_numpy(rng.standard_normal(24)).to(DEV)
    far = c + 100.0
    _, nearest = A.centroid_scores(rows, torch.stack([far, c, c]))
    assert (nearest == 1).all()


def test_a_nan_centroid_is_never_skipped():
    """A NaN in any class's centroid (not only class 0's) makes every distance and the maximum NaN, at every class-group width."""
    import mirx.anomaly as A
    rng = np.random.default_rng(13)
    for d in (8, 7):                                   # 16-byte and 4-byte row loads
        rows = torch.from_numpy(rng.standard_normal((70, d)).astype(np.float32)).to(DEV)
        for k, bad in ((2, 1), (3, 2), (6, 5), (2, 0)):
            cent = torch.from_numpy(rng.standard_normal((k, d))).to(DEV)
            cent[bad, d - 1] = float("nan")
            dist, _, mx = A._min_dist_device(rows, cent)
            assert torch.isnan(dist).all() and torch.isnan(mx).all(), (d, k, bad)
            with pytest.raises(ValueError, match="NaN or infinite"):
                A.centroid_scores(rows, cent)


def _end_to_end(model, train, test, tmp_path, name):
    import mirx.anomaly as A
    args = types.SimpleNamespace(save_dir=str(tmp_path), resume=f"runs/{name}.pth")
    res = A.evaluate(model, train, test, DEV, args)
    assert A.last_native
    z = np.load(os.path.join(str(tmp_path), f"{name}.npz"))
    assert sorted(z.files) == sorted(["auroc", "aupr", "fpr", "tpr", "prec", "recall", "roc_fpr"])
    ref = R.chain(res["train_embeds"].float().cpu().numpy(), res["train_labels"].cpu().numpy(),
                  res["embeds"].float().cpu().numpy(), res["labels"].cpu().numpy())
    # the precondition: no two different normalised scores within 1e-9, so both sides see the same groups in the same order
    gaps = np.diff(np.unique(ref["dists"]))
    assert gaps.size == 0 or gaps.min() > 1e-9, gaps.min()
    assert np.abs(res["dists"].cpu().numpy() - ref["dists"]).max() <= 1e-12
    for key in ("auroc", "aupr", "fpr"):
        assert abs(float(z[key]) - ref[key]) <= TOL, (key, float(z[key]), ref[key])
    f, t, _ = R.roc_curve(ref["thresholds"], ref["tps"], ref["fps"])
    p, r, _ = R.precision_recall_curve(ref["thresholds"], ref["tps"], ref["fps"])
    assert np.array_equal(z["roc_fpr"], f) and np.array_equal(z["tpr"], t)
    assert np.array_equal(z["prec"], p) and np.array_equal(z["recall"], r)
    assert z["fpr"].shape == ()


def test_evaluate_with_the_standin_model(tmp_path):
    model, train, test = R.standin()
    _end_to_end(model.to(DEV), train, test, tmp_path, "standin")


def test_evaluate_with_densenet121(tmp_path):
    from mirx.model import DenseNet121
    from oracle import densenet as OD
    torch.manual_seed(0)
    model = DenseNet121().eval()
    model.load_state_dict(OD.randomize_bn_stats(model.state_dict(), seed=3))
    _end_to_end(model.to(DEV), R.image_loader(24, 2, 224, 21, batch=8), R.image_loader(18, 3, 224, 22, batch=6), tmp_path, "densenet")
