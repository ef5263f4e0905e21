"""Float64 restatement of the anomaly chain (mirx.anomaly, k_anomaly.hip), written from the definitions and independent of the
package: centroid sums and means in float64 with no float32 rounding, double distances, the compact arrays (one record per
distinct score, descending), AUROC / AUPR from them and the reference's FPR-at-recall cutoff rule (anomaly/anomaly.py:59-67 of
the reference).  reference_centroids restates the reference's OWN arithmetic -- numpy's float32 mean(axis=0) -- so that the
tests can state the reference's error e_ref against float64 on the same inputs."""
from fractions import Fraction

import numpy as np


def centroids(rows, labels, classes):
    """[K, D] float64: sum of the float64 images of the rows of each class / count (no float32 rounding)."""
    rows = np.asarray(rows, dtype=np.float64)
    labels = np.asarray(labels)
    out = np.empty((len(classes), rows.shape[1]))
    counts = np.zeros(len(classes), dtype=np.int64)
    for j, c in enumerate(classes):
        m = labels == c
        counts[j] = m.sum()
        out[j] = rows[m].sum(axis=0) / counts[j] if counts[j] else np.nan
    return out, counts


def reference_centroids(rows, labels, classes):
    """The reference's arithmetic (test_anomaly.py:31-32): numpy's mean of a float32 array, a float32 result."""
    rows = np.asarray(rows, dtype=np.float32)
    labels = np.asarray(labels)
    return np.stack([rows[labels == c].mean(axis=0) for c in classes])


def min_dist(rows, cent):
    """(dist float64 [N] not normalised, nearest [N]): Euclidean distance in double to the nearest centroid, lowest class on a tie."""
    rows = np.asarray(rows, dtype=np.float64)
    cent = np.asarray(cent, dtype=np.float64)
    d = np.stack([np.sqrt(((rows - c) ** 2).sum(axis=1)) for c in cent], axis=1)
    return d.min(axis=1), d.argmin(axis=1)


def compact(scores, positive):
    """Distinct scores descending, tps, fps (float64, int64, int64) -- by plain counting, no sort-order subtleties."""
    scores = np.asarray(scores, dtype=np.float64)
    positive = np.asarray(positive) != 0
    thr = np.unique(scores)[::-1]
    pos_sorted = np.sort(scores[positive])
    neg_sorted = np.sort(scores[~positive])
    tps = pos_sorted.size - np.searchsorted(pos_sorted, thr, side="left")
    fps = neg_sorted.size - np.searchsorted(neg_sorted, thr, side="left")
    return thr + 0.0, tps.astype(np.int64), fps.astype(np.int64)


def auroc(tps, fps):
    """Trapezoid area under (fps, tps) from (0, 0), exact in rationals, rounded once."""
    P, N = int(tps[-1]), int(fps[-1])
    area, tp0, fp0 = 0, 0, 0
    for tp, fp in zip(tps.tolist(), fps.tolist()):
        area += (fp - fp0) * (tp + tp0)
        tp0, fp0 = tp, fp
    return float(Fraction(area, 2 * P * N))


def aupr(tps, fps):
    """Step integral sum_t (recall_t - recall_{t-1}) * precision_t, float64, in threshold order."""
    P = float(tps[-1])
    tp0 = np.r_[0, tps[:-1]]
    return float(np.sum(((tps - tp0) / P) * (tps / (tps + fps).astype(np.float64))))


def fpr_at_recall(tps, fps, level):
    """The reference's cutoff: records 0 .. last_ind (the first with tps == P), reversed, (recall 1, fps 0) appended; the
    first minimum of |recall - level| in that order."""
    P = tps[-1]
    last = int(np.nonzero(tps == P)[0][0])
    cand = [(abs(float(tps[i]) / float(P) - level), int(fps[i])) for i in range(last, -1, -1)] + [(abs(1.0 - level), 0)]
    best = min(range(len(cand)), key=lambda i: (cand[i][0], i))
    return cand[best][1] / float(fps[-1])


def measures(scores, positive, level=0.95):
    thr, tps, fps = compact(scores, positive)
    return {"thresholds": thr, "tps": tps, "fps": fps, "auroc": auroc(tps, fps), "aupr": aupr(tps, fps),
            "fpr": fpr_at_recall(tps, fps, level)}


def roc_curve(thr, tps, fps):
    """scikit-learn's roc_curve (drop_intermediate=True) from the compact arrays."""
    if len(fps) > 2:
        keep = [0] + [i for i in range(1, len(fps) - 1)
                      if (fps[i + 1] - 2 * fps[i] + fps[i - 1]) != 0 or (tps[i + 1] - 2 * tps[i] + tps[i - 1]) != 0] + [len(fps) - 1]
        thr, tps, fps = thr[keep], tps[keep], fps[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    return fps / fps[-1], tps / tps[-1], np.r_[np.inf, thr]


def precision_recall_curve(thr, tps, fps):
    """scikit-learn 1.7's precision_recall_curve from the compact arrays."""
    prec = tps / (tps + fps).astype(np.float64)
    rec = tps / tps[-1]
    return np.r_[prec[::-1], 1.0], np.r_[rec[::-1], 0.0], thr[::-1].copy()


def chain(train, train_labels, test, test_labels, classes=(0, 1), anomaly=2, level=0.95):
    """The whole driver in float64 from given embeddings."""
    cent, _ = centroids(train, train_labels, classes)
    d, nearest = min_dist(test, cent)
    d = d / d.max()
    m = measures(d, np.asarray(test_labels) == anomaly, level)
    m.update(dists=d, nearest=nearest, centroids=cent)
    return m


# ---- the stand-in model and loaders of the driver tests ----------------------------------------------------------------
def standin(n_train=24, n_test=18, dim=16, seed=5):
    """(model, train_loader, test_loader): a fixed seeded Linear on flattened 3 x 8 x 8 inputs, list-of-batches loaders; train
    labels cycle 0 / 1, test labels 0 / 1 / 2."""
    import torch

    class Flat(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.fc = torch.nn.Linear(192, dim)
            with torch.no_grad():
                self.fc.weight.copy_(torch.randn(dim, 192, generator=g) * 0.1)
                self.fc.bias.copy_(torch.randn(dim, generator=g) * 0.1)

        def forward(self, x):
            return self.fc(x.flatten(1))

    return Flat().eval(), image_loader(n_train, 2, 8, seed + 1), image_loader(n_test, 3, 8, seed + 2)


def image_loader(n, n_labels, side, seed, batch=7):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, side, side, generator=g)
    y = torch.arange(n) % n_labels
    x = x + y.float().reshape(-1, 1, 1, 1) * 0.5                 # the classes differ, so the measures are not degenerate
    return [(x[i:i + batch], y[i:i + batch]) for i in range(0, n, batch)]
