"""Anomaly evaluation: nearest-class-centroid scores and AUROC / AUPR / FPR at a recall level.

Mirrors (paths into the reference tree):
  anomaly/anomaly.py        stable_cumsum, fpr_and_fdr_at_recall, get_measures, show_performance, print_measures,
                            print_measures_with_std, show_performance_comparison, recall_level_default
  anomaly/test_anomaly.py   evaluate(model, train_loader, test_loader, device, args)   (15-76)

The reference embeds a train and a test set, takes the mean embedding of the train classes 0 and 1, scores every test image by
its Euclidean distance to the nearer of the two (scipy cdist in double), divides by the largest, and reports roc_auc_score,
average_precision_score and fpr_and_fdr_at_recall(.., 0.95) plus scikit-learn's roc_curve and precision_recall_curve for
"label 2 is the anomaly".

Here one sort gives everything: the distinct scores in descending order with the positives (tps) and negatives (fps) at or above
each -- the "compact arrays" -- and the three measures and both curves are functions of those.
  * CUDA tensors: mirx_class_centroids, mirx_centroid_min_dist and mirx_binary_rank_metrics (k_anomaly.hip, the sort of
    k_ranksort.hip); embeddings stay on the device from the model to the measures.  The centroids stay fp64 (numpy's mean of an
    fp32 array rounds them to fp32).
  * anything else: the same definitions in numpy (no scikit-learn import).
`last_native` tells which path ran last.

Two defects of the reference's driver are NOT reproduced:
  * test_anomaly.py:56 rebinds `labels` to the 0/1 vector, so line 64's get_measures(dists[labels == 2], dists[labels != 2])
    receives no positives at all and returns (nan, 0.0, 1 / n).  evaluate() here measures the split lines 51-57 build, the one
    the curves come from.
  * the .npz saves fpr=fpr after line 64 has rebound `fpr` to the scalar.  The field names are kept -- auroc, aupr, fpr (the
    scalar FPR at 95 % recall, as bound at save time), tpr, prec, recall -- and roc_fpr holds the ROC curve's x axis.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

recall_level_default = 0.95
last_native = False

MAX_N = 1 << 30                # include/mirx.h MIRX_ANOMALY_MAX_*
MAX_SEGMENTS = 65535
MAX_K = 64
MAX_D = 16384

_FLAG_TEXT = ((_lib.ANOMALY_BAD_SCORE, "a NaN or infinite score"),
              (_lib.ANOMALY_BAD_NORM, "the largest distance is 0 (or not finite): nothing to normalise by"),
              (_lib.ANOMALY_BAD_ONE_CLASS, "a segment without positives or without negatives"),
              (_lib.ANOMALY_BAD_EMPTY_CLASS, "a class without rows"))


_BINARY_CODINGS = tuple(frozenset(c) for c in ((0, 1), (-1, 1), (0,), (-1,), (1,)))


def _raise_flags(flags, what):
    if flags:
        raise ValueError(f"{what}: " + "; ".join(t for b, t in _FLAG_TEXT if flags & b))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the reference's anomaly.py --------------------------------------------------------------------------------------
def stable_cumsum(arr, rtol=1e-05, atol=1e-08):
    """Running sum of `arr` (flattened) accumulated in float64.  The last entry is compared with the total that numpy's
    pairwise summation gives; a disagreement beyond rtol / atol means the running sum has drifted -> RuntimeError."""
    flat = np.asarray(arr).reshape(-1)
    running = np.add.accumulate(flat, dtype=np.float64)
    if running.size:
        total = float(np.add.reduce(flat, dtype=np.float64))
        if abs(float(running[-1]) - total) > atol + rtol * abs(total):
            raise RuntimeError(f"stable_cumsum: the running sum ends at {running[-1]!r} but the total is {total!r}")
    return running


def _compact_numpy(scores, positive):
    """Distinct scores descending with tps / fps at or above each (float64, int64, int64).  A stable sort of -scores: any
    order inside a group of equal scores gives the same arrays."""
    order = np.argsort(-scores, kind="stable")
    s = scores[order]
    p = positive[order].astype(np.int64)
    ends = np.r_[np.nonzero(s[1:] != s[:-1])[0], s.size - 1]
    tps = np.cumsum(p)[ends]
    return s[ends] + 0.0, tps, ends + 1 - tps


def _fpr_from_compact(tps, fps, recall_level):
    """FPR at the record whose recall is nearest to recall_level, by the rule of the reference's anomaly.py:59-67 read on the
    compact arrays: only records up to the first one that holds every positive take part, and of two equally near records
    the LATER one wins (the reference scans them backwards and keeps the first minimum; the (recall 1, fps 0) point it appends
    ties with that last record and comes after it, so it never wins)."""
    positives = tps[-1]
    full = int(np.searchsorted(tps, positives))
    gap = np.abs(tps[:full + 1] / positives - recall_level)
    pick = full - int(np.argmin(gap[::-1]))
    return float(fps[pick] / fps[-1])


def _measures_from_compact(tps, fps, recall_level):
    """(auroc, aupr, fpr) of one segment from its compact arrays: the definitions of mirx_binary_rank_metrics."""
    P, N = int(tps[-1]), int(fps[-1])
    tp0, fp0 = np.r_[0, tps[:-1]], np.r_[0, fps[:-1]]
    area = int(np.sum((fps - fp0) * (tps + tp0)))               # int64: exact, below 2^63 for n <= 2^30
    auroc = area / (2.0 * P * N)
    aupr = float(np.sum(((tps - tp0) / float(P)) * (tps / (tps + fps).astype(np.float64))))
    return auroc, aupr, _fpr_from_compact(tps, fps, recall_level)


def fpr_and_fdr_at_recall(y_true, y_score, recall_level=recall_level_default, pos_label=None):
    """FPR at the threshold whose recall is nearest to recall_level (the reference's anomaly.py:27-67, its tie rule included)."""
    y_true = np.asarray(y_true)
    y_score = np.asarray(y_score, dtype=np.float64).ravel()
    if pos_label is None:
        # without a pos_label the labels must be a 0/1 or -1/1 coding (or one value of those); 1 is then the positive
        present = frozenset(np.unique(y_true).tolist())
        if present not in _BINARY_CODINGS:
            raise ValueError(f"fpr_and_fdr_at_recall: y_true is not binary (values {sorted(present)}) and no pos_label is given")
        pos_label = 1
    positive = (y_true == pos_label).ravel()
    _, tps, fps = _compact_numpy(y_score, positive)
    return _fpr_from_compact(tps, fps, recall_level)


def get_measures(_pos, _neg, recall_level=recall_level_default):
    """anomaly.py:70-81 -> (auroc, aupr, fpr); positives first, as the reference stacks them."""
    dev = _pos.device if torch.is_tensor(_pos) and _pos.is_cuda else None
    if dev is not None and torch.is_tensor(_neg) and _neg.is_cuda:
        pos, neg = _pos.reshape(-1).double(), _neg.reshape(-1).double()
        if pos.numel() == 0 or neg.numel() == 0:
            raise ValueError("get_measures: pos and neg must both be non-empty")
        examples = torch.cat((pos, neg))
        labels = torch.zeros(examples.numel(), dtype=torch.uint8, device=dev)
        labels[:pos.numel()] = 1
    else:
        pos = np.asarray(_pos.cpu() if torch.is_tensor(_pos) else _pos, dtype=np.float64).reshape(-1)
        neg = np.asarray(_neg.cpu() if torch.is_tensor(_neg) else _neg, dtype=np.float64).reshape(-1)
        if pos.size == 0 or neg.size == 0:
            raise ValueError("get_measures: pos and neg must both be non-empty")
        examples = np.concatenate((pos, neg))
        labels = np.zeros(examples.size, dtype=bool)
        labels[:pos.size] = True
    m = binary_metrics(examples, labels, recall_level)
    return m["auroc"], m["aupr"], m["fpr"]


def _print_report(indent, heading, recall_level, cells, padded=False):
    """The report block every printer of the reference's anomaly.py writes: a tab-indented heading, then the FPR<level>, AUROC
    and AUPR lines, each label followed by three tabs and its cell.  `cells` = the three preformatted cells in that order;
    `padded`: AUROC / AUPR labels padded to seven characters, as print_measures and print_measures_with_std have them."""
    labels = ["FPR%d:" % int(100 * recall_level), "AUROC:", "AUPR:"]
    if padded:
        labels[1:] = [name.ljust(7) for name in labels[1:]]
    print("\t" * indent + heading)
    for name, cell in zip(labels, cells):
        print(name + "\t\t\t" + cell)


def _pct(*values):
    """percent cells with two decimals, tab-separated the way each printer separates them"""
    return ["%.2f" % (100 * v) for v in values]


def show_performance(pos, neg, method_name='Ours', recall_level=recall_level_default):
    """Measures of positive scores `pos` (the class to detect) against negative scores `neg`, printed."""
    auroc, aupr, fpr = get_measures(pos[:], neg[:], recall_level)
    _print_report(3, method_name, recall_level, [_pct(v)[0] for v in (fpr, auroc, aupr)])


def print_measures(auroc, aupr, fpr, method_name='Ours', recall_level=recall_level_default):
    _print_report(4, method_name, recall_level, [_pct(v)[0] for v in (fpr, auroc, aupr)], padded=True)


def print_measures_with_std(aurocs, auprs, fprs, method_name='Ours', recall_level=recall_level_default):
    """Mean and population standard deviation over runs."""
    _print_report(4, method_name, recall_level,
                  ["\t+/- ".join(_pct(np.mean(v), np.std(v))) for v in (fprs, aurocs, auprs)], padded=True)


def show_performance_comparison(pos_base, neg_base, pos_ours, neg_ours, baseline_name='Baseline',
                                method_name='Ours', recall_level=recall_level_default):
    """Two detectors side by side: the baseline's positive / negative scores, then ours."""
    base = get_measures(pos_base[:], neg_base[:], recall_level)
    ours = get_measures(pos_ours[:], neg_ours[:], recall_level)
    _print_report(3, baseline_name + "\t" + method_name, recall_level,
                  ["\t\t".join(_pct(base[i], ours[i])) for i in (2, 0, 1)])


# ---- centroids and scores --------------------------------------------------------------------------------------------
def _check_rows(name, rows, k):
    if rows.ndim != 2 or not 1 <= rows.shape[0] <= MAX_N or not 1 <= rows.shape[1] <= MAX_D:
        raise ValueError(f"{name}: rows must be [1 <= N <= 2^30, 1 <= D <= {MAX_D}] (got {tuple(rows.shape)})")
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{name}: needs 1 <= K <= {MAX_K} classes (got {k})")


def class_centroids(embeds, labels, classes=(0, 1), return_counts=False):
    """Mean embedding of every class in `classes` -> [K, D] float64 (rows whose label is in no class are left out).
    CUDA fp32 embeds: [HIP] mirx_class_centroids, a CUDA result; otherwise numpy float64 sums.  ValueError for an empty class."""
    global last_native
    classes = [int(c) for c in classes]
    k = len(classes)
    if torch.is_tensor(embeds) and embeds.is_cuda:
        _check_rows("class_centroids", embeds, k)
        rows = embeds.detach().float().contiguous()
        n, d = rows.shape
        lab = torch.as_tensor(labels).to(rows.device, torch.int64).reshape(-1).contiguous()
        if lab.numel() != n:
            raise ValueError(f"class_centroids: {n} rows but {lab.numel()} labels")
        lib = _lib.load()
        nws = lib.mirx_class_centroids_workspace_bytes(n, d, k)
        if nws < 0:
            _lib.check(int(nws), "mirx_class_centroids_workspace_bytes")
        with torch.cuda.device(rows.device):
            ws = torch.empty((nws,), dtype=torch.uint8, device=rows.device)
            cent = torch.empty((k, d), dtype=torch.float64, device=rows.device)
            counts = torch.empty((k,), dtype=torch.int64, device=rows.device)
            bad = torch.zeros((1,), dtype=torch.int32, device=rows.device)
            cl = (ctypes.c_int64 * k)(*classes)
            _lib.check(lib.mirx_class_centroids(_ptr(rows), n, d, _ptr(lab), ctypes.cast(cl, ctypes.c_void_p), k, _ptr(ws), nws,
                                                _ptr(cent), _ptr(counts), _ptr(bad), _stream(rows.device)), "mirx_class_centroids")
        _raise_flags(int(bad.item()), "class_centroids")
        last_native = True
        return (cent, counts) if return_counts else cent
    rows = np.asarray(embeds.detach().cpu() if torch.is_tensor(embeds) else embeds)
    _check_rows("class_centroids", rows, k)
    lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1)
    if lab.size != rows.shape[0]:
        raise ValueError(f"class_centroids: {rows.shape[0]} rows but {lab.size} labels")
    cent = np.empty((k, rows.shape[1]), dtype=np.float64)
    counts = np.zeros(k, dtype=np.int64)
    taken = np.zeros(lab.size, dtype=bool)
    for j, c in enumerate(classes):
        m = (lab == c) & ~taken                     # a repeated class value: the first takes the rows
        taken |= m
        counts[j] = int(m.sum())
        if counts[j] == 0:
            raise ValueError("class_centroids: a class without rows")
        cent[j] = rows[m].astype(np.float64).sum(axis=0) / counts[j]
    last_native = False
    return (cent, counts) if return_counts else cent


def _min_dist_device(rows, cent):
    """[HIP] mirx_centroid_min_dist -> (dist fp64 [N], nearest int32 [N], max fp64 [1]), not normalised."""
    n, d = rows.shape
    k = cent.shape[0]
    lib = _lib.load()
    with torch.cuda.device(rows.device):
        dist = torch.empty((n,), dtype=torch.float64, device=rows.device)
        nearest = torch.empty((n,), dtype=torch.int32, device=rows.device)
        mx = torch.empty((1,), dtype=torch.float64, device=rows.device)
        _lib.check(lib.mirx_centroid_min_dist(_ptr(rows), n, d, _ptr(cent), k, _ptr(dist), _ptr(nearest), _ptr(mx),
                                              _stream(rows.device)), "mirx_centroid_min_dist")
    return dist, nearest, mx


def _prep_scores_args(test_embeds, centroids):
    rows = test_embeds.detach().float().contiguous()
    cent = torch.as_tensor(centroids).to(rows.device, torch.float64).contiguous()
    if cent.dim() != 2 or cent.shape[1] != rows.shape[1]:
        raise ValueError(f"centroid_scores: centroids must be [K, {rows.shape[1]}] (got {tuple(cent.shape)})")
    _check_rows("centroid_scores", rows, cent.shape[0])
    return rows, cent


def centroid_scores(test_embeds, centroids):
    """Distance of every row to its nearest centroid (the lowest class on a tie), divided by the largest distance ->
    (dists float64 [N], nearest [N]).  test_anomaly.py:46-48.  ValueError when the largest distance is 0 or not finite."""
    global last_native
    if torch.is_tensor(test_embeds) and test_embeds.is_cuda:
        rows, cent = _prep_scores_args(test_embeds, centroids)
        dist, nearest, mx = _min_dist_device(rows, cent)
        m = float(mx.item())
        if not (0.0 < m < float("inf")):
            _raise_flags(_lib.ANOMALY_BAD_NORM if m == 0.0 else _lib.ANOMALY_BAD_SCORE, "centroid_scores")
        last_native = True
        return dist / mx, nearest
    rows = np.asarray(test_embeds.detach().cpu() if torch.is_tensor(test_embeds) else test_embeds).astype(np.float64)
    cent = np.asarray(centroids.cpu() if torch.is_tensor(centroids) else centroids, dtype=np.float64)
    if cent.ndim != 2 or rows.ndim != 2 or cent.shape[1] != rows.shape[1]:
        raise ValueError(f"centroid_scores: centroids must be [K, D] for rows [N, D] (got {cent.shape}, {rows.shape})")
    _check_rows("centroid_scores", rows, cent.shape[0])
    d = np.stack([np.sqrt(((rows - c) ** 2).sum(axis=1)) for c in cent], axis=1)
    nearest = d.argmin(axis=1).astype(np.int32)
    d = d.min(axis=1)
    m = d.max()
    if not (0.0 < m < np.inf):
        _raise_flags(_lib.ANOMALY_BAD_NORM if m == 0.0 else _lib.ANOMALY_BAD_SCORE, "centroid_scores")
    last_native = False
    return d / m, nearest


# ---- binary ranking metrics ------------------------------------------------------------------------------------------
def _binary_metrics_device(scores, positive, recall_level, norm=None):
    """[HIP] mirx_binary_rank_metrics on scores [S, n] fp64 / positive [S, n] uint8 (CUDA) -> per-segment results."""
    s, n = scores.shape
    if not (1 <= n <= MAX_N and 1 <= s <= MAX_SEGMENTS):
        raise ValueError(f"binary_metrics: needs 1 <= n <= 2^30 and 1 <= S <= {MAX_SEGMENTS} (got S = {s}, n = {n})")
    lib = _lib.load()
    dev = scores.device
    nws = lib.mirx_binary_rank_metrics_workspace_bytes(s, n)
    if nws < 0:
        _lib.check(int(nws), "mirx_binary_rank_metrics_workspace_bytes")
    with torch.cuda.device(dev):
        ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
        thr = torch.empty((s, n), dtype=torch.float64, device=dev)
        tps = torch.empty((s, n), dtype=torch.int64, device=dev)
        fps = torch.empty((s, n), dtype=torch.int64, device=dev)
        cnt = torch.empty((s,), dtype=torch.int64, device=dev)
        out = torch.empty((3, s), dtype=torch.float64, device=dev)
        bad = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.check(lib.mirx_binary_rank_metrics(_ptr(scores), _ptr(positive), s, n, _ptr(norm) if norm is not None else None,
                                                float(recall_level), _ptr(ws), nws, _ptr(thr), _ptr(tps), _ptr(fps), _ptr(cnt),
                                                _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(bad), _stream(dev)),
                   "mirx_binary_rank_metrics")
    _raise_flags(int(bad.item()), "binary_metrics")
    return thr, tps, fps, cnt.cpu().tolist(), out.cpu().numpy()


def binary_metrics(scores, positive, recall_level=recall_level_default, _norm=None):
    """AUROC, AUPR, FPR at `recall_level` and the compact arrays of scores [n] (or [S, n]: S independent segments) with
    positive [n] / [S, n] (non-zero = positive).  -> {"auroc", "aupr", "fpr": floats, "thresholds", "tps", "fps": numpy arrays
    of the T distinct scores, descending}; for [S, n] every entry is a list of S.  CUDA scores take the native path.
    ValueError: a NaN or infinite score, a segment without positives or without negatives."""
    global last_native
    if not 0.0 <= float(recall_level) <= 1.0:
        raise ValueError("binary_metrics: recall_level must be in [0, 1]")
    if torch.is_tensor(scores) and scores.is_cuda:
        sc = scores.detach().double()
        single = sc.dim() == 1
        sc = sc.reshape(1, -1) if single else sc
        if sc.dim() != 2:
            raise ValueError("binary_metrics: scores must be [n] or [S, n]")
        sc = sc.contiguous()
        pos = (torch.as_tensor(positive).to(sc.device) != 0).to(torch.uint8).reshape(sc.shape).contiguous()
        thr, tps, fps, cnt, out = _binary_metrics_device(sc, pos, recall_level, _norm)
        # only the T records of each segment cross to the host, not the [S, n] buffers
        res = {"auroc": [float(v) for v in out[0]], "aupr": [float(v) for v in out[1]], "fpr": [float(v) for v in out[2]],
               "thresholds": [thr[i, :t].cpu().numpy() for i, t in enumerate(cnt)],
               "tps": [tps[i, :t].cpu().numpy() for i, t in enumerate(cnt)],
               "fps": [fps[i, :t].cpu().numpy() for i, t in enumerate(cnt)]}
        last_native = True
    else:
        sc = np.asarray(scores.detach().cpu() if torch.is_tensor(scores) else scores, dtype=np.float64)
        single = sc.ndim == 1
        sc = sc.reshape(1, -1) if single else sc
        if sc.ndim != 2 or sc.shape[1] < 1:
            raise ValueError("binary_metrics: scores must be [n] or [S, n], n >= 1")
        pos = (np.asarray(positive.cpu() if torch.is_tensor(positive) else positive) != 0).reshape(sc.shape)
        flags = 0
        if not np.isfinite(sc).all():
            flags |= _lib.ANOMALY_BAD_SCORE
        if any(p.all() or not p.any() for p in pos):
            flags |= _lib.ANOMALY_BAD_ONE_CLASS
        _raise_flags(flags, "binary_metrics")
        res = {k: [] for k in ("auroc", "aupr", "fpr", "thresholds", "tps", "fps")}
        for s_, p_ in zip(sc, pos):
            thr, tps, fps = _compact_numpy(s_, p_)
            a, b, c = _measures_from_compact(tps, fps, recall_level)
            for k, v in zip(res, (a, b, c, thr, tps, fps)):
                res[k].append(v)
        last_native = False
    return {k: v[0] for k, v in res.items()} if single else res


def roc_curve(thresholds, tps, fps, drop_intermediate=True):
    """scikit-learn's roc_curve from the compact arrays -> (fpr, tpr, thresholds): corners only when drop_intermediate, then
    the leading (0, 0) point with threshold inf.  O(T) numpy."""
    thresholds, tps, fps = np.asarray(thresholds, dtype=np.float64), np.asarray(tps), np.asarray(fps)
    if drop_intermediate and len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    tps, fps, thresholds = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thresholds]
    return fps / fps[-1], tps / tps[-1], thresholds


def precision_recall_curve(thresholds, tps, fps):
    """scikit-learn 1.7's precision_recall_curve from the compact arrays -> (precision, recall, thresholds): one point per
    distinct score, recall decreasing, the final (1, 0) point appended, thresholds ascending.  O(T) numpy."""
    thresholds, tps, fps = np.asarray(thresholds, dtype=np.float64), np.asarray(tps), np.asarray(fps)
    precision = tps / (tps + fps).astype(np.float64)            # tps + fps >= 1 at every record
    recall = tps / tps[-1]
    return np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0)), thresholds[::-1].copy()


# ---- the driver ------------------------------------------------------------------------------------------------------
@torch.no_grad()
def evaluate(model, train_loader, test_loader, device, args):
    """test_anomaly.py:15-76 with its signature, prints and .npz (fields: see the module docstring).  Embeddings that come
    out of the model on a CUDA device never leave it: centroids, distances, normalisation, the sort and the measures run in
    libmirx; only the T curve points and three numbers cross to the host."""
    global last_native
    from .evaluate import embed_loader
    tr_embeds, tr_labels = embed_loader(model, train_loader, device)
    te_embeds, te_labels = embed_loader(model, test_loader, device)
    positive = te_labels.reshape(-1) == 2
    if torch.is_tensor(te_embeds) and te_embeds.is_cuda:
        cent = class_centroids(tr_embeds, tr_labels, (0, 1))
        rows, cent = _prep_scores_args(te_embeds, cent)
        dist, nearest, mx = _min_dist_device(rows, cent)
        m = binary_metrics(dist, positive, recall_level_default, _norm=mx)   # ranks on dist / max, as the reference does
        dists = dist / mx
        native = True
    else:
        cent = class_centroids(tr_embeds, tr_labels, (0, 1))
        dists, nearest = centroid_scores(te_embeds, cent)
        m = binary_metrics(dists, positive.cpu().numpy(), recall_level_default)
        native = False
    last_native = native
    roc_fpr, tpr, _ = roc_curve(m["thresholds"], m["tps"], m["fps"])
    prec, recall, _ = precision_recall_curve(m["thresholds"], m["tps"], m["fps"])
    auroc, aupr, fpr = m["auroc"], m["aupr"], m["fpr"]
    print_measures(auroc, aupr, fpr)
    result = {"auroc": auroc, "aupr": aupr, "fpr": fpr, "tpr": tpr, "prec": prec, "recall": recall, "roc_fpr": roc_fpr,
              "dists": dists, "nearest": nearest, "centroids": cent, "embeds": te_embeds, "labels": te_labels,
              "train_embeds": tr_embeds, "train_labels": tr_labels}
    if getattr(args, "save_dir", None):
        os.makedirs(args.save_dir, exist_ok=True)
        file_name = args.resume.split('/')[-1].split('.')[0]
        save_path = os.path.join(args.save_dir, file_name)
        np.savez(save_path, auroc=auroc, aupr=aupr, fpr=fpr, tpr=tpr, prec=prec, recall=recall, roc_fpr=roc_fpr)
    return result
