"""Anomaly evaluation on one GPU: class centroids, nearest-centroid distances and the binary ranking metrics (mirx.anomaly,
k_anomaly.hip) on seeded embeddings, beside the reference's algorithm restated here and run on the host in the same process:
numpy's float32 centroid mean, float64 distances to the two centroids, the minimum, / max, a stable argsort, cumulative sums,
one point per distinct score, AUROC / AUPR / FPR at 95 % recall.

    python tools/bench_anomaly.py [--steps 5] [--warmup 3] [--shapes ref,64k,1m] [--kernels-only] [--out profiles/<name>.txt]

Shapes (train rows, test rows = scores, D): ref = 2000, 400, 1024 (the size of the reference's own run: a few hundred test
images); 64k = 65536, 65536, 1024; 1m = 2^20, 2^20, 1024 (train and test are the same 4 GiB tensor).  Native times are
CUDA-event means over three windows of at least 250 ms each (and at least `steps` calls; `calls_*` records the count) after
`warmup` calls: the figure is the median and `spread` the (max - min) / median of the three.  `gbps_distance` = N * D * 4 bytes / the distance pass's time.  The host side is timed with
perf_counter, the device-to-host copy of the embeddings (which the reference's driver also pays) apart from the arithmetic; it
runs `host_steps` times (once at the large shapes).  --kernels-only runs the native calls alone (for a
`rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"ref": (2000, 400, 1024), "64k": (65536, 65536, 1024), "1m": (1 << 20, 1 << 20, 1024)}


MIN_WINDOW_MS = 250.0


def _window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _time3(fn, min_steps, warmup):
    """Three windows of at least MIN_WINDOW_MS each (and at least min_steps calls): the call count comes from a timed trial
    window.  -> (median ms per call, (max - min) / median, calls per window)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    trial = _window(fn, min_steps) / min_steps
    steps = max(min_steps, int(MIN_WINDOW_MS / max(trial, 1e-4)) + 1)
    t = sorted(_window(fn, steps) / steps for _ in range(3))
    return round(t[1], 4), round((t[2] - t[0]) / t[1], 4), steps


def _embeddings(n, d, n_labels, seed, dev):
    """[n, d] fp32 on the device in chunks (class c shifted by 0.05 c so that the measures are not degenerate), labels cycling"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    y = torch.arange(n, device=dev) % n_labels
    for i in range(0, n, 65536):
        j = min(n, i + 65536)
        x[i:j] = torch.randn((j - i, d), generator=g, device=dev) + 0.05 * y[i:j, None].float()
    return x, y


def host_chain(train, train_labels, test, positive, level=0.95):
    """The reference's algorithm on the host, restated: test_anomaly.py:31-57 and what get_measures computes."""
    c = np.stack([train[train_labels == 0].mean(axis=0), train[train_labels == 1].mean(axis=0)]).astype(np.float64)
    dist = np.empty(test.shape[0])
    for i in range(0, test.shape[0], 16384):                      # cdist in double, in blocks that bound the host's memory
        x = test[i:i + 16384].astype(np.float64)
        dist[i:i + 16384] = np.minimum(np.sqrt(((x - c[0]) ** 2).sum(axis=1)), np.sqrt(((x - c[1]) ** 2).sum(axis=1)))
    dist /= dist.max()
    order = np.argsort(dist, kind="mergesort")[::-1]
    s, p = dist[order], positive[order]
    idx = np.r_[np.where(np.diff(s))[0], s.size - 1]
    tps = np.cumsum(p, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    P, N = tps[-1], fps[-1]
    tp0, fp0 = np.r_[0, tps[:-1]], np.r_[0, fps[:-1]]
    auroc = float(np.sum((fps - fp0) * (tps + tp0)) / (2 * P * N))
    aupr = float(np.sum((tps - tp0) / P * tps / (tps + fps)))
    last = tps.searchsorted(P)
    rec = np.r_[(tps / P)[last::-1], 1]
    fpr = float(np.r_[fps[last::-1], 0][np.argmin(np.abs(rec - level))] / N)
    return auroc, aupr, fpr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="least calls per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="ref,64k,1m")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mirx.anomaly as A
    assert torch.cuda.is_available(), "bench_anomaly needs a GPU"
    dev = torch.device("cuda:0")
    res = []
    for name in a.shapes.split(","):
        n_train, n_test, d = SHAPES[name]
        steps = a.steps
        test, test_labels = _embeddings(n_test, d, 3, 2, dev)
        train, train_labels = (test, test_labels) if name == "1m" else _embeddings(n_train, d, 2, 1, dev)
        positive = test_labels == 2
        out = {"shape": name, "train_rows": n_train, "test_rows": n_test, "d": d}

        cent = A.class_centroids(train, train_labels, (0, 1))
        dist, _, mx = A._min_dist_device(test, cent)
        pos8 = positive.to(torch.uint8).reshape(1, -1).contiguous()

        def chain():
            c = A.class_centroids(train, train_labels, (0, 1))
            dd, _, m = A._min_dist_device(test, c)
            return A.binary_metrics(dd, positive, 0.95, _norm=m)

        m = chain()
        assert A.last_native
        out["auroc"], out["aupr"], out["fpr"], out["distinct_scores"] = m["auroc"], m["aupr"], m["fpr"], int(len(m["tps"]))
        out["ms_native"], out["spread_native"], out["calls_native"] = _time3(chain, steps, a.warmup)
        out["ms_centroids"], out["spread_centroids"], out["calls_centroids"] = _time3(lambda: A.class_centroids(train, train_labels, (0, 1)), steps, a.warmup)
        out["ms_distance"], out["spread_distance"], out["calls_distance"] = _time3(lambda: A._min_dist_device(test, cent), steps, a.warmup)
        out["gbps_distance"] = round(n_test * d * 4 / (out["ms_distance"] * 1e-3) / 1e9, 1)
        out["gbps_centroids"] = round(n_train * d * 4 / (out["ms_centroids"] * 1e-3) / 1e9, 1)
        out["ms_sort_and_metrics"], out["spread_sort_and_metrics"], out["calls_sort_and_metrics"] = _time3(
            lambda: A._binary_metrics_device(dist.reshape(1, -1), pos8, 0.95, mx), steps, a.warmup)
        if not a.kernels_only:
            host_steps = 3 if n_test <= 65536 else 1
            t0 = time.perf_counter()
            tr, trl = train.cpu().numpy(), train_labels.cpu().numpy()
            te, pos = (tr, None) if name == "1m" else (test.cpu().numpy(), None)
            pos = positive.cpu().numpy()
            out["ms_host_copy"] = round((time.perf_counter() - t0) * 1e3, 2)
            t0 = time.perf_counter()
            for _ in range(host_steps):
                h = host_chain(tr, trl, te, pos)
            out["ms_host_restatement"] = round((time.perf_counter() - t0) * 1e3 / host_steps, 2)
            out["host_steps"] = host_steps
            out["host_auroc"], out["host_aupr"], out["host_fpr"] = h
            del tr, te
        print(json.dumps(out), flush=True)
        res.append(out)
        del train, test, dist, cent
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(f"# tools/bench_anomaly.py --steps {a.steps} --warmup {a.warmup} --shapes {a.shapes}"
                     f"{' --kernels-only' if a.kernels_only else ''} on {torch.cuda.get_device_name(0)}\n"
                     f"# ms per call: CUDA-event means, median of three windows of at least {MIN_WINDOW_MS:.0f} ms (calls_* calls each); "
                     "spread_* = (max - min) / median of the three; host_* = perf_counter, host_steps runs\n")
            for d_ in res:
                fh.write(json.dumps(d_) + "\n")


if __name__ == "__main__":
    main()
