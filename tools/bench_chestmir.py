"""ChestMIR two-stage evaluation on one GPU: mirx.chestmir.evaluate_dataset on seeded COVID-shape (N = 299, 5 lesions) and
VinDr-shape (N = 3000, 16 lesions) datasets (D = 64, Dr = 32, 0-4 regions per image, topk 50, weight 0.5), natively and on the
numpy formulas (the package's own fallback path, which is the reference's algorithm: forced by hiding the GPU from the gate)
in the same process.  The native call is split into the event-to-event time around the base ranking (FlatIndex.rank_all), the
re-rank launch (all stages), the metric launches (upper bounds on kernel time: host gaps between launches fall inside), and the rest (upload, plans, majority vote and reports on the host).

    python tools/bench_chestmir.py [--steps 5] [--warmup 2] [--numpy-steps 1] [--shapes covid,vindr] [--out profiles/<name>.json]

Wall-clock medians over `steps` calls after `warmup` calls (the call ends with host work, so it is timed on the host with the
device synchronised); those parts from CUDA events inside the call; one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"covid": (299, "DEFAULT_COVID_LESIONS", 3), "vindr": (3000, "DEFAULT_VINDR_LESIONS", 6)}


def dataset(C, n, lesions, classes, seed, d=64, dr=32, max_regions=4):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, classes, size=n)
    gv = rng.standard_normal((classes, d))[cls] + 1.5 * rng.standard_normal((n, d))
    centre = {C.canonical_lesion_name(x): rng.standard_normal(dr) for x in lesions}
    maps = []
    for _ in range(n):
        m = {}
        for _ in range(int(rng.integers(0, max_regions + 1))):
            name = C.canonical_lesion_name(lesions[int(rng.integers(0, len(lesions)))])
            v = (centre[name] + rng.standard_normal(dr)).astype(np.float32)
            m.setdefault(name, []).append(v / np.linalg.norm(v))
        maps.append(m)
    return C.EvalDataset(image_names=[f"{i}.png" for i in range(n)], labels=np.asarray([f"c{c}" for c in cls], dtype=object),
                         global_vectors=C.normalize_rows(gv.astype(np.float32)), lesion_vectors=maps)


def _wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-steps", type=int, default=1)
    ap.add_argument("--shapes", default="covid,vindr")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx import chestmir as C

    rows = []
    for shape in a.shapes.split(","):
        n, attr, classes = SHAPES[shape]
        lesions = list(getattr(C, attr))
        ds = dataset(C, n, lesions, classes, seed=n)
        parts = []

        def native():
            C.evaluate_dataset(ds, lesions)
            parts.append(dict(C.evaluate_dataset.last_timings))

        wall = _wall(native, a.steps, a.warmup)
        assert C.evaluate_dataset.last_native
        parts = parts[-a.steps:]
        med = lambda k: statistics.median(p[k] for p in parts)  # noqa: E731
        gate = C._gpu
        C._gpu = lambda: False                                  # the numpy formulas of the same functions
        try:
            host = _wall(lambda: C.evaluate_dataset(ds, lesions), a.numpy_steps, 0)
            assert not C.evaluate_dataset.last_native
            sim = ds.global_vectors @ ds.global_vectors.T
            np.fill_diagonal(sim, -np.inf)
            t0 = time.perf_counter()
            C.rerank_with_adaptive_lesion(sim, ds.lesion_vectors, lesions, 50, 0.5)
            for name in lesions:
                C.rerank_with_specific_lesion(sim, ds.lesion_vectors, name, 50, 0.5)
            host_rerank = (time.perf_counter() - t0) * 1e3
        finally:
            C._gpu = gate
        native_ms = statistics.median(wall)
        row = dict(bench="chestmir", shape=shape, n=n, lesions=len(lesions), stages=len(lesions) + 1, topk=50,
                   native_ms=round(native_ms, 3), native_min_ms=round(min(wall), 3), native_max_ms=round(max(wall), 3),
                   rank_ms=round(med("rank_ms"), 3), rerank_kernel_ms=round(med("rerank_ms"), 3), metric_kernel_ms=round(med("metric_ms"), 3),
                   host_rest_ms=round(native_ms - med("rank_ms") - med("rerank_ms") - med("metric_ms"), 3),
                   numpy_ms=round(statistics.median(host), 3), numpy_rerank_loops_ms=round(host_rerank, 3),
                   speedup=round(statistics.median(host) / native_ms, 2),
                   rerank_speedup=round(host_rerank / max(med("rerank_ms"), 1e-6), 1), steps=a.steps, warmup=a.warmup,
                   numpy_steps=a.numpy_steps, device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
