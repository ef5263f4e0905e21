#!/usr/bin/env python3
"""IVF_FLAT against the flat index on one resident gallery (development tool; not the contract bench).

The gallery is clustered -- unit rows around `--centres` random unit centres -- because IVF recall on uniform random rows
says nothing.  For every query count and nprobe the two arms alternate in one process after a warm-up of each; a call is timed
with the host clock around a device synchronise; medians with the range of the repeats are reported, with recall@k of the IVF
ids against the flat index's exact ids, and the train and add times of the IVF index."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mirx.index import FlatIndex, IvfFlatIndex  # noqa: E402


def clustered(n, d, centres, spread, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    c = torch.nn.functional.normalize(torch.randn(centres, d, generator=g, device=dev), dim=1)
    out = torch.empty((n, d), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 17):
        m = min(1 << 17, n - s)
        which = torch.randint(0, centres, (m,), generator=g, device=dev)
        out[s:s + m] = torch.nn.functional.normalize(c[which] + spread / d ** 0.5 * torch.randn(m, d, generator=g, device=dev), dim=1)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--centres", type=int, default=512)
    ap.add_argument("--spread", type=float, default=0.5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", default="1,10,32,128,1024")
    ap.add_argument("--queries", default="1,64,4096")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--heavy-repeats", type=int, default=3, help="repeats of a call that scores more than 2^33 (query, row) pairs")
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = clustered(a.n, a.d, a.centres, a.spread, dev, 1234)
    flat = FlatIndex(a.d, "COSINE", 0)
    flat.reserve(a.n)
    t_flat_add, _ = timed(lambda: flat.add(rows))
    ivf = IvfFlatIndex(a.d, "COSINE", a.nlist, 0)
    t_train, _ = timed(lambda: ivf.train(rows, iters=a.train_iters))
    t_add, _ = timed(lambda: ivf.add(rows))
    sizes = ivf.list_sizes()
    out = {"rows": a.n, "dim": a.d, "nlist": a.nlist, "centres": a.centres, "spread": a.spread, "k": a.k,
           "train_ms": t_train, "train_rows": min(a.n, 256 * a.nlist), "train_iters": a.train_iters, "ivf_add_ms": t_add,
           "flat_add_ms": t_flat_add, "list_sizes": {"min": int(sizes.min()), "median": float(statistics.median(sizes.tolist())),
                                                      "max": int(sizes.max()), "empty": int((sizes == 0).sum())}, "cases": []}
    print({k: v for k, v in out.items() if k != "cases"}, flush=True)
    g = torch.Generator(device=dev).manual_seed(4321)
    for nq in [int(v) for v in a.queries.split(",")]:
        pick = torch.randint(0, a.n, (nq,), generator=g, device=dev)
        q = torch.nn.functional.normalize(rows[pick] + 0.3 / a.d ** 0.5 * torch.randn(nq, a.d, generator=g, device=dev), dim=1)
        exact = flat.search(q, a.k)[1]
        for nprobe in [int(v) for v in a.nprobe.split(",")]:
            ids = ivf.search(q, a.k, nprobe)[1]                              # warm-up of this shape (flat: above)
            st = ivf.last_stats()
            hit = (ids[:, :, None] == exact[:, None, :]).any(dim=2).float().mean().item()
            reps = a.heavy_repeats if st["rows_scored"] > 1 << 33 else a.repeats
            t_ivf, t_flat = [], []
            for _ in range(reps):                                            # alternating arms
                t_ivf.append(timed(lambda: ivf.search(q, a.k, nprobe))[0])
                t_flat.append(timed(lambda: flat.search(q, a.k))[0])
            case = {"queries": nq, "nprobe": nprobe, "recall_at_k": hit, "ivf": stat(t_ivf), "flat": stat(t_flat),
                    "rows_scored_per_query": st["rows_scored"] / nq, "work_items": st["work_items"], "batches": st["batches"]}
            out["cases"].append(case)
            print(case, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
