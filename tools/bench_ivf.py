#!/usr/bin/env python3
"""IVF_FLAT against the flat index on one resident gallery (development tool; not the contract bench).

The gallery is clustered -- unit rows around `--centres` random unit centres -- because IVF recall on uniform random rows
says nothing.  For every query count and nprobe the two arms alternate in one process after a warm-up of each; a call is timed
with the host clock around a device synchronise; medians with the range of the repeats are reported, with recall@k of the IVF
ids against the flat index's exact ids, and the train and add times of the IVF index.

--index-type IVF_SQ8 adds an IvfSq8Index with the IVF_FLAT index's centroids and a range trained on the same strided
sample as a third alternating arm, its recall against the exact ids and against IVF_FLAT's at equal nprobe, and for both index
types the device memory held after the build and the peak during add (torch.cuda.mem_get_info, polled from a thread).

--index-type IVF_PQ --m M[,M2] keeps the IVF_SQ8 arm and adds one IvfPqIndex per m on the same centroids, its
codebooks trained on at most 65 536 strided rows: further alternating arms, with the codebook-training and add times, the memory
figures, and recall against the exact ids and against IVF_FLAT's at equal nprobe.

--by-residual adds, beside every raw PQ arm, an IvfResidualPqIndex of the same m on the same centroids in the same
process (its codebooks trained on the residuals of the same strided rows): arm "rpq<m>" next to "pq<m>", the same figures."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mirx.index import IVF_TRAIN_ROWS_PER_LIST, FlatIndex, ivf_index_spec, strided_sample  # noqa: E402


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


def free_bytes(settle=False):
    """free device memory; settle: after a synchronise and with torch's cached blocks returned, so that a difference of two
    readings is what libmirx holds (masters and scratch), not what torch keeps for reuse"""
    if settle:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def peak_during(fn):
    """(ms, the most device memory in use during fn() above what was in use before it, polled every 0.2 ms)"""
    torch.cuda.synchronize()
    start, low, done = free_bytes(True), [free_bytes()], threading.Event()

    def poll():
        while not done.is_set():
            low[0] = min(low[0], free_bytes())
            time.sleep(2e-4)

    th = threading.Thread(target=poll)
    th.start()
    try:
        ms = timed(fn)[0]
    finally:
        done.set()
        th.join()
    return ms, start - min(low[0], free_bytes())


def recall(ids, want):
    return (ids[:, :, None] == want[:, None, :]).any(dim=2).float().mean().item()


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
    ap.add_argument("--index-type", default="IVF_FLAT", choices=["IVF_FLAT", "IVF_SQ8", "IVF_PQ"])
    ap.add_argument("--m", default="", help="IVF_PQ: the sub-quantiser counts, one arm each (e.g. 64,32)")
    ap.add_argument("--codebook-iters", type=int, default=10)
    ap.add_argument("--by-residual", action="store_true", help="IVF_PQ: a residual-coded arm rpq<m> beside every raw arm pq<m>")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = clustered(a.n, a.d, a.centres, a.spread, dev, 1234)

    def build(index_type, **params):                                                  # an index of the family from the one table
        cls, kwargs = ivf_index_spec(a.d, index_type, dict(params, nlist=a.nlist))
        return cls(a.d, "COSINE", device=0, **kwargs)

    flat = FlatIndex(a.d, "COSINE", 0)
    flat.reserve(a.n)
    t_flat_add, _ = timed(lambda: flat.add(rows))
    ivf = build("IVF_FLAT")
    held0 = free_bytes(True)
    t_train, _ = timed(lambda: ivf.train(rows, iters=a.train_iters))
    t_add, peak_add = peak_during(lambda: ivf.add(rows))
    held = held0 - free_bytes(True)
    sizes = ivf.list_sizes()
    out = {"rows": a.n, "dim": a.d, "nlist": a.nlist, "centres": a.centres, "spread": a.spread, "k": a.k,
           "train_ms": t_train, "train_rows": min(a.n, 256 * a.nlist), "train_iters": a.train_iters, "ivf_add_ms": t_add,
           "flat_add_ms": t_flat_add, "list_sizes": {"min": int(sizes.min()), "median": float(statistics.median(sizes.tolist())),
                                                      "max": int(sizes.max()), "empty": int((sizes == 0).sum())},
           "index_type": a.index_type, "ivf_held_bytes": held, "ivf_add_peak_bytes": peak_add, "cases": []}
    if a.index_type == "IVF_PQ" and not a.m:
        ap.error("--index-type IVF_PQ needs --m")
    sq8, pqs = None, {}
    if a.index_type in ("IVF_SQ8", "IVF_PQ"):                                          # the same centroids, the range from train()'s sample
        held0 = free_bytes(True)
        sq8 = build("IVF_SQ8")
        sq8.set_centroids(ivf.centroids)
        sample = strided_sample(rows, IVF_TRAIN_ROWS_PER_LIST * a.nlist)
        t_range, _ = timed(lambda: sq8.train_range(sample))
        del sample
        t_add8, peak_add8 = peak_during(lambda: sq8.add(rows))
        out.update({"sq8_train_range_ms": t_range, "sq8_add_ms": t_add8, "sq8_held_bytes": held0 - free_bytes(True),
                    "sq8_add_peak_bytes": peak_add8, "rows_bytes_fp32": a.n * a.d * 4})
    arms = [(f"pq{int(v)}", int(v), False) for v in a.m.split(",") if v] if a.index_type == "IVF_PQ" else []
    if a.by_residual:
        arms = [arm for name, m, _ in arms for arm in ((name, m, False), (f"r{name}", m, True))]
    for name, m, residual in arms:
        held0 = free_bytes(True)
        pq = build("IVF_PQ", m=m, by_residual=residual)
        pq.set_centroids(ivf.centroids)
        t_cb, _ = timed(lambda: pq.train_codebooks(rows, a.codebook_iters))
        t_addp, peak_addp = peak_during(lambda: pq.add(rows))
        out[name] = {"m": m, "by_residual": residual, "train_codebooks_ms": t_cb, "codebook_rows": min(a.n, 65536),
                     "codebook_iters": a.codebook_iters, "add_ms": t_addp, "held_bytes": held0 - free_bytes(True),
                     "add_peak_bytes": peak_addp, "code_bytes": a.n * m}
        pqs[name] = pq
    print({k: v for k, v in out.items() if k != "cases"}, flush=True)
    g = torch.Generator(device=dev).manual_seed(4321)
    for nq in [int(v) for v in a.queries.split(",")]:
        pick = torch.randint(0, a.n, (nq,), generator=g, device=dev)
        q = torch.nn.functional.normalize(rows[pick] + 0.3 / a.d ** 0.5 * torch.randn(nq, a.d, generator=g, device=dev), dim=1)
        exact = flat.search(q, a.k)[1]
        for nprobe in [int(v) for v in a.nprobe.split(",")]:
            ids = ivf.search(q, a.k, nprobe)[1]                              # warm-up of this shape (flat: above)
            st = ivf.last_stats()
            hit = recall(ids, exact)
            ids8 = None if sq8 is None else sq8.search(q, a.k, nprobe)[1]   # warm-up of the third arm
            idsp, stp = {}, {}
            for name, pq in pqs.items():                                     # warm-up of the PQ arms
                idsp[name] = pq.search(q, a.k, nprobe)[1]
                stp[name] = pq.last_stats()
            reps = a.heavy_repeats if st["rows_scored"] > 1 << 33 else a.repeats
            t_ivf, t_flat, t_sq8, t_pq = [], [], [], {name: [] for name in pqs}
            for _ in range(reps):                                            # alternating arms
                t_ivf.append(timed(lambda: ivf.search(q, a.k, nprobe))[0])
                if sq8 is not None:
                    t_sq8.append(timed(lambda: sq8.search(q, a.k, nprobe))[0])
                for name, pq in pqs.items():
                    t_pq[name].append(timed(lambda: pq.search(q, a.k, nprobe))[0])
                t_flat.append(timed(lambda: flat.search(q, a.k))[0])
            case = {"queries": nq, "nprobe": nprobe, "recall_at_k": hit, "ivf": stat(t_ivf), "flat": stat(t_flat),
                    "rows_scored_per_query": st["rows_scored"] / nq, "work_items": st["work_items"], "batches": st["batches"]}
            if sq8 is not None:
                case.update({"sq8": stat(t_sq8), "sq8_recall_at_k": recall(ids8, exact), "sq8_recall_vs_ivf_flat": recall(ids8, ids)})
            for name in pqs:
                case[name] = dict(stat(t_pq[name]), recall_at_k=recall(idsp[name], exact), recall_vs_ivf_flat=recall(idsp[name], ids),
                                  work_items=stp[name]["work_items"], batches=stp[name]["batches"])
            out["cases"].append(case)
            print(case, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
