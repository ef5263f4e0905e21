"""The deep search route beside the exact tier it replaces, on one GPU, same index, same process.

    python tools/bench_search_deep.py [--rows 1048576] [--dims 1024 256] [--nq 4096 1] [--k 65 100 256 1024]
                                      [--steps 2] [--warmup 1] [--out profiles/r30_search_deep.txt]

Per (dim, nq, k): a COSINE index of `rows` unit vectors (seeded), queries = noisy copies of gallery rows.
    exact   FlatIndex.search          k past TIER1_MAX_K: fp64 scores of every row + row top-k (what the parent answers with)
    deep    FlatIndex.search_deep     the filter GEMM with deep candidate lists
The two alternate inside each of three rounds; every figure is a device-synchronised mean over a window of `steps` calls after
`warmup` calls; reported: the median of the three windows and spread = (max - min) / median, and whether deep wins by more than
the two spreads.  Before anything is timed the two results are compared: ids and fp64 scores equal to the bit.  One more deep
call with MIRX_OPT_PROFILE gives the per-stage times (last_timings) and the route's counters (last_stats).  Records are written
as they are produced."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dims", type=int, nargs="+", default=[1024, 256])
    ap.add_argument("--nq", type=int, nargs="+", default=[4096, 1])
    ap.add_argument("--k", type=int, nargs="+", default=[65, 100, 256, 1024])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx import _lib as L
    from mirx.index import FlatIndex, deep_min_rows
    dev = torch.device("cuda:0")
    out_fh = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_fh:
            out_fh.write(line + "\n")
            out_fh.flush()

    emit({"device": torch.cuda.get_device_name(0), "rows": a.rows, "dims": a.dims, "nq": a.nq, "k": a.k, "steps": a.steps,
          "warmup": a.warmup})
    for d in a.dims:
        gen = torch.Generator(device=dev).manual_seed(1)
        g = torch.nn.functional.normalize(torch.randn(a.rows, d, generator=gen, device=dev), dim=1)
        ix = FlatIndex(d, "COSINE", 0)
        ix.add(g)
        for nq in a.nq:
            rows = torch.randint(0, a.rows, (nq,), generator=gen, device=dev)
            q = torch.nn.functional.normalize(g[rows] + 0.5 / d ** 0.5 * torch.randn(nq, d, generator=gen, device=dev), dim=1).contiguous()
            for k in a.k:
                want = ix.search(q, k, return_f64=True)
                got = ix.search_deep(q, k, return_f64=True)
                st = ix.last_stats()
                same = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
                arms = {"exact": lambda: ix.search(q, k), "deep": lambda: ix.search_deep(q, k)}
                win = {name: [] for name in arms}
                for _ in range(3):
                    for name, fn in arms.items():
                        win[name].append(_window(fn, a.steps, a.warmup))
                rec = {"dim": d, "nq": nq, "k": k, "deep_min_rows": deep_min_rows(k, nq), "equal_to_the_bit": same}
                for name, w in win.items():
                    w = sorted(w)
                    rec[name + "_ms"] = round(w[1], 3)
                    rec[name + "_spread"] = round((w[2] - w[0]) / w[1], 4)
                    rec[name + "_windows_ms"] = [round(x, 3) for x in w]
                rec["speedup"] = round(rec["exact_ms"] / rec["deep_ms"], 2)
                rec["deep_wins_by_more_than_the_spreads"] = bool(
                    rec["deep_ms"] * (1 + rec["deep_spread"]) < rec["exact_ms"] * (1 - rec["exact_spread"]))
                ix.set_option(L.OPT_PROFILE, 1)
                ix.search_deep(q, k)
                rec["deep_stage_ms"] = {s: round(v, 3) for s, v in ix.last_timings().items()}
                ix.set_option(L.OPT_PROFILE, 0)
                rec["deep_stats"] = st
                rec["candidates_per_query"] = round(st["candidates"] / max(st["tier1_answered"], 1), 1)
                rec["reranked_per_query"] = round(st["reranked"] / max(st["tier1_answered"], 1), 1)
                emit(rec)
        del ix, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
