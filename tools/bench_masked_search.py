"""Search under a row mask on one GPU: FlatIndex.search(allow=) against the unmasked search of the same index and against what
a user had to do before -- build a fresh index of the allowed rows and search that.

    python tools/bench_masked_search.py [--rows 1048576] [--dim 1024] [--steps 3] [--warmup 1] [--out profiles/r22_masked_search.txt]

Gallery: `rows` unit vectors of `dim` floats, ids = 7 + 3 * row; queries are noisy copies of gallery rows; k = 10.  For each metric
(IP, L2) and query count (4096, 1) the arms are
    unmasked              search(q, 10)
    masked f              search(q, 10, allow=mask) with a random device mask that allows the fraction f of the rows
                          (1.0, 0.5, 0.05: the bf16 filter route; 0.01: the gathered exact route)
    fresh f               gather the allowed rows and ids, FlatIndex.add them to a new index, search it, drop it
Every arm is a device-synchronised mean over a window of `steps` calls after `warmup` calls; the arms of one (metric, Q) alternate
inside each of three rounds in one process, and the figure is the median of the three windows with spread = (max - min) / median.
Before anything is timed the masked answers are compared with the fresh index's, bit for bit.  `route` is read from the stats
of the call: tier1 = the bf16 filter answered, exact = the fp64 scan answered.  One JSON line per arm."""
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
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.index import FlatIndex
    dev = torch.device("cuda:0")
    n, d = a.rows, a.dim
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.nn.functional.normalize(torch.randn(n, d, generator=gen, device=dev), dim=1)
    ids = 7 + 3 * torch.arange(n, dtype=torch.int64, device=dev)
    pick = torch.randint(0, n, (4096,), generator=gen, device=dev)
    q_all = torch.nn.functional.normalize(g[pick] + 0.02 * torch.randn(4096, d, generator=gen, device=dev), dim=1)
    fractions = (1.0, 0.5, 0.05, 0.01)
    masks = {f: (torch.rand(n, generator=gen, device=dev) < f) if f < 1.0 else torch.ones(n, dtype=torch.bool, device=dev)
             for f in fractions}
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for metric in ("IP", "L2"):
        ix = FlatIndex(d, metric, 0)
        ix.add(g, ids)

        def fresh_search(f, q):
            m = masks[f]
            fx = FlatIndex(d, metric, 0)
            fx.add(g[m], ids[m])
            return fx.search(q, 10, return_f64=True)

        for f in fractions[1:]:                                     # correctness first: masked == fresh, to the bit
            s1, i1 = ix.search(q_all[:64], 10, return_f64=True, allow=masks[f])
            s2, i2 = fresh_search(f, q_all[:64])
            assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int64), s2.view(torch.int64)), (metric, f)
        for nq in (4096, 1):
            q = q_all[:nq].contiguous()
            arms = {"unmasked": lambda: ix.search(q, 10)}
            for f in fractions:
                arms[f"masked {f}"] = (lambda f=f: ix.search(q, 10, allow=masks[f]))
            for f in fractions[1:]:
                arms[f"fresh {f}"] = (lambda f=f: fresh_search(f, q))
            times = {name: [] for name in arms}
            routes = {}
            for _ in range(3):
                for name, fn in arms.items():
                    fresh = name.startswith("fresh")
                    times[name].append(_window(fn, 1 if fresh else a.steps, 0 if fresh and times[name] else a.warmup))
                    if not fresh:
                        st = ix.last_stats()
                        routes[name] = {"tier1": st["tier1_answered"], "exact": st["exact_answered"]}
            for name, t in times.items():
                t = sorted(t)
                rec = {"metric": metric, "rows": n, "dim": d, "nq": nq, "k": 10, "arm": name, "ms": round(t[1], 3),
                       "spread": round((t[2] - t[0]) / t[1], 4)}
                if name in routes:
                    rec["route"] = routes[name]
                if name.startswith("masked"):
                    rec["allowed_rows"] = int(masks[float(name.split()[1])].sum())
                emit(rec)
        del ix
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
