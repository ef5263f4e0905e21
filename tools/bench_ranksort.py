"""Full ranking on one GPU: FlatIndex.rank_all with the bitonic network and with the radix sort on the largest gallery both take
(nq 64, n 65536, d 256), rank_all on the README's gallery size (nq 64, n 2^20, d 256), and rank_top(k = 2000) at (nq 64, n 2^20,
d 1024).  Every call includes the fp64 score tiles it sorts; `ms_scores_topk10` (an exact-tier search with k = 10 on the same
index: the same score tiles and a cheap selection) is printed beside it to show how much of a call is not the sort.

    python tools/bench_ranksort.py [--steps 5] [--warmup 2] [--min-window-ms 250] [--out profiles/r14_ranksort.txt]

Times are CUDA-event means over a window of at least `steps` calls and at least `min-window-ms` (sized from one timed call) after
`warmup` calls, measured three times: the figure is the median and `spread` the (max - min) / median of the three.  The two sorts
of the first case alternate in one process on one index, and their outputs are compared bit for bit before anything is timed.
One JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


MIN_WINDOW_MS = 250.0


def _time3(fn, steps, warmup):
    """(median of three windows, (max - min) / median)"""
    steps = max(steps, int(MIN_WINDOW_MS / max(_time(fn, 1, warmup), 1e-3)) + 1)
    t = sorted(_time(fn, steps, warmup) for _ in range(3))
    return round(t[1], 3), round((t[2] - t[0]) / t[1], 4)


def _gallery(n, d, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=dev), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-window-ms", type=float, default=250.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    global MIN_WINDOW_MS
    MIN_WINDOW_MS = a.min_window_ms
    from mirx import _lib
    from mirx.index import FlatIndex
    assert torch.cuda.is_available(), "bench_ranksort needs a GPU"
    dev = torch.device("cuda:0")
    res = []

    def emit(d):
        print(json.dumps(d), flush=True)
        res.append(d)

    def index(n, d):
        ix = FlatIndex(d, "COSINE", 0)
        ix.add(_gallery(n, d, 1, dev))
        ix.set_option(_lib.OPT_TIERS, _lib.TIER_EXACT_ONLY)          # the k = 10 companion scores every row in fp64 too
        return ix, _gallery(64, d, 2, dev)

    # (nq 64, n 65536, d 256): the two sorts on one index
    n, d = 65536, 256
    ix, q = index(n, d)
    out = {}
    for name, sort in (("bitonic", _lib.RANK_SORT_BITONIC), ("radix", _lib.RANK_SORT_RADIX)):
        ix.set_option(_lib.OPT_RANK_SORT, sort)
        out[name] = ix.rank_all(q, with_scores=True)
    assert torch.equal(out["bitonic"][0], out["radix"][0]) and torch.equal(out["bitonic"][1], out["radix"][1])
    del out
    row = {"call": "rank_all", "nq": 64, "n": n, "d": d}
    for rep in range(2):                                              # alternate the two, twice
        for name, sort in (("bitonic", _lib.RANK_SORT_BITONIC), ("radix", _lib.RANK_SORT_RADIX)):
            ix.set_option(_lib.OPT_RANK_SORT, sort)
            row[f"ms_{name}_{rep}"], row[f"spread_{name}_{rep}"] = _time3(lambda: ix.rank_all(q, with_scores=True), a.steps, a.warmup)
    row["ms_scores_topk10"], _ = _time3(lambda: ix.search(q, 10), a.steps, a.warmup)
    row["radix_over_bitonic"] = round((row["ms_radix_0"] + row["ms_radix_1"]) / (row["ms_bitonic_0"] + row["ms_bitonic_1"]), 4)
    emit(row)
    del ix
    torch.cuda.empty_cache()

    # (nq 64, n 2^20, d 256): rank_all, sort option on auto
    n, d = 1 << 20, 256
    ix, q = index(n, d)
    row = {"call": "rank_all", "nq": 64, "n": n, "d": d}
    row["ms_auto"], row["spread_auto"] = _time3(lambda: ix.rank_all(q, with_scores=True), a.steps, a.warmup)
    row["ms_scores_topk10"], _ = _time3(lambda: ix.search(q, 10), a.steps, a.warmup)
    emit(row)
    del ix
    torch.cuda.empty_cache()

    # (nq 64, n 2^20, d 1024): rank_top(k = 2000)
    n, d = 1 << 20, 1024
    ix, q = index(n, d)
    row = {"call": "rank_top", "k": 2000, "nq": 64, "n": n, "d": d}
    row["ms"], row["spread"] = _time3(lambda: ix.rank_top(q, 2000), a.steps, a.warmup)
    row["ms_scores_topk10"], _ = _time3(lambda: ix.search(q, 10), a.steps, a.warmup)
    emit(row)

    if a.out:
        with open(a.out, "w") as fh:
            fh.write(f"# tools/bench_ranksort.py on {torch.cuda.get_device_name(0)}: steps >= {a.steps}, windows >= "
                     f"{a.min_window_ms:g} ms, warmup {a.warmup}; ms per call of 64 queries, scores included\n")
            for d_ in res:
                fh.write(json.dumps(d_) + "\n")


if __name__ == "__main__":
    main()
