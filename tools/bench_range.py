"""Range search on one GPU: FlatIndex.range_search against the top-10 search of the PARENT commit's library (the yardstick), and
against itself forced onto the exact route.

    python tools/bench_range.py [--parent-lib path/to/parent/libmirx.so] [--rows 1048576] [--dim 1024] [--nq 4096]
                                [--steps 3] [--warmup 1] [--out profiles/r24_range_search.txt]

Gallery: `rows` unit vectors of `dim` floats (seed 1), ids = 7 + 3 * row; queries are noisy copies of gallery rows; COSINE.
Arms, alternating inside each of three rounds in one process on one box:
    (a) parent search k=10   mirx_index_search of the library at --parent-lib (built from the parent commit into a scratch
                             directory), loaded by path beside this tree's and driven through the C ABI on the same arrays;
                             without --parent-lib the arm runs this tree's search and says so
    (b) range ~10 / ~256     range_search(q, lo) with lo set from the exact scores of 64 of the queries so that the mean number of
                             hits per query is about 10 / about 256
    (c) the same two calls under MIRX_OPT_TIERS = MIRX_TIER_EXACT_ONLY (one call per window: they take seconds)
Every figure is a device-synchronised mean over a window of `steps` calls after `warmup` calls; reported: the median of the three
windows and spread = (max - min) / median.  (b) == (c) is checked bit for bit before anything is timed.  Each range line carries
the call's own stats (filter / exact answered, candidates, hits) and `gather_bytes` = candidates * dimp * 4: what the fp64
re-score of every candidate reads of the fp32 gallery (DERIVED from the recorded candidate count, not measured)."""
import argparse
import ctypes
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


class _ParentIndex:
    """the few calls of the parent library this tool needs, bound by hand: its ABI is this tree's minus the range entry points"""

    def __init__(self, path, dim, rows, ids):
        from mirx import _lib
        self.lib = ctypes.CDLL(path)
        for name in ("mirx_index_create", "mirx_index_add", "mirx_index_search", "mirx_index_destroy", "mirx_version"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = _lib.SYMBOLS[name]
        self.version = self.lib.mirx_version()
        self.h = ctypes.c_void_p()
        assert self.lib.mirx_index_create(dim, 0, 0, ctypes.byref(self.h)) == 0
        torch.cuda.synchronize()
        assert self.lib.mirx_index_add(self.h, ctypes.c_void_p(rows.data_ptr()), rows.shape[0], ctypes.c_void_p(ids.data_ptr())) == 0

    def search(self, q, k):
        sc = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
        ids = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
        rc = self.lib.mirx_index_search(self.h, ctypes.c_void_p(q.data_ptr()), q.shape[0], k, None, ctypes.c_void_p(sc.data_ptr()),
                                        ctypes.c_void_p(ids.data_ptr()),
                                        ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream))
        assert rc == 0
        return sc, ids

    def close(self):
        self.lib.mirx_index_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx import _lib
    from mirx.index import FlatIndex
    dev = torch.device("cuda:0")
    n, d, nq = a.rows, a.dim, a.nq
    dimp = (d + 127) // 128 * 128
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.nn.functional.normalize(torch.randn(n, d, generator=gen, device=dev), dim=1)
    ids = 7 + 3 * torch.arange(n, dtype=torch.int64, device=dev)
    pick = torch.randint(0, n, (nq,), generator=gen, device=dev)
    q = torch.nn.functional.normalize(g[pick] + 0.02 * torch.randn(nq, d, generator=gen, device=dev), dim=1).contiguous()
    ix = FlatIndex(d, "COSINE", 0)
    ix.add(g, ids)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    emit({"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "nq": nq, "steps": a.steps, "warmup": a.warmup})
    # lo for about h hits per query: between the pooled (64 h)-th and the next exact score of 64 of the queries
    s64, _ = ix.search(q[:64], 1024, return_f64=True)
    pooled = s64.reshape(-1).sort(descending=True).values
    los = {h: float((pooled[64 * h - 1] + pooled[64 * h]) / 2) for h in (10, 256)}
    assert pooled[64 * 256] > s64[:, -1].max()                      # the 1024 kept per query cover the pooled prefix

    def forced(fn):
        ix.set_option(_lib.OPT_TIERS, _lib.TIER_EXACT_ONLY)
        try:
            return fn()
        finally:
            ix.set_option(_lib.OPT_TIERS, _lib.TIER_AUTO)

    stats = {}
    for h, lo in los.items():                                       # correctness first: the routes agree, to the bit
        l1, s1, i1 = ix.range_search(q, lo, return_f64=True)
        stats[h] = ix.range_last_stats()
        l2, s2, i2 = forced(lambda: ix.range_search(q, lo, return_f64=True))
        stats[("exact", h)] = ix.range_last_stats()
        assert torch.equal(l1, l2) and torch.equal(i1, i2) and torch.equal(s1.view(torch.int64), s2.view(torch.int64)), h
    parent = _ParentIndex(a.parent_lib, d, g, ids) if a.parent_lib else None
    if parent:
        sp, ip = parent.search(q, 10)
        st, it = ix.search(q, 10)
        assert torch.equal(ip, it) and torch.equal(sp.view(torch.int32), st.view(torch.int32))
    arms = {"(a) parent search k=10" if parent else "(a) THIS TREE's search k=10 (no --parent-lib)":
            ((lambda: parent.search(q, 10)) if parent else (lambda: ix.search(q, 10)), a.steps, a.warmup)}
    for h, lo in los.items():
        arms["(b) range ~%d" % h] = ((lambda lo=lo: ix.range_search(q, lo)), a.steps, a.warmup)
    for h, lo in los.items():
        arms["(c) range ~%d exact" % h] = ((lambda lo=lo: forced(lambda: ix.range_search(q, lo))), 1, 0)
    times = {name: [] for name in arms}
    for _ in range(3):
        for name, (fn, steps, warmup) in arms.items():
            times[name].append(_window(fn, steps, warmup))
    for name, t in times.items():
        t = sorted(t)
        rec = {"arm": name, "ms": round(t[1], 3), "spread": round((t[2] - t[0]) / t[1], 4), "windows_ms": [round(v, 3) for v in t]}
        if "range" in name:
            h = int(name.split("~")[1].split()[0])
            st = stats[("exact", h)] if "exact" in name else stats[h]
            rec.update(lo=los[h], stats=st, hits_per_query=round(st["hits"] / nq, 2))
            if "exact" not in name:
                rec.update(candidates_per_query=round(st["candidates"] / nq, 2), gather_bytes_derived=st["candidates"] * dimp * 4)
        emit(rec)
    if parent:
        emit({"parent_lib_version": parent.version})
        parent.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
