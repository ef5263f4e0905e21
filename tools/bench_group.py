"""Grouping search on one GPU: every route of FlatIndex.search_grouped beside the top-10 search of the PARENT commit's library (the
yardstick), beside what a caller had to do without it, and the figures behind the routing constants.

    python tools/bench_group.py [--parent-lib path/to/parent/libmirx.so] [--rows 1048576] [--dim 1024] [--nq 4096] [--sub 64]
                                [--steps 3] [--warmup 1] [--out profiles/r25_group_search.txt]

Gallery: `rows` unit vectors of `dim` floats (seed 1), ids 0 .. rows-1; queries are noisy copies of gallery rows; COSINE.
Arms, alternating inside each of three rounds in one process on one box (`nq` queries unless the arm says `sub`: the slow arms
run on the first `sub` queries and one call per window):
    (0) parent search k=10     mirx_index_search of the library at --parent-lib, driven through the C ABI on the same arrays;
                               without --parent-lib the arm runs this tree's search and says so
    (a) direct, 3 / 15 labels  balanced labels, limit = all, group_size 1, beside the same number of masked search(k=1) calls made
                               by hand (what Collection.search(expr='label == ..') per label costs at the index)
    (b) walk / walk + fill     2^17 groups of 8, limit 10, group_size 1 / 3; beside rank_top(k=8192) + a host walk of the ids (sub)
    (c) deepen                 the same call forced onto route="deepen" (sub); each (b) line carries the share of queries that
                               needed deepening
    (d) prefixes alone         search(k=64, fp64) as the walk takes it (the filter-GEMM tier), search(k=256) as a limit of 64
                               takes it (the exact tier, sub), and that grouping call (sub)
    (x) crossovers (sub)     direct against walk at 15 / 32 / 64 balanced labels (GROUP_DIRECT_MAX); groups of 4096 rows
                               completed by the fill against the same call deepening (GROUP_FILL_MAX)
    (1) one query              the arms (0), (a), (b) with a single query
Every figure is a device-synchronised mean over a window of `steps` calls after `warmup` calls; reported: the median of the three
windows and spread = (max - min) / median, and `x_parent` = the arm's time per query over the parent top-10's time per query.
Before anything is timed the routes are compared bit for bit on the `sub` queries.  Records are written as they are produced."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_range import _ParentIndex, _window  # noqa: E402  (the same parent binding and timing window)


def _host_walk(ids, codes, limit, group_size):
    """what a caller did by hand: walk each query's ranked ids on the host"""
    out = []
    for row in ids.tolist():
        slots, where = [], {}
        for i in row:
            if i < 0:
                break
            c = codes[i]
            s = where.get(c)
            if s is None:
                if len(slots) >= limit:
                    continue
                s = where[c] = len(slots)
                slots.append([])
            if len(slots[s]) < group_size:
                slots[s].append(i)
        out.append(slots)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--sub", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.index import GROUP_DIRECT_MAX, GROUP_FILL_MAX, FlatIndex
    dev = torch.device("cuda:0")
    n, d, nq, sub = a.rows, a.dim, a.nq, min(a.sub, a.nq)
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.nn.functional.normalize(torch.randn(n, d, generator=gen, device=dev), dim=1)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    pick = torch.randint(0, n, (nq,), generator=gen, device=dev)
    q = torch.nn.functional.normalize(g[pick] + 0.02 * torch.randn(nq, d, generator=gen, device=dev), dim=1).contiguous()
    qs, q1 = q[:sub].contiguous(), q[:1].contiguous()
    ix = FlatIndex(d, "COSINE", 0)
    ix.add(g, ids)
    out_fh = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_fh:
            out_fh.write(line + "\n")
            out_fh.flush()

    emit({"device": torch.cuda.get_device_name(0), "rows": n, "dim": d, "nq": nq, "sub": sub, "steps": a.steps, "warmup": a.warmup,
          "GROUP_DIRECT_MAX": GROUP_DIRECT_MAX, "GROUP_FILL_MAX": GROUP_FILL_MAX})
    perm = torch.randperm(n, generator=gen, device=dev)
    labels = {k: (perm % k).contiguous() for k in (3, 15, 32, 64)}              # balanced labels
    small = (perm % max(n // 8, 1)).contiguous()                               # groups of 8
    big = (perm % max(n // GROUP_FILL_MAX, 1)).contiguous()                    # groups of GROUP_FILL_MAX rows
    masks = {k: [(labels[k] == c).view(torch.uint8) for c in range(k)] for k in (3, 15)}

    def same(x, y):
        return all(torch.equal(u, v) for u, v in zip(x, y))

    # correctness first: the routes agree, to the bit
    for codes, limit, gs, routes in ((labels[15], 15, 1, ("direct", "walk")), (small, 10, 1, ("walk", "deepen")),
                                     (small, 10, 3, ("walk", "deepen")), (big, 10, 3, ("walk", "deepen"))):
        ref = ix.search_grouped(qs, codes, limit, gs, return_f64=True, route=routes[0])
        assert same(ref, ix.search_grouped(qs, codes, limit, gs, return_f64=True, route=routes[1])), (limit, gs, routes)
    # the host walk of a k = 8192 prefix decides the groups (group_size 1); it cannot promise a group's further rows, which may
    # rank anywhere in the gallery -- that arm is timed with group_size 3 as the cost a caller paid for an incomplete answer
    host = _host_walk(ix.rank_top(qs, 8192)[1].cpu(), small.cpu().tolist(), 10, 1)
    assert ix.search_grouped(qs, small, 10, 1)[0].cpu().tolist() == host
    parent = _ParentIndex(a.parent_lib, d, g, ids) if a.parent_lib else None
    if parent:
        sp, ip = parent.search(q, 10)
        st, it = ix.search(q, 10)
        assert torch.equal(ip, it) and torch.equal(sp.view(torch.int32), st.view(torch.int32))
    top10 = (lambda x: parent.search(x, 10)) if parent else (lambda x: ix.search(x, 10))

    def by_hand(x, k):
        for m in masks[k]:
            ix.search(x, 1, allow=m)

    def rank_and_walk():
        _host_walk(ix.rank_top(qs, 8192)[1].cpu(), small_host, 10, 3)

    small_host = small.cpu().tolist()
    fast, slow = (a.steps, a.warmup), (1, 0)
    name0 = "(0) parent search k=10" if parent else "(0) THIS TREE's search k=10 (no --parent-lib)"
    grouped = lambda x, codes, limit, gs, route="auto": (lambda: ix.search_grouped(x, codes, limit, gs, route=route))
    arms = {
        name0: (lambda: top10(q), nq, fast, None),
        "(a) direct 3 labels": (grouped(q, labels[3], 3, 1), nq, fast, True),
        "(a) by hand: 3 masked search k=1": (lambda: by_hand(q, 3), nq, fast, None),
        "(a) direct 15 labels": (grouped(q, labels[15], 15, 1), nq, fast, True),
        "(a) by hand: 15 masked search k=1": (lambda: by_hand(q, 15), nq, fast, None),
        "(b) walk: 2^17 groups of 8, limit 10, group_size 1": (grouped(q, small, 10, 1), nq, fast, True),
        "(b) walk + fill: the same, group_size 3": (grouped(q, small, 10, 3), nq, fast, True),
        "(b) by hand (sub): rank_top k=8192 + host walk": (rank_and_walk, sub, slow, None),
        "(c) deepen forced (sub): group_size 1": (grouped(qs, small, 10, 1, "deepen"), sub, slow, True),
        "(c) deepen forced (sub): group_size 3": (grouped(qs, small, 10, 3, "deepen"), sub, slow, True),
        "(x) fill (sub): groups of %d rows, limit 10, group_size 3" % GROUP_FILL_MAX: (grouped(qs, big, 10, 3), sub, slow, True),
        "(x) deepen forced (sub): the same": (grouped(qs, big, 10, 3, "deepen"), sub, slow, True),
        "(1) parent search k=10, one query": (lambda: top10(q1), 1, fast, None),
        "(1) direct 3 labels, one query": (grouped(q1, labels[3], 3, 1), 1, fast, True),
        "(1) direct 15 labels, one query": (grouped(q1, labels[15], 15, 1), 1, fast, True),
        "(1) walk group_size 1, one query": (grouped(q1, small, 10, 1), 1, fast, True),
        "(1) walk + fill group_size 3, one query": (grouped(q1, small, 10, 3), 1, fast, True),
    }
    arms.update({
        "(d) first prefix alone: search k=64 fp64": (lambda: ix.search(q, 64, return_f64=True), nq, fast, None),
        "(d) first prefix alone (sub): search k=64 fp64": (lambda: ix.search(qs, 64, return_f64=True), sub, fast, None),
        "(d) large-limit prefix alone (sub): search k=256 fp64, the exact tier": (lambda: ix.search(qs, 256, return_f64=True), sub, slow, None),
        "(d) large limit (sub): 2^17 groups of 8, limit 64, group_size 1": (grouped(qs, small, 64, 1), sub, slow, True),
    })
    for k in (15, 32, 64):
        arms["(x) direct (sub): %d labels, limit all" % k] = (grouped(qs, labels[k], k, 1, "direct"), sub, slow, True)
        arms["(x) walk forced (sub): %d labels, limit all" % k] = (grouped(qs, labels[k], k, 1, "walk"), sub, slow, True)
    times, stats = {name: [] for name in arms}, {}
    for _ in range(3):
        for name, (fn, _, (steps, warmup), has_stats) in arms.items():
            times[name].append(_window(fn, steps, warmup))
            print("# %s: %.3f ms" % (name, times[name][-1]), file=sys.stderr, flush=True)      # (progress; the records follow)
            if has_stats:
                stats[name] = ix.group_last_stats()
    base = {nq: None, 1: None}
    for name, t in times.items():
        t = sorted(t)
        queries = arms[name][1]
        rec = {"arm": name, "queries": queries, "ms": round(t[1], 3), "ms_per_query": round(t[1] / queries, 5),
               "spread": round((t[2] - t[0]) / t[1], 4), "windows_ms": [round(v, 3) for v in t]}
        if name.startswith("(0)"):
            base[nq] = t[1] / queries
        if name.startswith("(1) parent"):
            base[1] = t[1]
        ref = base[1] if queries == 1 else base[nq]
        if ref:
            rec["x_parent"] = round(t[1] / queries / ref, 2)
        if name in stats:
            st = stats[name]
            rec.update(stats=st, deepen_share=round(st["deepen"] / max(st["nq"], 1), 4))
        emit(rec)
    if parent:
        emit({"parent_lib_version": parent.version})
        parent.close()
    if out_fh:
        out_fh.close()


if __name__ == "__main__":
    main()
