"""Hybrid search on one GPU: hybrid_search over two collections beside the two plain searches it is made of (all a caller could
run before), beside the same lists fused on the host with dictionaries, and the fusion kernel alone.

    python tools/bench_hybrid.py [--rows 1048576] [--dims 1024 256] [--nq 4096] [--list 100] [--limit 10] [--sub 64]
                                 [--steps 3] [--warmup 1] [--out profiles/r26_hybrid_search.txt]

Two COSINE collections of `rows` unit vectors (seeded), `dims` floats each.  The first holds paths 0 .. rows-1, the second a
permutation of rows/4 .. rows/4 + rows-1, so three quarters of the documents are in both, under different ids.  A query is a
document held by both: a noisy copy of its row in each collection.  Every request asks for `list` hits, the fusion for `limit`.
Arms, alternating inside each of three rounds in one process on one box:
    (0) two index searches          FlatIndex.search on each collection, results left on the device: the floor of any fusion
    (0) two Collection.search       the same through the public call (one Hit per row found): what a caller had before
    (1) hybrid_search, RRF / weighted   the public call: searches, id -> code, kernel, `limit` Hits per query
    (2) host fusion alone (sub)     the dictionary method over the two Collection.search results of the first `sub` queries
    (3) fuse kernel alone           mirx.index.fuse_ranked on the device-resident codes and distances of all queries
    (4) join table                  built once per state of the collections: the one-off cost (host scan + upload), one window
Every figure is a device-synchronised mean over a window of `steps` calls after `warmup` calls; reported: the median of the three
windows and spread = (max - min) / median.  Before anything is timed hybrid_search is compared with the host fusion on the
`sub` queries: same documents, same order, the same fp64 score bits.  Records are written as they are produced."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_range import _window  # noqa: E402  (the same timing window)


def host_fusion(lists, ranker, limit, code_of):
    """the dictionary method, per query: lists = one list of Hit per request; equal scores by the documents' codes"""
    score = {}
    for r, hits in enumerate(lists):
        for rank, h in enumerate(hits, 1):
            key = h.entity.get("image_path")
            if ranker[0] == "rrf":
                t = 1.0 / (ranker[1] + rank)
            else:
                t = ranker[1][r] * ((1.0 + h.distance) * 0.5)
            score[key] = score.get(key, 0.0) + t
    return sorted(score.items(), key=lambda kv: (-kv[1], code_of[kv[0]]))[:limit]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dims", type=int, nargs=2, default=[1024, 256])
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--list", type=int, default=100)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--sub", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.index import fuse_ranked
    from mirx.retriever import AnnSearchRequest, Collection, RRFRanker, WeightedRanker, _join_table, hybrid_search
    dev = torch.device("cuda:0")
    n, nq, sub, L = a.rows, a.nq, min(a.sub, a.nq), a.list
    gen = torch.Generator(device=dev).manual_seed(1)
    shift = n // 4
    perm = torch.randperm(n, generator=gen, device=dev)
    paths = [[f"img/{i}.png" for i in range(n)], [f"img/{i}.png" for i in (perm + shift).tolist()]]
    cols, rows = [], []
    for name, d, p in zip("ab", a.dims, paths):
        g = torch.nn.functional.normalize(torch.randn(n, d, generator=gen, device=dev), dim=1)
        c = Collection(name, d, metric_type="COSINE")
        c.insert([p, ["l"] * n, g])
        cols.append(c)
        rows.append(g)
    # documents held by both: path shift + j is row shift + j of a and row inv[j] of b
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, device=dev)
    doc = torch.randint(0, n - shift, (nq,), generator=gen, device=dev)
    where = [doc + shift, inv[doc]]
    qs = [torch.nn.functional.normalize(g[w] + 0.02 * torch.randn(nq, g.shape[1], generator=gen, device=dev), dim=1).contiguous()
          for g, w in zip(rows, where)]
    del rows
    out_fh = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_fh:
            out_fh.write(line + "\n")
            out_fh.flush()

    emit({"device": torch.cuda.get_device_name(0), "rows": n, "dims": a.dims, "nq": nq, "list": L, "limit": a.limit, "sub": sub,
          "steps": a.steps, "warmup": a.warmup})
    reqs = [AnnSearchRequest(q, name, limit=L) for q, name in zip(qs, "ab")]
    reqs_sub = [AnnSearchRequest(q[:sub], name, limit=L) for q, name in zip(qs, "ab")]
    by_name = dict(zip("ab", cols))
    rankers = {"RRF": RRFRanker(), "weighted": WeightedRanker(0.6, 0.4)}

    t0 = time.perf_counter()
    table = _join_table(cols, "image_path")
    for ci, c in enumerate(cols):
        table.device_codes(ci, c.index.device)
    torch.cuda.synchronize()
    emit({"arm": "(4) join table: host scan of 2 x rows keys + upload, once per state", "ms": round((time.perf_counter() - t0) * 1e3, 1),
          "documents": len(table.owners)})

    # correctness first: the public call against the dictionary method, to the bit
    code_of = {}
    for p in paths:
        for key in p:
            code_of.setdefault(key, len(code_of))
    lists_sub = [c.search(r.data, limit=L, output_fields=["image_path"]) for c, r in zip(cols, reqs_sub)]
    own = [f"img/{i + shift}.png" for i in doc[:sub].tolist()]
    for rk in rankers.values():
        form = rk.kernel_form(["COSINE", "COSINE"])
        got = hybrid_search(by_name, reqs_sub, rk, a.limit)
        for qi in range(sub):
            want = host_fusion([l[qi] for l in lists_sub], form, a.limit, code_of)
            assert [(h.entity.get("image_path"), h.distance.hex()) for h in got[qi]] == [(k, s.hex()) for k, s in want], qi
        found = sum(1 for qi in range(sub) if got[qi][0].entity.get("image_path") == own[qi])
    emit({"check": "hybrid_search == host dictionary fusion on the sub queries (documents, order, fp64 score bits)",
          "queries_whose_own_document_ranks_first": found})

    # the device-resident inputs of the kernel alone
    codes, dist = [], []
    for ci, (c, q) in enumerate(zip(cols, qs)):
        sc, ids = c.index.search(q, L)
        codes.append(table.device_codes(ci, dev)[c.index._positions(ids)])
        dist.append(sc)
    codes, dist = torch.cat(codes, dim=1).contiguous(), torch.cat(dist, dim=1).contiguous()
    form_rrf, form_w = (rk.kernel_form(["COSINE", "COSINE"]) for rk in rankers.values())

    def two_index_searches():
        for c, q in zip(cols, qs):
            c.index.search(q, L)

    def two_collection_searches():
        for c, q in zip(cols, qs):
            c.search(q, limit=L, output_fields=["image_path"])

    fast, slow = (a.steps, a.warmup), (1, 0)
    arms = {
        "(0) two index searches k=%d, results on the device" % L: (two_index_searches, nq, fast),
        "(0) two Collection.search limit=%d (Hit objects)" % L: (two_collection_searches, nq, slow),
        "(1) hybrid_search RRF": (lambda: hybrid_search(by_name, reqs, rankers["RRF"], a.limit), nq, fast),
        "(1) hybrid_search weighted": (lambda: hybrid_search(by_name, reqs, rankers["weighted"], a.limit), nq, fast),
        "(2) host fusion alone (sub), RRF": (lambda: [host_fusion([l[qi] for l in lists_sub], form_rrf, a.limit, code_of)
                                                      for qi in range(sub)], sub, fast),
        "(3) fuse kernel alone, RRF": (lambda: fuse_ranked(codes, dist, [L, L], form_rrf, a.limit, n_codes=len(table.owners)), nq, fast),
        "(3) fuse kernel alone, weighted": (lambda: fuse_ranked(codes, dist, [L, L], form_w, a.limit, n_codes=len(table.owners)), nq, fast),
    }
    times = {name: [] for name in arms}
    for _ in range(3):
        for name, (fn, _, (steps, warmup)) in arms.items():
            times[name].append(_window(fn, steps, warmup))
            print("# %s: %.3f ms" % (name, times[name][-1]), file=sys.stderr, flush=True)          # (progress; the records follow)
    for name, t in times.items():
        t = sorted(t)
        queries = arms[name][1]
        emit({"arm": name, "queries": queries, "ms": round(t[1], 3), "ms_per_query": round(t[1] / queries, 5),
              "spread": round((t[2] - t[0]) / t[1], 4), "windows_ms": [round(v, 3) for v in t]})
    if out_fh:
        out_fh.close()


if __name__ == "__main__":
    main()
