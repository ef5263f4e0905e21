"""Leave-group-out search beside its floor and beside what a caller had before it, on one GPU, same index, same process.

    python tools/bench_leave_out.py [--rows 1048576] [--dims 1024 256] [--nq 4096 1] [--k 10 100] [--groups 8 100]
                                    [--steps 2] [--warmup 1] [--out profiles/r32_leave_out.txt]

Per (dim, group size G, nq, k): a COSINE index of `rows` unit vectors (seeded) whose rows carry the code row // G scattered by a
permutation (rows / G groups of G rows); queries are gallery rows with their own codes, so every query leaves out its own row
and the G - 1 others of its group.
    leave_out  FlatIndex.search_leave_out(max_left_out=G)      the new call
    floor      FlatIndex.search / search_deep(exclude_ids=own)  the parent's call: the same work minus the predicate
    deepen     search_deep(k + G) + a torch gather of the codes, the mask and a stable first-k selection: what a caller does
               without the new call (only the ids are selected; the scores would cost another gather)
The arms alternate inside each of three rounds; every figure is a device-synchronised mean over a window of `steps` calls after
`warmup` calls; reported: the median of the three windows and spread = (max - min) / median.  Before anything is timed the new
call's result is compared, ids and fp64 scores to the bit, with the per-code masked search on a sample of queries, and the
`deepen` arm's ids with the new call's.  One more call with MIRX_OPT_PROFILE gives the stage times (last_timings) and the
counters (last_stats: left_out, and how many queries the guard sent on).  Records are written as they are produced.  The group-of-
100 arm runs at the first nq and k only."""
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
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--groups", type=int, nargs="+", default=[8, 100])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx import _lib as L
    from mirx.index import FlatIndex, tier1_max_k
    dev = torch.device("cuda:0")
    out_fh = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_fh:
            out_fh.write(line + "\n")
            out_fh.flush()

    emit({"device": torch.cuda.get_device_name(0), "rows": a.rows, "dims": a.dims, "nq": a.nq, "k": a.k, "groups": a.groups,
          "steps": a.steps, "warmup": a.warmup})
    for d in a.dims:
        gen = torch.Generator(device=dev).manual_seed(1)
        g = torch.nn.functional.normalize(torch.randn(a.rows, d, generator=gen, device=dev), dim=1)
        ix = FlatIndex(d, "COSINE", 0)
        ix.add(g)                                                   # auto ids: a row's id is its number
        perm = torch.randperm(a.rows, generator=gen, device=dev)
        for gi, G in enumerate(a.groups):
            codes = (perm // G).to(torch.int32).contiguous()
            for nq in (a.nq if gi == 0 else a.nq[:1]):
                own = torch.randint(0, a.rows, (nq,), generator=gen, device=dev)
                q = g[own].contiguous()
                qc = codes[own].contiguous()
                for k in (a.k if gi == 0 else a.k[:1]):
                    floor_find = ix.search if k + 1 <= tier1_max_k() else ix.search_deep

                    def deepen():
                        _, ids = ix.search_deep(q, k + G)
                        keep = codes[ids.clamp_min(0)] != qc[:, None]
                        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :k]
                        return ids.gather(1, order)

                    got = ix.search_leave_out(q, k, codes, qc, return_f64=True, max_left_out=G)
                    st = ix.last_stats()
                    same = True
                    for i in range(0, nq, max(nq // a.sample, 1)):
                        want = (ix.search if k <= tier1_max_k() else ix.search_deep)(q[i:i + 1], k, return_f64=True,
                                                                                     allow=codes != qc[i])
                        same = same and bool(torch.equal(got[0][i:i + 1], want[0]) and torch.equal(got[1][i:i + 1], want[1]))
                    deepen_same = bool(torch.equal(deepen(), got[1]))
                    arms = {"leave_out": lambda: ix.search_leave_out(q, k, codes, qc, max_left_out=G),
                            "floor": lambda: floor_find(q, k, exclude_ids=own),
                            "deepen": deepen}
                    win = {name: [] for name in arms}
                    for _ in range(3):
                        for name, fn in arms.items():
                            win[name].append(_window(fn, a.steps, a.warmup))
                    rec = {"dim": d, "group": G, "nq": nq, "k": k, "equal_to_the_bit_to_the_masked_search": same,
                           "deepen_ids_equal": deepen_same}
                    for name, w in win.items():
                        w = sorted(w)
                        rec[name + "_ms"] = round(w[1], 3)
                        rec[name + "_spread"] = round((w[2] - w[0]) / w[1], 4)
                        rec[name + "_windows_ms"] = [round(x, 3) for x in w]
                    rec["over_floor"] = round(rec["leave_out_ms"] / rec["floor_ms"], 3)
                    rec["deepen_over_leave_out"] = round(rec["deepen_ms"] / rec["leave_out_ms"], 2)
                    ix.set_option(L.OPT_PROFILE, 1)
                    ix.search_leave_out(q, k, codes, qc, max_left_out=G)
                    rec["leave_out_stage_ms"] = {s: round(v, 3) for s, v in ix.last_timings().items()}
                    floor_find(q, k, exclude_ids=own)
                    rec["floor_stage_ms"] = {s: round(v, 3) for s, v in ix.last_timings().items()}
                    ix.set_option(L.OPT_PROFILE, 0)
                    rec["leave_out_stats"] = st
                    rec["left_out_per_query"] = round(st["left_out"] / max(st["tier1_answered"], 1), 2)
                    rec["retried_or_scanned"] = {"incomplete": st["incomplete"], "overflowed": st["overflowed"],
                                                 "exact_answered": st["exact_answered"]}
                    emit(rec)
        del ix, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
