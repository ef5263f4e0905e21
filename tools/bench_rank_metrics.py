"""The fused, streaming metric tail (FlatIndex.rank_metrics) beside the two-call form it replaces, on one GPU, same
index, same process.

    python tools/bench_rank_metrics.py [--shapes 1048576x256x64 1048576x1024x64 65536x1024x4096] [--steps 2] [--warmup 1]
                                       [--self-eval 112120x256] [--out profiles/r33_rank_metrics.txt]

Per shape rows x dim x nq: a COSINE index of seeded unit rows with labels in 0 .. 13, groups of 1 .. 8 rows; the queries are
gallery rows with their own id excluded and their own code.
    fused       FlatIndex.rank_metrics(row_codes=, query_codes=)                       the new call
    two_call    FlatIndex.rank_all + metrics.rank_metrics_device(gallery_codes=, ..)   the [nq, rows] ranking written and read back
    rank_all    the first half of two_call alone
    one_wave    the second half alone, on a ranking made before: the walk with one wavefront per list
    rank_top1   FlatIndex.rank_top(k = 1): scores + sort + a one-slot write; fused - rank_top1 is the segmented walk's share
The arms alternate inside each of three rounds; every figure is a device-synchronised mean over a window of `steps` calls after
`warmup` calls; reported: the median of the three windows and spread = (max - min) / median.  Before anything is timed the two
forms are compared: integer outputs equal, largest |AP difference|.
--self-eval N x dim: nih.evaluate_map(groups=) over N synthetic images with 14-bit labels (wall time of one call after a warm-up
on 2048 images, torch.cuda.max_memory_allocated, and the ranking workspace of the index computed from its plan)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KAPPAS = (1, 5, 10)


def _window(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _groups(n, gen, dev):
    """codes of groups of sizes 1 .. 8 dealt to a permutation of the rows (36 rows per cycle of eight groups)"""
    sizes = torch.arange(n, device=dev) % 36
    starts = torch.tensor([0, 1, 3, 6, 10, 15, 21, 28], device=dev)
    in_cycle = torch.bucketize(sizes, starts, right=True) - 1
    codes = (torch.arange(n, device=dev) // 36) * 8 + in_cycle
    return codes[torch.randperm(n, generator=gen, device=dev)].to(torch.int32).contiguous()


class _Lookup(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, idx):
        return {"embedding": self.table[idx]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["1048576x256x64", "1048576x1024x64", "65536x1024x4096"])
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--self-eval", default="112120x256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx import nih
    from mirx.index import FlatIndex
    from mirx.metrics import rank_metrics_device
    dev = torch.device("cuda:0")
    out_fh = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_fh:
            out_fh.write(line + "\n")
            out_fh.flush()

    emit({"device": torch.cuda.get_device_name(0), "shapes": a.shapes, "steps": a.steps, "warmup": a.warmup, "kappas": KAPPAS})
    for shape in a.shapes:
        rows, d, nq = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(1)
        g = torch.nn.functional.normalize(torch.randn(rows, d, generator=gen, device=dev), dim=1)
        ix = FlatIndex(d, "COSINE", 0)
        ix.add(g)                                                     # auto ids: a row's id is its number
        labels = torch.randint(0, 14, (rows,), generator=gen, device=dev)
        codes = _groups(rows, gen, dev)
        own = torch.randint(0, rows, (nq,), generator=gen, device=dev)
        q, ql, qc = g[own].contiguous(), labels[own].contiguous(), codes[own].contiguous()
        del g

        def fused():
            return ix.rank_metrics(q, labels, ql, KAPPAS, exclude_ids=own, self_kind=0, row_codes=codes, query_codes=qc)

        def walk(ranks):
            return rank_metrics_device(ranks, labels, ql, KAPPAS, gallery_codes=codes, query_codes=qc)

        def two_call():
            return walk(ix.rank_all(q, exclude_ids=own))

        one, two = fused(), two_call()
        same = all(bool(torch.equal(one[k], two[k])) for k in ("cnt", "nrel", "maxpos"))
        nan_same = bool(torch.equal(torch.isnan(one["ap"]), torch.isnan(two["ap"])))
        ap_diff = float(torch.nan_to_num(one["ap"] - two["ap"]).abs().max())
        kept = ix.rank_all(q, exclude_ids=own)
        arms = {"fused": fused, "two_call": two_call, "rank_all": lambda: ix.rank_all(q, exclude_ids=own),
                "one_wave": lambda: walk(kept), "rank_top1": lambda: ix.rank_top(q, 1, exclude_ids=own)}
        win = {name: [] for name in arms}
        for _ in range(3):
            for name, fn in arms.items():
                win[name].append(_window(fn, a.steps, a.warmup))
        rec = {"rows": rows, "dim": d, "nq": nq, "integers_equal": same, "nan_in_the_same_places": nan_same, "max_abs_ap_diff": ap_diff,
               "mean_ap": float(torch.nanmean(one["ap"]))}
        for name, w in win.items():
            w = sorted(w)
            rec[name + "_ms"] = round(w[1], 3)
            rec[name + "_spread"] = round((w[2] - w[0]) / w[1], 4)
            rec[name + "_windows_ms"] = [round(x, 3) for x in w]
        rec["segmented_walk_share_ms"] = round(rec["fused_ms"] - rec["rank_top1_ms"], 3)
        rec["two_call_over_fused"] = round(rec["two_call_ms"] / rec["fused_ms"], 3)
        emit(rec)
        del ix, kept, one, two
        torch.cuda.empty_cache()

    if a.self_eval:
        n, d = (int(v) for v in a.self_eval.split("x"))
        gen = torch.Generator(device=dev).manual_seed(2)
        table = torch.randn(n, d, generator=gen, device=dev)
        multi = (torch.rand(n, 14, generator=gen, device=dev) < 0.12).float().cpu()
        groups = _groups(n, gen, dev).cpu().numpy()
        model = _Lookup(table)

        def loader(m):
            return [(torch.arange(s, min(s + 8192, m)), multi[s:min(s + 8192, m)]) for s in range(0, m, 8192)]

        nih.evaluate_map(model, loader(2048), dev, 0.4, groups=groups[:2048])          # warm-up: code objects, allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rec = {"self_eval_images": n, "dim": d}
        for name, gr in (("with_groups", groups), ("without_groups", None)):
            t0 = time.perf_counter()
            m_ap = nih.evaluate_map(model, loader(n), dev, 0.4, groups=gr)
            torch.cuda.synchronize()
            rec[name + "_wall_s"] = round(time.perf_counter() - t0, 3)
            rec[name + "_mAP_percent"] = m_ap
        rec["torch_max_memory_allocated_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        ld = (n + 63) // 64 * 64
        per = max(1, min((1 << 29) // (ld * 32), 1024))
        rec["queries_per_batch"] = per
        rec["ranking_workspace_MiB"] = round(per * (ld * 8 + n * 24) / 2 ** 20, 1)
        rec["an_n_by_n_int64_ranking_would_take_GiB"] = round(n * n * 8 / 2 ** 30, 1)
        emit(rec)


if __name__ == "__main__":
    main()
