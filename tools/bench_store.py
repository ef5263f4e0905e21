"""Measurements of DESIGN.md 31 (profiles/r21_store.txt): Collection.load() from a store against Collection.insert of the same
rows from host memory, FlatIndex.remove against a fresh index re-added from the survivors, and a plain device copy of the bytes
the row moves carry.  The two sides of each pair alternate in one process; every figure is printed per repetition.

  python tools/bench_store.py [--rows 1000000] [--dim 1024] [--reps 5] [--dir DIR]
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_store.py --remove-only      (the kernels' split)
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mirx import retriever as R  # noqa: E402
from mirx import store as S  # noqa: E402
from mirx.index import FlatIndex  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(name, xs, extra=""):
    xs = sorted(xs)
    print(f"{name}: min {xs[0] * 1e3:.1f} ms  median {xs[len(xs) // 2] * 1e3:.1f} ms  max {xs[-1] * 1e3:.1f} ms  "
          f"({', '.join(f'{x * 1e3:.1f}' for x in xs)}) {extra}", flush=True)


def bench_load(args, rows):
    n, dim = rows.shape
    R.MODEL_CONFIGS["bench"] = {"embedding_dim": dim, "description": "bench", "collection_names": {"default": "bench_gallery"}}
    root = tempfile.mkdtemp(dir=args.dir)
    try:
        paths, labels = [f"img/{i}.png" for i in range(n)], [i % 7 for i in range(n)]
        col = R.MilvusManager(uri=root).create_collection("bench")
        step = 100000
        t_flush = 0.0
        for s in range(0, n, step):
            col.insert([paths[s:s + step], labels[s:s + step], rows[s:s + step]])
            t0 = time.perf_counter()
            col.flush()
            t_flush += time.perf_counter() - t0
        size = os.path.getsize(os.path.join(root, "bench_gallery", "rows.0.f32"))
        print(f"store written: {n} x {dim}, rows file {size / 2 ** 30:.2f} GiB, {n // step} flushes {t_flush:.2f} s in all", flush=True)
        t_read = []
        for _ in range(2):                                   # the file read alone, warm page cache (the first pass warms it)
            stored = R.MilvusManager(uri=root)._disk.open("bench_gallery")
            t0 = time.perf_counter()
            got = sum(r.shape[0] for _, r in stored.chunks())
            t_read.append(time.perf_counter() - t0)
            assert got == n
        print(f"file read alone (chunks of {S.LOAD_CHUNK_BYTES >> 20} MiB): "
              f"{t_read[-1]:.3f} s = {size / t_read[-1] / 1e9:.2f} GB/s", flush=True)
        t_load, t_insert, t_open = [], [], []
        for rep in range(args.reps):
            t0 = time.perf_counter()
            c = R.MilvusManager(uri=root).create_collection("bench")          # metadata from disk, nothing resident
            t_open.append(time.perf_counter() - t0)
            dt, _ = timed(c.load)
            t_load.append(dt)
            assert len(c.index) == n
            del c
            m = R.MilvusManager(uri=None).create_collection("bench")
            dt, _ = timed(lambda: m.insert([paths, labels, rows]))
            t_insert.append(dt)
            assert len(m.index) == n
            del m
        spread("open (manifest, ids, columns)", t_open)
        spread("Collection.load() from the store", t_load, f"= {size / min(t_load) / 1e9:.2f} GB/s at best")
        spread("Collection.insert from host memory", t_insert)
    finally:
        shutil.rmtree(root, ignore_errors=True)
        R.MODEL_CONFIGS.pop("bench", None)


def bench_remove(args, rows_dev, frac, reps):
    n, dim = rows_dev.shape
    ids = torch.arange(n, dtype=torch.int64, device="cuda")
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))[: int(n * frac)].to("cuda")
    keep = torch.ones(n, dtype=torch.bool, device="cuda")
    keep[perm] = False
    t_remove, t_fresh, t_fresh_held = [], [], []
    for rep in range(reps):
        ix = FlatIndex(dim, "COSINE", 0)
        ix.add(rows_dev, ids)
        dt, removed = timed(lambda: ix.remove(perm))
        t_remove.append(dt)
        assert removed == perm.numel()
        check_ids = ix.rows(0, 1000)[1]
        del ix
        # what a user does today: read the survivors out of the index, build a fresh one from them
        old = FlatIndex(dim, "COSINE", 0)
        old.add(rows_dev, ids)

        def rebuild():
            r, i = old.rows()
            fresh = FlatIndex(dim, "COSINE", 0)
            fresh.add(r[keep], i[keep])
            return fresh
        dt, fresh = timed(rebuild)
        t_fresh.append(dt)
        assert torch.equal(fresh.rows(0, 1000)[1], check_ids)
        del fresh, old

        def rebuild_held():                                   # the best case: the survivors already sit in a device tensor
            fresh = FlatIndex(dim, "COSINE", 0)
            fresh.add(held, held_ids)
            return fresh
        held, held_ids = rows_dev[keep], ids[keep]
        dt, fresh = timed(rebuild_held)
        t_fresh_held.append(dt)
        del fresh, held, held_ids
    tag = f"{frac * 100:.0f} % of {n} x {dim}"
    spread(f"remove {tag}", t_remove)
    spread(f"fresh index from rows() of the old one, {tag}", t_fresh)
    spread(f"fresh index from survivors held on the device, {tag}", t_fresh_held)
    # a plain device copy of the bytes the moves carry once: survivors x dimp x (4 + 2) bytes
    dimp = (dim + 127) // 128 * 128
    nbytes = int(keep.sum()) * dimp * 6
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t_copy = [timed(lambda: dst.copy_(src))[0] for _ in range(reps + 1)][1:]
    spread(f"plain device copy of {nbytes / 2 ** 30:.2f} GiB (the moves carry it twice: gather, place)", t_copy,
           f"= {nbytes * 2 / min(t_copy) / 1e12:.2f} TB/s read + written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the temporary store goes (default: the system's temporary directory)")
    ap.add_argument("--remove-only", action="store_true", help="one removal of 1 %% and one of 50 %%, for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_store.py measures on a GPU; none is visible")
    g = torch.Generator().manual_seed(1)
    rows = torch.nn.functional.normalize(torch.randn(args.rows, args.dim, generator=g), dim=1)
    rows_dev = rows.to("cuda")
    if not args.remove_only:
        bench_load(args, rows.numpy())
    for frac in (0.01, 0.5):
        bench_remove(args, rows_dev, frac, 1 if args.remove_only else args.reps)


if __name__ == "__main__":
    main()
