"""Device-side Resize / CenterCrop against the host path, on one GPU, in one process.

    python tools/bench_preprocess.py [--rows 200000] [--window 0.3] [--windows 3] [--only all|base|forms] [--out profiles/<name>.txt]

The device path is default_transform as it is (tf.batch_pixels / tf.batch: mirx.preprocess, mirx_resample_batch).  The host path
is the same transform with its batch attributes removed, which sends every call site down the code it had before they existed
(tf.pixels / tf in Pillow, one image at a time).  Every shape is warmed on both paths first; then the two paths alternate, one
window of at least `window` seconds each, `windows` windows per path; a window's figure is its wall time per call (each call
ends with its results on the host, so the device is idle at both ends).  Reported per case: the median over the windows and
the spread (max - min) / median of either path.

  search            MilvusRetriever.search(PIL image), seeded DenseNet121, `rows` gallery rows, top-10; sources 300 x 280 RGB
                    (bench.py's image), 1024 x 1024 L, 2048 x 2500 L, 1024 x 1024 RGB
  batch_search      64 images per call, 300 x 280 RGB and 1024 x 1024 L
  encode_npy_paths  one chunk of 64 .npy files of 1024 x 1024 through the ConvNeXtV2 NIH model at 384 (resize 432)
  kernel, copy      per source and for the 64-image batches: the launch alone and the host-to-device copy alone, each between
                    device events (median of 20 after 3 warm-up runs)
  forms the square stretch and BICUBIC, same model and gallery, each transform against itself without its batch
                    attributes: search 300 x 280 RGB stretched to 224; search 1024 x 1024 L, bicubic 480 -> 448; search
                    2048 x 2500 L, bicubic stretch to 384; batch_search of 64 x 1024 x 1024 L, bicubic stretch to 384
One JSON line per case; --out also writes everything to a file."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _image(w, h, mode, seed):
    from PIL import Image
    shape = (h, w, 3) if mode == "RGB" else (h, w)
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def _host_only(tf):
    """The transform without its batch attributes: the call sites' earlier code."""
    del tf.batch, tf.batch_pixels, tf.last_preprocess
    return tf


def _window(fn, seconds):
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while True:
        fn()
        calls += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def _ab(name, dev_fn, host_fn, args, extra=None):
    for _ in range(2):
        dev_fn()
        host_fn()
    d, h = [], []
    for _ in range(args.windows):
        d.append(_window(dev_fn, args.window))
        h.append(_window(host_fn, args.window))
    md, mh = statistics.median(d), statistics.median(h)
    rec = {"case": name, "device_ms": round(md, 4), "host_ms": round(mh, 4), "host_over_device": round(mh / md, 3),
           "device_spread": round((max(d) - min(d)) / md, 3), "host_spread": round((max(h) - min(h)) / mh, 3),
           "device_windows_ms": [round(v, 4) for v in d], "host_windows_ms": [round(v, 4) for v in h]}
    rec.update(extra or {})
    return rec


def _events(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def kernel_and_copy(name, images, resize, size, f32, interpolation="bilinear"):
    """The launch alone and the copy alone for one packed batch."""
    from mirx import _lib as L
    from mirx import preprocess as P
    from mirx.retriever import IMAGENET_MEAN, IMAGENET_STD
    import ctypes
    items = [(im, P.plan(im.size[0], im.size[1], resize, size, interpolation)) for im in images]
    tables, layout, nbytes = P.blob_layout(items)
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    P.blob_fill(pinned.numpy(), items, tables, layout)
    gpu = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty((len(images), 3, size, size), dtype=torch.float32 if f32 else torch.uint8, device="cuda")
    mean, std = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        L.check(lib.mirx_resample_batch(pinned.data_ptr(), gpu.data_ptr(), nbytes, len(images), size,
                                        L.RESAMPLE_OUT_F32 if f32 else L.RESAMPLE_OUT_U8, mean, std, out.data_ptr(), stream))

    t_copy = _events(lambda: gpu.copy_(pinned, non_blocking=True))
    t_kernel = _events(launch)
    t0 = time.perf_counter()
    for _ in range(5):
        P.blob_fill(pinned.numpy(), items, tables, layout)
    t_pack = (time.perf_counter() - t0) / 5 * 1e3
    return {"case": name, "images": len(images), "bytes": nbytes, "form": "fp32" if f32 else "uint8", "kernel_ms": round(t_kernel, 4),
            "copy_ms": round(t_copy, 4), "host_pack_ms": round(t_pack, 4)}


def forms(args, emit, mgr, model):
    """The rows of DESIGN 30: each new shape on the device path against the same transform on the host path."""
    from mirx.retriever import MilvusRetriever, default_transform
    cases = [("search 300x280 RGB, stretch to 224", _image(300, 280, "RGB", 0), 1, dict(img_size=224, resize=(224, 224))),
             ("search 1024x1024 L, bicubic 480 -> 448", _image(1024, 1024, "L", 1), 1,
              dict(img_size=448, resize=480, interpolation="bicubic")),
             ("search 2048x2500 L, bicubic stretch to 384", _image(2048, 2500, "L", 2), 1,
              dict(img_size=384, resize=(384, 384), interpolation="bicubic")),
             ("batch_search 64 x 1024x1024 L, bicubic stretch to 384", _image(1024, 1024, "L", 1), 64,
              dict(img_size=384, resize=(384, 384), interpolation="bicubic"))]
    for name, img, count, kw in cases:
        r_dev = MilvusRetriever(mgr, "densenet121", model, default_transform(**kw))
        r_host = MilvusRetriever(mgr, "densenet121", model, _host_only(default_transform(**kw)))
        r_dev.load_collection()
        r_host.load_collection()
        if count == 1:
            a, qa = r_dev.search(img, top_k=10)
            b, qb = r_host.search(img, top_k=10)
            assert a == b and torch.equal(qa, qb), name
            dev_fn, host_fn = (lambda: r_dev.search(img, top_k=10)), (lambda: r_host.search(img, top_k=10))
        else:
            batch = [img] * count
            assert r_dev.batch_search(batch, top_k=10) == r_host.batch_search(batch, top_k=10), name
            dev_fn, host_fn = (lambda: r_dev.batch_search(batch, top_k=10)), (lambda: r_host.batch_search(batch, top_k=10))
        assert r_dev.last_preprocess == {"device": count, "host": 0}, name
        emit(_ab(name, dev_fn, host_fn, args))
        emit(kernel_and_copy("kernel " + name.split(" ", 1)[1], [img] * count, kw["resize"], kw["img_size"], count > 1,
                             kw.get("interpolation", "bilinear")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--only", choices=("all", "base", "forms"), default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from mirx import nih
    from mirx.model import DenseNet121
    from mirx.retriever import MilvusManager, MilvusRetriever, default_transform
    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def finish():
        if args.out:
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit({"device": torch.cuda.get_device_name(0), "rows": args.rows, "window_s": args.window, "windows": args.windows,
          "only": args.only})
    torch.manual_seed(0)
    model = DenseNet121().eval().to(dev)
    mgr = MilvusManager(device=0)
    mgr.connect()
    mgr.create_collection("densenet121", drop_old=True)
    col = mgr.collections["densenet121"]
    g = torch.Generator(device=dev).manual_seed(7)
    for s0 in range(0, args.rows, 50_000):
        n = min(50_000, args.rows - s0)
        emb = torch.nn.functional.normalize(torch.randn((n, 1024), generator=g, device=dev), dim=1)
        col.insert([[f"img_{s0 + i}.png" for i in range(n)], ["normal"] * n, emb])
    if args.only in ("all", "forms"):
        forms(args, emit, mgr, model)
    if args.only == "forms":
        return finish()
    r_dev = MilvusRetriever(mgr, "densenet121", model, default_transform(224))
    r_host = MilvusRetriever(mgr, "densenet121", model, _host_only(default_transform(224)))
    r_dev.load_collection()
    r_host.load_collection()

    sources = [("300x280 RGB", _image(300, 280, "RGB", 0)), ("1024x1024 L", _image(1024, 1024, "L", 1)),
               ("2048x2500 L", _image(2048, 2500, "L", 2)), ("1024x1024 RGB", _image(1024, 1024, "RGB", 3))]
    for name, img in sources:
        a, qa = r_dev.search(img, top_k=10)
        assert r_dev.last_preprocess == {"device": 1, "host": 0}
        b, qb = r_host.search(img, top_k=10)
        assert a == b and torch.equal(qa, qb), name
        emit(_ab(f"search {name}", lambda: r_dev.search(img, top_k=10), lambda: r_host.search(img, top_k=10), args))
        emit(kernel_and_copy(f"kernel {name}", [img], 256, 224, False))
    for name, img in (sources[0], sources[1]):
        batch = [img] * 64
        assert r_dev.batch_search(batch, top_k=10) == r_host.batch_search(batch, top_k=10)
        emit(_ab(f"batch_search 64 x {name}", lambda: r_dev.batch_search(batch, top_k=10),
                 lambda: r_host.batch_search(batch, top_k=10), args))
        emit(kernel_and_copy(f"kernel 64 x {name}", batch, 256, 224, True))
    del r_dev, r_host, model, col
    mgr.disconnect()
    torch.cuda.empty_cache()

    spec = nih.BACKBONE_SPECS["convnextv2"]
    torch.manual_seed(1)
    nmodel = spec.model_builder(14, spec.default_backbone_name, False).eval().to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(5)
        paths = []
        for i in range(64):
            p = os.path.join(tmp, f"{i:05d}_Chest_X-ray_Mass_{i}.npy")
            np.save(p, rng.integers(0, 256, (1024, 1024), dtype=np.uint8))
            paths.append(p)
        tf_dev, tf_host = nih.build_nih_val_transform(384, 432), _host_only(nih.build_nih_val_transform(384, 432))
        a = nih.encode_npy_paths(nmodel, tf_dev, paths, dev, 64)
        b = nih.encode_npy_paths(nmodel, tf_host, paths, dev, 64)
        assert all(np.array_equal(x["embedding"], y["embedding"]) for x, y in zip(a, b))
        emit(_ab("encode_npy_paths 64 x 1024x1024 .npy, ConvNeXtV2 NIH 384", lambda: nih.encode_npy_paths(nmodel, tf_dev, paths, dev, 64),
                 lambda: nih.encode_npy_paths(nmodel, tf_host, paths, dev, 64), args))
        imgs = [nih.load_npy_as_pil(p) for p in paths]
        emit(kernel_and_copy("kernel 64 x 1024x1024 L -> 384", imgs, 432, 384, True))
        t0 = time.perf_counter()
        for p in paths:
            nih.load_npy_as_pil(p)
        emit({"case": "load_npy_as_pil 64 files (both paths pay it)", "ms": round((time.perf_counter() - t0) * 1e3, 3)})
    finish()


if __name__ == "__main__":
    main()
