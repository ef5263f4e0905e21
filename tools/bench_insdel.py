"""Insertion / deletion curves on one GPU: a seeded mirx DenseNet121 at 224 x 224, one query against K hits, both modes.

    python tools/bench_insdel.py [--steps 10] [--warmup 2] [--shapes 1000:1,1000:5,1000:10,224:1,224:20] [--max-batch 1024]
                                 [--kernels-only] [--out profiles/<name>.txt]

Per shape (step:K; step 1000 = 52 images per curve, step 224 = 225), in one process:
  ms_native        mirx.xai.insdel_curves (all 2K curves as one job)
  ms_parent_loop   2K calls of mirx.xai.CausalMetric.evaluate with its conv2d blur: the per-(pair, mode) path this replaces
  ms_forward_floor the bare forward of as many random images in the same max_batch chunks (+ the query's): what no glue can beat
  ms_stage_*       the native job's stages alone: steps (sort), blur, compose of all images, curves (scoring)
Times are CUDA-event means over `steps` calls after `warmup` calls; the native call and the floor are measured three times
(median, `spread` = (max - min) / median of the three), the parent loop once with steps / 2 (at least 2).  One JSON line per
shape.  --kernels-only runs the native calls alone (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

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


def _time3(fn, steps, warmup):
    """(median of three windows, (max - min) / median)"""
    t = sorted(_time(fn, steps, warmup) for _ in range(3))
    return round(t[1], 4), round((t[2] - t[0]) / t[1], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="1000:1,1000:5,1000:10,224:1,224:20")
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mirx.insdel as I
    from mirx.model import DenseNet121
    from mirx.xai import CausalMetric, gkern, insdel_curves
    assert torch.cuda.is_available(), "bench_insdel needs a GPU"
    dev = torch.device("cuda:0")
    size, hw = 224, 224 * 224
    torch.manual_seed(0)
    model = DenseNet121().eval().to(dev)
    g = torch.Generator().manual_seed(1)
    kmax = max(int(s.split(":")[1]) for s in a.shapes.split(","))
    xq = torch.randn(1, 3, size, size, generator=g).to(dev)
    xr = torch.randn(kmax, 3, size, size, generator=g).to(dev)
    sal = torch.relu(torch.randn(kmax, size, size, generator=g)).to(dev)          # ReLU'd maps: half the pixels tied at 0
    sal_host = sal.cpu().numpy()
    kern = gkern(51, math.sqrt(50)).to(dev)
    conv_blur = lambda x: F.conv2d(x, kern, padding=25)                          # noqa: E731
    blur = I.GaussianBlur(51, math.sqrt(50))
    subs = {"del": torch.zeros_like, "ins": blur}
    res = []
    for shape in a.shapes.split(","):
        step, k = (int(v) for v in shape.split(":"))
        n_steps = math.ceil(hw / step)
        total = 2 * k * (n_steps + 1)
        native = lambda: insdel_curves(model, xq, xr[:k], sal[:k], step, substrates=subs, max_batch=a.max_batch)   # noqa: E731
        assert native().last_native
        d = {"step": step, "K": k, "images": total, "max_batch": a.max_batch}
        d["ms_native"], d["spread_native"] = _time3(native, a.steps, a.warmup)
        if not a.kernels_only:
            def parent():
                for i in range(k):
                    CausalMetric(model, "del", step, torch.zeros_like, input_size=size).evaluate(xq, xr[i:i + 1], sal_host[i])
                    CausalMetric(model, "ins", step, conv_blur, input_size=size).evaluate(xq, xr[i:i + 1], sal_host[i])
            d["ms_parent_loop"] = round(_time(parent, max(2, a.steps // 2), 1), 4)
            rnd = torch.randn(min(a.max_batch, total), 3, size, size, device=dev)

            def floor():
                with torch.no_grad():
                    model(xq)
                    for lo in range(0, total, a.max_batch):
                        model(rnd[:min(a.max_batch, total - lo)])
            d["ms_forward_floor"], d["spread_forward_floor"] = _time3(floor, a.steps, a.warmup)
            t = I.insdel_steps(sal[:k].reshape(k, hw), step)
            bank = torch.cat([xr[:k], blur(xr[:k])]).reshape(2 * k, 3, hw)
            idx = torch.arange(k, dtype=torch.int32, device=dev)
            start = torch.stack([idx, idx + k], 1).reshape(-1).contiguous()
            finish = torch.stack([torch.full_like(idx, -1), idx], 1).reshape(-1).contiguous()
            row = idx.repeat_interleave(2).contiguous()
            buf = torch.empty((min(a.max_batch, total), 3, hw), device=dev)

            def compose():
                for lo in range(0, total, a.max_batch):
                    n = min(a.max_batch, total - lo)
                    I.insdel_compose(t, bank, start, finish, row, n_steps, lo, n, out=buf[:n])
            feats = F.normalize(torch.randn(total, 1024, device=dev), dim=1)
            qf = feats[:1].clone()
            d["ms_stage_steps"] = round(_time(lambda: I.insdel_steps(sal[:k].reshape(k, hw), step), 10 * a.steps, a.warmup), 4)
            d["ms_stage_blur"] = round(_time(lambda: blur(xr[:k]), 10 * a.steps, a.warmup), 4)
            d["ms_stage_blur_conv2d"] = round(_time(lambda: conv_blur(xr[:k]), 10 * a.steps, a.warmup), 4)
            d["ms_stage_compose"] = round(_time(compose, 10 * a.steps, a.warmup), 4)
            d["ms_stage_curves"] = round(_time(lambda: I.insdel_scores(qf, feats, 2 * k, n_steps), 10 * a.steps, a.warmup), 4)
            d["native_over_parent"] = round(d["ms_native"] / d["ms_parent_loop"], 4)
            d["share_above_floor"] = round((d["ms_native"] - d["ms_forward_floor"]) / d["ms_native"], 4)
            del rnd, buf, bank, feats
        print(json.dumps(d), flush=True)
        res.append(d)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(f"# tools/bench_insdel.py on {torch.cuda.get_device_name(0)}: steps {a.steps}, warmup {a.warmup}; ms per call\n")
            for d in res:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
