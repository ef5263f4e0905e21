"""MedSigLIP Grad-CAM on one GPU: mirx.xai.compute_gradcam_saliency on a seeded MedSigLIP at 448 x 448 (N = 1024, 27 layers,
16 heads, head_dim 72) at (1 query, K retrieved) for K = 1, 5 (the driver's default top_k) and 8, native against the torch
formulas (autograd through the tower, one image at a time, as the reference's second pass) on the same model in the same
process.  Also the native call split into the retrieved forward (the tower alone) and the Grad-CAM kernels on its tokens.

    python tools/bench_gradcam.py [--steps 5] [--warmup 2] [--retrieved 1,5,8] [--out profiles/<name>.json]

Times are CUDA-event means over `steps` calls after `warmup` calls; one JSON line per measurement."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--retrieved", default="1,5,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx import siglip_gradcam as G
    from mirx import xai
    from mirx.model import MedSigLIP

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = MedSigLIP().to(dev).eval()
    rows = []
    for k in [int(v) for v in a.retrieved.split(",")]:
        img = torch.randn((k + 1, 3, 448, 448), generator=torch.Generator().manual_seed(k)).to(dev)
        q, r = img[:1], img[1:].contiguous()
        native = _time(lambda: xai.compute_gradcam_saliency(m, q, r, dev), a.steps, a.warmup)
        assert xai.compute_gradcam_saliency.last_native
        with torch.no_grad():
            qemb = m(q)
            fwd = _time(lambda: m.backbone._last_layer_tokens(r), a.steps, a.warmup)
            x = m.backbone._last_layer_tokens(r)
            kern = _time(lambda: G.gradcam_from_tokens(m, qemb, x, (448, 448)), a.steps, a.warmup)
        torch_ms = _time(lambda: [G._single_torch(m, qemb, r[i:i + 1]) for i in range(k)], max(1, a.steps // 2), 1)
        row = dict(bench="gradcam", retrieved=k, queries=1, size=448, native_ms=round(native, 3), torch_ms=round(torch_ms, 3),
                   speedup=round(torch_ms / native, 2), retrieved_forward_ms=round(fwd, 3), gradcam_kernels_ms=round(kern, 3),
                   kernel_share=round(kern / native, 4), steps=a.steps, warmup=a.warmup,
                   device=torch.cuda.get_device_name(dev))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
