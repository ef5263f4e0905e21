"""SimCAM saliency on one GPU: the four configurations of the reference's drivers at their sizes (DenseNet121 224, ResNet50 224,
ConvNeXtV2 384, MedSigLIP 448; seeded weights), per explainer call at (1 query, 1 retrieved) and (1, 5), split into the
feature forward (the native tap alone) and the rest; same-process baselines on the same native features: the reference's
formulas in torch (matmul, amax, clamp, sum, interpolate) and, for DenseNet, its per-position loop; and mirx_simcam alone at
MedSigLIP geometry with P = 64 against the 157.3 TF f32 matrix peak.

    python tools/bench_simcam.py [--steps 10] [--warmup 3] [--configs densenet,resnet,convnext,medsiglip] [--out profiles/<name>.json]

Times are CUDA-event means over `steps` calls after `warmup` calls; one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_PEAK_TF = 157.3


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


def _torch_formulas(q, r, h, w, H, W, eps, maps):
    """explanations.py SimCAM / SimCAM_MedSigLIP after the hook, on rows q [1, hw, C], r [K, hw, C]."""
    D = torch.matmul(q.expand(r.shape[0], -1, -1), r.transpose(1, 2))
    D = (D / (D.amax(dim=(1, 2), keepdim=True) + eps)).clamp(min=0).view(r.shape[0], h, w, h, w)
    if maps == "retrieved":
        return F.interpolate(D.sum(dim=(1, 2)).unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False)
    return F.interpolate(torch.stack((D.sum(dim=(3, 4)), D.sum(dim=(1, 2))), dim=1), size=(H, W), mode="bilinear",
                         align_corners=False)


def _loop_formula(x, H, W):
    """explanations.py SimCAM_Densenet121's decomposition: one torch.sum per (i, j, k, l)."""
    hh, ww = x.shape[1], x.shape[2]
    D = torch.zeros([hh, ww, hh, ww], device=x.device)
    for i in range(hh):
        for j in range(ww):
            for k in range(hh):
                for l in range(ww):  # noqa: E741
                    D[i, j, k, l] = torch.sum(x[0, i, j] * x[1, k, l])
    D = (D / torch.max(D)).clamp(min=0)
    return F.interpolate(torch.stack((D.sum(dim=(2, 3)), D.sum(dim=(0, 1)))).unsqueeze(1), size=(H, W), mode="bilinear")


def _config(name, dev):
    from mirx import model as M
    from mirx.simcam import SimCAM, SimCAM_Densenet121, SimCAM_MedSigLIP
    torch.manual_seed(0)
    if name == "densenet":
        m = M.DenseNet121().eval().to(dev)
        seq = nn.Sequential(*list(m.children())[0], *list(m.children())[1:])
        ex = SimCAM_Densenet121(seq, seq[0], target_layers=["relu"]).eval()
        tap = lambda x: m._relu_rows(x[:2], m._cache())                         # noqa: E731
        return ex, tap, 224, 0.0, "dense"
    if name == "resnet":
        m = M.ResNet50().eval().to(dev)
        return SimCAM(m, m.resnet50[7][2]), lambda x: m._layer4_rows(x, m._cache()), 224, 1e-8, "both"
    if name == "convnext":
        m = M.ConvNeXtV2().eval().to(dev)
        b = m.convnext

        def tap(x):
            t, h, w = b._forward_rows(x)
            return t.view(x.shape[0], h * w, -1), h, w
        return SimCAM(b, b.stages[3].blocks[2]), tap, 384, 1e-8, "both"
    m = M.MedSigLIP().eval().to(dev)

    def tap(x):
        t = m.backbone.last_hidden_state(x)
        return t, 32, 32
    return SimCAM_MedSigLIP(m, m.backbone.post_layernorm), tap, 448, 1e-8, "retrieved"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="densenet,resnet,convnext,medsiglip")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.simcam import simcam_maps
    dev = torch.device("cuda:0")
    res = []

    def emit(d):
        print(json.dumps(d), flush=True)
        res.append(d)

    with torch.no_grad():
        for name in filter(None, a.configs.split(",")):
            ex, tap, size, eps, maps = _config(name, dev)
            for nr in (1, 5):
                g = torch.Generator().manual_seed(nr)
                xq = torch.randn(1, 3, size, size, generator=g).to(dev)
                x = torch.randn(nr, 3, size, size, generator=g).to(dev)
                xa = torch.cat([xq, x])
                ex(xq, x)
                assert ex.last_native, name
                t_call = _time(lambda: ex(xq, x), a.steps, a.warmup)
                t_fwd = _time(lambda: tap(xa), a.steps, a.warmup)
                rows, h, w = tap(xa)
                q, r = (rows[0], rows[1:2]) if maps == "dense" else (rows[0], rows[1:])
                km = "both" if maps == "dense" else maps
                t_kern = _time(lambda: simcam_maps(q, r, h, w, (size, size), eps, km), a.steps, a.warmup)
                t_torch = _time(lambda: _torch_formulas(q[None], r, h, w, size, size, eps if eps else 1e-8, km), a.steps, a.warmup)
                d = {"config": name, "size": size, "queries": 1, "retrieved": nr, "hw": h * w, "C": int(rows.shape[-1]),
                     "ms_per_call": round(t_call, 4), "ms_tap_forward": round(t_fwd, 4), "ms_simcam_maps": round(t_kern, 4),
                     "ms_torch_formulas_on_native_features": round(t_torch, 4)}
                if maps == "dense":
                    img = rows.view(rows.shape[0], h, w, -1)
                    d["ms_reference_loop_formula"] = round(_time(lambda: _loop_formula(img, size, size), 1, 1), 2)
                emit(d)
            del ex, tap
            torch.cuda.empty_cache()
        # the pairs kernel alone at MedSigLIP geometry, P = 64
        g = torch.Generator().manual_seed(7)
        q = torch.randn(1024, 1152, generator=g).to(dev)
        r = torch.randn(64, 1024, 1152, generator=g).to(dev)
        out = torch.empty(64, 448, 448, device=dev)
        t = _time(lambda: simcam_maps(q, r, 32, 32, (448, 448), 1e-8, "retrieved", out=out), a.steps, a.warmup)
        # a 1 x 1 output makes k_simcam_maps negligible: the call is then k_simcam_pairs
        out1 = torch.empty(64, 1, 1, device=dev)
        t_pairs = _time(lambda: simcam_maps(q, r, 32, 32, (1, 1), 1e-8, "retrieved", out=out1), a.steps, a.warmup)
        t_torch = _time(lambda: _torch_formulas(q[None], r, 32, 32, 448, 448, 1e-8, "retrieved"), a.steps, a.warmup)
        flop = 64 * 2.0 * 1024 * 1024 * 1152
        emit({"config": "medsiglip_pairs_p64", "hw": 1024, "C": 1152, "P": 64, "ms_simcam_maps": round(t, 4),
              "ms_pairs_only": round(t_pairs, 4), "tflops_pairs": round(flop / t_pairs / 1e9, 2),
              "share_of_f32_peak_pairs": round(flop / t_pairs / 1e9 / F32_PEAK_TF, 4),
              "tflops_whole_call": round(flop / t / 1e9, 2), "ms_torch_formulas": round(t_torch, 4)})
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "results": res}, fh, indent=1)


if __name__ == "__main__":
    main()
