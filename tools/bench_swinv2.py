"""SwinV2-B embedding throughput at 384 x 384 on one GPU: the native path and, in the same process on the same GPU, the
torch-eager fp32 forward of the same module (library GEMMs, softmax, roll and copies) as the comparison.

    python tools/bench_swinv2.py [--batches 1,64,256] [--steps 5] [--warmup 2] [--out profiles/<name>.json]
    python tools/bench_swinv2.py --bound-bits          (what the host-side input bounds cost, per residual-stream Linear)

Prints one JSON line per (path, batch): img/s from CUDA events over `steps` forwards after `warmup`.  Weights are random with
non-trivial LayerNorm affines and logit scales (tests/_swinv2_ref.randomize)."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    return a.elapsed_time(b) / 1000.0 / steps


def bound_bits(m, n=4):
    """Per block: log2(bound / max |x|) of the inputs of the Linears whose terms scale comes from a host-side bound -- qkv and
    fc1 (the residual stream), proj (attention output), fc2 (GELU output) and each stage's reduction (the merged stream),
    measured on the eager fp32 forward of n random images.  Two fp16 terms keep ~22 bits relative to each value whatever the
    scale; a loose bound only moves small values toward the low term's subnormal floor."""
    from mirx.model import _SwinPatchMerging
    seen = {}
    hooks = []

    def grab(key):
        def h(mod, args, out=None):
            seen[key] = max(seen.get(key, 0.0), float(args[0].abs().max()))
        return h
    bb = m.swinv2
    for si, stage in enumerate(bb.layers):
        if isinstance(stage.downsample, _SwinPatchMerging):
            hooks.append(stage.downsample.reduction.register_forward_hook(grab((si, "reduction"))))
        for j, blk in enumerate(stage.blocks):
            hooks.append(blk.attn.register_forward_pre_hook(grab((si, j, "qkv"))))      # (the qkv weight is applied by F.linear)
            hooks.append(blk.attn.proj.register_forward_hook(grab((si, j, "proj"))))
            hooks.append(blk.mlp.fc1.register_forward_hook(grab((si, j, "fc1"))))
            hooks.append(blk.mlp.fc2.register_forward_hook(grab((si, j, "fc2"))))
    x = torch.randn(n, 3, 384, 384, device="cuda")
    with torch.no_grad():
        m.forward_eager(x)
        cache = m._cache()
    for h in hooks:
        h.remove()
    rows = []
    for si, (stage, sc) in enumerate(zip(bb.layers, cache["stages"])):
        if (si, "reduction") in seen:
            rows.append({"stage": si, "linear": "reduction", "bits": round(math.log2(sc["r_in"] / seen[(si, "reduction")]), 2)})
        for j, e in enumerate(sc["blocks"]):
            for name, bound in (("qkv", e["r_qkv"]), ("proj", e["b_att"]), ("fc1", e["r_fc1"]), ("fc2", e["b_hid"])):
                rows.append({"stage": si, "block": j, "linear": name, "bits": round(math.log2(bound / seen[(si, j, name)]), 2)})
    allv = [r["bits"] for r in rows]
    return {"per_linear": rows, "max_bits": max(allv), "mean_bits": round(sum(allv) / len(allv), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bound-bits", action="store_true")
    a = ap.parse_args()
    from mirx.model import SwinV2
    from _swinv2_ref import randomize
    torch.manual_seed(0)
    m = randomize(SwinV2(), seed=1).eval().cuda()
    if a.bound_bits:
        r = bound_bits(m)
        print(json.dumps({k: v for k, v in r.items() if k != "per_linear"}))
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(r, fh, indent=1)
        return
    rows = []
    for bs in [int(v) for v in a.batches.split(",")]:
        x = torch.randn(bs, 3, 384, 384, device="cuda")
        with torch.no_grad():
            runs = [("native_fp32", lambda: m(x))]
            if not a.no_eager:
                runs.append(("eager_fp32", lambda: torch.nn.functional.normalize(m.forward_eager(x), dim=1)))
            for name, fn in runs:
                sec = _time(fn, a.steps, a.warmup)
                r = {"path": name, "batch": bs, "img_per_s": round(bs / sec, 1), "ms_per_step": round(sec * 1e3, 3),
                     "steps": a.steps, "device": torch.cuda.get_device_name(0)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
