"""ConvNeXtV2_SRA embedding throughput at 384 x 384 on one GPU: the native path (backbone rows + the k_attnpool.hip head), the plain
ConvNeXtV2 native path on the same backbone weights, and, in the same process on the same GPU, the torch-eager fp32 forward of the
same ConvNeXtV2_SRA module (library convolutions, GEMMs, softmax, bmm, layer_norm) as the comparison.

    python tools/bench_sra.py [--batches 1,64,256] [--steps 5] [--warmup 2] [--no-eager] [--sra-only] [--out profiles/<name>.json]

Prints one JSON line per (path, batch): img/s from CUDA events over `steps` forwards after `warmup`, and for the SRA native path
its ratio to ConvNeXtV2 native at the same batch.  Weights are random with non-trivial LayerNorm affines, GRN parameters and head
weights (tests/_sra_ref.randomize)."""
import argparse
import json
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


def _eager(m, x):
    # grad mode with no parameter requiring grad: every block takes its torch graph and no autograd state is kept
    with torch.enable_grad():
        return m(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--sra-only", action="store_true", help="the SRA native path alone (for a kernel trace of its forward)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.model import ConvNeXtV2, ConvNeXtV2_SRA
    from _sra_ref import randomize
    torch.manual_seed(0)
    sra = randomize(ConvNeXtV2_SRA(num_heads=a.heads), seed=1).eval().cuda().requires_grad_(False)
    base = ConvNeXtV2().eval().cuda().requires_grad_(False)
    base.load_state_dict({k: v for k, v in sra.state_dict().items() if k.startswith("convnext.")}, strict=True)
    rows = []
    for bs in [int(v) for v in a.batches.split(",")]:
        x = torch.randn(bs, 3, 384, 384, device="cuda")
        runs = [("sra_native_fp32", lambda: sra(x))]
        if not a.sra_only:
            runs.append(("convnextv2_native_fp32", lambda: base(x)))
        if not (a.no_eager or a.sra_only):
            runs.append(("sra_eager_fp32", lambda: _eager(sra, x)))
        rate = {}
        with torch.no_grad():
            for name, fn in runs:
                sec = _time(fn, a.steps, a.warmup)
                rate[name] = bs / sec
                r = {"path": name, "batch": bs, "img_per_s": round(bs / sec, 1), "ms_per_step": round(sec * 1e3, 3),
                     "steps": a.steps, "device": torch.cuda.get_device_name(0)}
                if name == "sra_native_fp32":
                    r["heads"] = a.heads
                if name == "convnextv2_native_fp32":
                    r["sra_over_convnextv2"] = round(rate["sra_native_fp32"] / rate[name], 4)
                rows.append(r)
                print(json.dumps(r), flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
