"""ResNet50 embedding throughput at 224 x 224 on one GPU: the native path (fp32 and uint8 input) and, in the same process on
the same GPU, the torch-eager fp32 forward of the same module (library convolutions) as the comparison.

    python tools/bench_resnet.py [--batches 1,64,256,1024] [--steps 10] [--warmup 3] [--out profiles/<name>.json]
    python tools/bench_resnet.py --bound-bits          (what the terms outputs' a-priori bounds cost, per convolution)

Prints one JSON line per (path, batch): img/s from CUDA events over `steps` forwards after `warmup`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def bound_bits(m, n=8):
    """Per convolution: log2(bound_b / max |y_b|) over n images -- the bits of the 22 that the scale of a terms output gives
    away because it is fixed from a bound before the launch (mirx_conv_terms) rather than from the values written."""
    x = torch.randn(n, 3, 224, 224, device="cuda")
    with torch.no_grad():
        m(x)
    r = m.__dict__["_mirx_last_ranges"].double().cpu()
    blocks = m._cache()["blocks"]
    rows, xin = [], r[1]
    for i, e in enumerate(blocks):
        b = 2 + 4 * i
        def bits(cw, xr, yr, rr=None):
            bound = xr * cw["wsum"] + cw["bmax"] + (rr if rr is not None else 0.0)
            return [round(v, 2) for v in torch.log2(bound / yr).tolist()]
        rows.append({"block": i, "conv1": bits(e["conv1"], xin, r[b]), "conv2": bits(e["conv2"], r[b], r[b + 1])})
        res = r[b + 2] if "down" in e else xin
        if "down" in e:
            rows[-1]["down"] = bits(e["down"], xin, r[b + 2])
        rows[-1]["conv3"] = bits(e["conv3"], r[b + 1], r[b + 3], res)
        xin = r[b + 3]
    allv = [v for row in rows for k, vs in row.items() if k != "block" for v in vs]
    return {"per_block": rows, "max_bits": max(allv), "mean_bits": sum(allv) / len(allv)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256,1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bound-bits", action="store_true")
    a = ap.parse_args()
    from mirx.model import ResNet50
    from oracle.densenet import randomize_bn_stats
    torch.manual_seed(0)
    m = ResNet50()
    m.load_state_dict(randomize_bn_stats(m.state_dict(), seed=1))
    m = m.eval().cuda()
    if a.bound_bits:
        r = bound_bits(m)
        print(json.dumps(r))
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(r, fh, indent=1)
        return
    rows = []
    for bs in [int(v) for v in a.batches.split(",")]:
        x = torch.randn(bs, 3, 224, 224, device="cuda")
        u = torch.randint(0, 256, (bs, 3, 224, 224), dtype=torch.uint8, device="cuda")
        with torch.no_grad():
            runs = [("native_fp32", lambda: m(x)), ("native_uint8", lambda: m(u))]
            if not a.no_eager:
                runs.append(("eager_fp32", lambda: torch.nn.functional.normalize(m.forward_eager(x), dim=1)))
            for name, fn in runs:
                sec = _time(fn, a.steps, a.warmup)
                r = {"path": name, "batch": bs, "img_per_s": round(bs / sec, 1), "ms_per_step": round(sec * 1e3, 3),
                     "steps": a.steps, "device": torch.cuda.get_device_name(0)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        del x, u
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
