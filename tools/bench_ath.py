"""ATH throughput on one GPU: ATHNet at 256 x 256 (native fp32 against the torch-eager fp32 forward of the same module, in the same
process), and the exact Hamming top-k (mirx.ath.hamming_topk) against a chunked torch baseline (`!=`-sum distances + topk) in the
same process.

    python tools/bench_ath.py [--batches 1,64,1024] [--steps 5] [--warmup 2] [--no-eager] [--no-hamming] [--no-model]
                              [--searches 1:1048576:36:10,4096:1048576:36:10,...] [--out profiles/<name>.json]

Prints one JSON line per measurement: img/s (model) or queries/s (search) from CUDA events over `steps` runs after `warmup`.  The
search includes packing the 0/1 query and gallery tensors (what a caller of hamming_topk pays).  The baseline is checked against
the native ranking on its distances (its tie order is torch.topk's, so only the distances are compared)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEARCHES = "1:1048576:36:10,4096:1048576:36:10,4096:1048576:64:10,4096:1048576:256:100"


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
    with torch.enable_grad():          # grad mode with no parameter requiring grad: the torch graph, no autograd state
        return m(x)


def _torch_hamming(q, g, k, chunk_elems=1 << 28):
    """Chunked torch baseline: distances by `!=`-sum over [qc, N, bits] chunks, then topk (smallest)."""
    qc = max(1, chunk_elems // (g.shape[0] * g.shape[1]))
    out_d, out_i = [], []
    for i in range(0, q.shape[0], qc):
        d = (q[i:i + qc, None, :] != g[None, :, :]).sum(dim=2, dtype=torch.int32)
        v, ix = torch.topk(d, k, dim=1, largest=False)
        out_d.append(v)
        out_i.append(ix)
    return torch.cat(out_d), torch.cat(out_i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--searches", default=SEARCHES)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-hamming", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.ath import ATHNet, hamming_topk
    dev_name = torch.cuda.get_device_name(0)
    rows = []

    def emit(r):
        r["device"] = dev_name
        rows.append(r)
        print(json.dumps(r), flush=True)

    if not a.no_model:
        torch.manual_seed(0)
        net = ATHNet(64, 4, input_size=256).eval().cuda().requires_grad_(False)
        for bs in [int(v) for v in a.batches.split(",")]:
            x = torch.rand(bs, 3, 256, 256, device="cuda")
            runs = [("ath_native_fp32", lambda: net(x))]
            if not a.no_eager:
                runs.append(("ath_eager_fp32", lambda: _eager(net, x)))
            rate = {}
            with torch.no_grad():
                for name, fn in runs:
                    sec = _time(fn, a.steps, a.warmup)
                    rate[name] = bs / sec
                    r = {"path": name, "batch": bs, "img_per_s": round(bs / sec, 1), "ms_per_step": round(sec * 1e3, 3),
                         "steps": a.steps}
                    if name == "ath_eager_fp32":
                        r["native_over_eager"] = round(rate["ath_native_fp32"] / rate[name], 3)
                    emit(r)
            del x
            torch.cuda.empty_cache()

    if not a.no_hamming:
        for spec in a.searches.split(","):
            nq, n, bits, k = (int(v) for v in spec.split(":"))
            gen = torch.Generator(device="cuda").manual_seed(nq + bits)
            q = (torch.rand((nq, bits), device="cuda", generator=gen) < 0.5).float()
            g = (torch.rand((n, bits), device="cuda", generator=gen) < 0.5).float()
            d_nat, _ = hamming_topk(q, g, k)
            sec = _time(lambda: hamming_topk(q, g, k), a.steps, a.warmup)
            r = {"path": "hamming_topk_native", "nq": nq, "n": n, "bits": bits, "k": k, "queries_per_s": round(nq / sec, 1),
                 "ms_per_search": round(sec * 1e3, 3), "steps": a.steps}
            emit(r)
            qb, gb = q.to(torch.int16), g.to(torch.int16)
            d_t, _ = _torch_hamming(qb, gb, k)
            tsteps = max(1, min(a.steps, 2))
            tsec = _time(lambda: _torch_hamming(qb, gb, k), tsteps, 1)
            emit({"path": "hamming_torch_chunked", "nq": nq, "n": n, "bits": bits, "k": k, "queries_per_s": round(nq / tsec, 1),
                  "ms_per_search": round(tsec * 1e3, 3), "steps": tsteps, "native_over_torch": round(tsec / sec, 2),
                  "distances_equal": bool(torch.equal(d_t, d_nat))})
            del q, g, qb, gb
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
