"""Attention rollout on one GPU: AttentionRolloutMedSigLIP on a seeded MedSigLIP at 448 x 448 (N = 1024, 27 layers, 16 heads,
head_dim 72), per explainer call at (1 query, 1 retrieved) and (1, 8), split into the query forward, the retrieved forward
(the native tower alone), the 27 layer kernels (on qkv captured from the tap) and the chain / finish; the same-process baseline
is the reference's formulas on backbone(output_attentions=True) (the torch path: library GEMMs, 27 materialised probability
tensors, kthvalue, bmm).  The layer kernel's scores are 2 * heads * N^2 * head_dim FLOP per image-layer; their rate is reported
against the 157.3 TF f32 matrix peak.

    python tools/bench_rollout.py [--steps 10] [--warmup 3] [--retrieved 1,8] [--out profiles/<name>.json]

It also times the retrieved forward with the layer kernels launched from the tap on the forward's stream against the same
launches on a side stream behind an event per layer (the overlap alternative).  Head-split variants are diagnostic builds of
k_rollout.hip selected with MIRX_LIB_PATH (`make -C <pkg>/csrc diag-src SRC=k_rollout NAME=ro_s1 FLAGS=-DMIRX_RO_SPLIT=1`).

Times are CUDA-event means over `steps` calls after `warmup` calls; one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--retrieved", default="1,8")
    ap.add_argument("--no-reference", action="store_true", help="skip the torch-path baseline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mirx.model import MedSigLIP
    from mirx.rollout import rollout_finish, rollout_layer, workspace_floats
    from mirx.xai import AttentionRolloutMedSigLIP
    dev = torch.device("cuda:0")
    res = []

    def emit(d):
        print(json.dumps(d), flush=True)
        res.append(d)

    torch.manual_seed(0)
    model = MedSigLIP().eval().to(dev)
    bb = model.backbone
    at = bb.encoder.layers[0].self_attn
    L, heads, dh, n = len(bb.encoder.layers), at.num_heads, at.head_dim, 1024
    ex = AttentionRolloutMedSigLIP(model)                     # mean, discard 0.9, query-guided: the drivers' defaults
    k = max(1, int(n * 0.9))
    with torch.no_grad():
        for nr in [int(v) for v in a.retrieved.split(",") if v]:
            g = torch.Generator().manual_seed(nr)
            xq = torch.randn(1, 3, 448, 448, generator=g).to(dev)
            x = torch.randn(nr, 3, 448, 448, generator=g).to(dev)
            ex(xq, x)
            assert ex.last_native
            t_call = _time(lambda: ex(xq, x), a.steps, a.warmup)
            t_q = _time(lambda: model(xq), a.steps, a.warmup)
            t_fwd = _time(lambda: bb.last_hidden_state(x), a.steps, a.warmup)
            qkvs = [None] * L

            def keep(i, qkv):
                qkvs[i] = qkv.clone()
            bb._hidden_tapped(x, keep)
            ws = torch.empty((workspace_floats(L, nr, n),), device=dev)

            def layers():
                for i in range(L):
                    rollout_layer(qkvs[i], heads, at.scale, "mean", k, i, L, ws)
            t_layers = _time(layers, a.steps, a.warmup)

            def tapped_same():
                bb._hidden_tapped(x, lambda i, qkv: rollout_layer(qkv, heads, at.scale, "mean", k, i, L, ws))
            side = torch.cuda.Stream(dev)

            def tapped_side():
                main = torch.cuda.current_stream(dev)

                def tap(i, qkv):
                    side.wait_stream(main)
                    qkv.record_stream(side)
                    with torch.cuda.stream(side):
                        rollout_layer(qkv, heads, at.scale, "mean", k, i, L, ws)
                bb._hidden_tapped(x, tap)
                main.wait_stream(side)
            t_same = _time(tapped_same, a.steps, a.warmup)
            t_side = _time(tapped_side, a.steps, a.warmup)
            out = torch.empty(nr, 448, 448, device=dev)
            patches = torch.nn.functional.normalize(torch.randn(nr, n, 512, device=dev), dim=-1)
            qf = torch.nn.functional.normalize(torch.randn(512, device=dev), dim=0)
            t_finish = _time(lambda: rollout_finish(ws, L, nr, 32, 32, (448, 448), patches, qf, out), a.steps, a.warmup)
            flop = 2.0 * heads * n * n * dh * L * nr
            del qkvs, ws
            torch.cuda.empty_cache()
            t_ref = float("nan") if a.no_reference else _time(lambda: ex._forward_torch(xq, x), max(1, a.steps // 2), 1)
            emit({"lib": os.path.basename(os.environ.get("MIRX_LIB_PATH", "libmirx.so")), "retrieved": nr, "queries": 1, "size": 448,
                  "N": n, "layers": L, "heads": heads, "head_dim": dh,
                  "ms_per_call": round(t_call, 3), "ms_query_forward": round(t_q, 3), "ms_retrieved_forward": round(t_fwd, 3),
                  "ms_layer_kernels": round(t_layers, 3), "ms_chain_finish": round(t_finish, 3),
                  "ms_forward_with_layer_kernels_same_stream": round(t_same, 3),
                  "ms_forward_with_layer_kernels_side_stream": round(t_side, 3),
                  "rollout_kernels_share_of_call": round((t_layers + t_finish) / t_call, 3),
                  "layer_kernel_tflops": round(flop / t_layers / 1e9, 2),
                  "layer_kernel_share_of_f32_matrix_peak": round(flop / t_layers / 1e9 / F32_PEAK_TF, 4),
                  "ms_reference_formulas_torch_path": None if a.no_reference else round(t_ref, 3),
                  "speedup_vs_reference": None if a.no_reference else round(t_ref / t_call, 2)})
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "results": res}, fh, indent=1)


if __name__ == "__main__":
    main()
