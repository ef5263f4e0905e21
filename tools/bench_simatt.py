"""SimAtt saliency on one GPU: compute_saliency.py's recipe on a seeded mirx DenseNet121 at 224 x 224 (with and without an fc),
per call of the native SimAtt at (1 query + 1 positive) and at a triplet, simatt_pairs at K = 1, 5, 8 and 64, K single SimAtt
calls (the drivers' per-hit loop) for comparison, the feature forward alone, mirx_simatt alone on the same rows, and the
same-process baseline: the same explainer on its torch path (the reference's formulas on the eager modules, autograd included).

    python tools/bench_simatt.py [--steps 200] [--warmup 20] [--embedding-dims 0,64] [--kernels-only] [--out profiles/<name>.txt]

Times are CUDA-event means over `steps` calls after `warmup` calls (a quarter of a second or more per window for the native
rows, which are measured three times: the figure is the median and `spread` the (max - min) / median of the three); the slow
baselines (the torch path, K single calls) use steps / 10, at least 5.  One JSON line per measurement.  --kernels-only runs the
native calls alone (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--embedding-dims", default="0,64")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mirx.simatt as S
    from mirx.model import DenseNet121
    assert torch.cuda.is_available(), "bench_simatt needs a GPU"
    dev = torch.device("cuda:0")
    res = []
    slow = max(5, a.steps // 10)

    def emit(d):
        print(json.dumps(d), flush=True)
        res.append(d)

    for emb in (int(e) for e in a.embedding_dims.split(",")):
        torch.manual_seed(0)
        model = DenseNet121(embedding_dim=emb or None).eval().to(dev)
        seq = nn.Sequential(*list(model.children())[0], *list(model.children())[1:]).eval()
        native = S.SimAtt(seq, seq[0], ["relu"])
        eager = S.SimAtt(seq, seq[0], ["relu"])
        fc = seq[2] if emb else None
        fw, fb = (fc.weight, fc.bias) if emb else (None, None)
        g = torch.Generator().manual_seed(1)
        xq = torch.randn(1, 3, 224, 224, generator=g).to(dev)
        xr = torch.randn(64, 3, 224, 224, generator=g).to(dev)

        def torch_path(fn):
            """fn() with the native gate shut: the reference's formulas, eager modules, autograd"""
            gate, S._native_plan = S._native_plan, lambda *args, **kw: None
            try:
                out = fn()
                assert not eager.last_native
                return out
            finally:
                S._native_plan = gate

        for tag, call, n_img in (("anchor_positive", lambda ex: ex(xq, xr[:1]), 2),
                                 ("triplet", lambda ex: ex(xq, xr[:1], xr[1:2]), 3)):
            call(native)
            assert native.last_native
            d = {"embedding_dim": emb, "shape": tag, "images": n_img}
            d["ms_native"], d["spread_native"] = _time3(lambda: call(native), a.steps, a.warmup)
            if not a.kernels_only:
                xa = torch.cat([xq, xr[:n_img - 1]])
                with torch.no_grad():
                    d["ms_feature_forward"] = round(_time(lambda: model._relu_rows(xa, model._cache()), a.steps, a.warmup), 4)
                    rows, h, w = model._relu_rows(xa, model._cache())
                    d["ms_mirx_simatt"], d["spread_mirx_simatt"] = _time3(
                        lambda: S.simatt_maps(rows, fw, fb, (224, 224), "group", h, w, positive=True), 10 * a.steps, a.warmup)
                d["ms_torch_path"] = round(torch_path(lambda: _time(lambda: call(eager), slow, 3)), 4)
            emit(d)
        for k in (1, 5, 8, 64):
            S.simatt_pairs(native, xq, xr[:k])
            assert native.last_native
            d = {"embedding_dim": emb, "shape": "pairs", "K": k}
            d["ms_native_pairs"], d["spread_native_pairs"] = _time3(lambda: S.simatt_pairs(native, xq, xr[:k]), a.steps, a.warmup)
            if not a.kernels_only:
                d["ms_native_k_single_calls"] = round(_time(lambda: [native(xq, xr[i:i + 1]) for i in range(k)], slow, 3), 4)
                with torch.no_grad():
                    rows, h, w = S._rows_of(model, torch.cat([xq, xr[:k]]))
                    d["ms_mirx_simatt"], d["spread_mirx_simatt"] = _time3(
                        lambda: S.simatt_maps(rows, fw, fb, (224, 224), "pairs", h, w, positive=True), 10 * a.steps, a.warmup)
                d["ms_torch_path_pairs"] = round(torch_path(lambda: _time(lambda: S.simatt_pairs(eager, xq, xr[:k]), slow if k <= 8 else 5, 2)), 4)
            emit(d)
        del model, seq, native, eager
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(f"# tools/bench_simatt.py on {torch.cuda.get_device_name(0)}: steps {a.steps}, warmup {a.warmup}; ms per call\n")
            for d in res:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
