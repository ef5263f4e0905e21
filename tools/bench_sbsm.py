"""SBSM occlusion saliency of one pair on one GPU: a seeded mirx DenseNet121 at 224 x 224, window 24, stride 5 (N = 2401 masks),
gpu_batch 250 -- the drivers' geometry.

    python tools/bench_sbsm.py [--reps 5] [--warmup 1] [--gpu-batch 250] [--out profiles/<name>.txt]

In one process, for Q = B = 1:
  native        mirx.xai.SBSMBatch as it is: interval-described windows, mirx_sbsm_compose / _gain / _accumulate
  parent_form   the formulation this replaced, restated here: uint8 masks [N, 1, H, W] and the dense fp32 [HW, N] matrix on the
                device, masked images as a broadcast product of gpu_batch // B whole masks, torch.cdist, one [., N] x [N, HW] matmul
The two calls alternate after the warm-up, `reps` times each; each time is a device-event interval around one call.  Printed:
every time, the medians, the spread (max - min) / median of each, the peak of torch.cuda.max_memory_allocated over one call of
each above the memory held before either explainer existed (the parent form's includes its mask tensors, which it needs on the
device), the device-event split of the native call into forwards / compose / gain + accumulate (each piece between its own
events, summed over the chunks), max |native - parent form| over the map, and the distance of each from the parent formulation
evaluated in float64 on the same fp32 embeddings.  One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class ParentForm:
    """SBSMBatch before the native path: device masks, [HW, N] matmul, torch.cdist."""

    def __init__(self, model, input_size, window, stride, gpu_batch, device):
        from mirx.xai import sliding_window_masks
        self.model, self.input_size, self.gpu_batch = model, input_size, gpu_batch
        self.masks = torch.from_numpy(sliding_window_masks(input_size, window, stride)).to(device)
        self.N = self.masks.shape[0]
        inv = (1 - self.masks.reshape(self.N, -1)).float()
        self._inv_t = inv.t().contiguous()
        self._count = inv.sum(dim=0)

    def __call__(self, x_q, x):
        b, c, h, w = x.shape
        with torch.no_grad():
            e_q = self.model(x_q)
            out = []
            per = max(1, self.gpu_batch // b)
            for n0 in range(0, self.N, per):
                m = self.masks[n0:n0 + per].to(x.dtype)
                out.append(self.model((m[:, None] * x[None]).reshape(-1, c, h, w)))
            e_m = torch.cat(out).reshape(self.N, b, -1)
            e_r = self.model(x)
            o_dist = torch.cdist(e_q, e_r).reshape(-1, 1)
            m_dist = torch.cdist(e_q, e_m.reshape(self.N * b, -1))
            m_dist = m_dist.reshape(-1, self.N, b).permute(0, 2, 1).reshape(-1, self.N)
            gain = (m_dist - o_dist).clamp(min=0)
            sal = (gain.float() @ self._inv_t.t()) / self._count
        return sal.reshape(-1, h, w)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _peak(fn, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _native_split(ex, model, x_q, x):
    """The native sequence of SBSMBatch.forward with an event pair around every piece -> ms (forwards, compose, gain + accumulate)."""
    from mirx import sbsm
    dev = x.device
    row_iv, col_iv = (torch.from_numpy(iv).to(dev) for iv in ex._intervals)
    pairs = {"forwards": [], "compose": [], "gain_accumulate": []}

    def piece(kind, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        pairs[kind].append((a, b))
        return out
    total = ex.N * x.shape[0]
    step = ex.gpu_batch
    with torch.no_grad():
        buf = torch.empty((min(step, total),) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        e_q = piece("forwards", lambda: model(x_q))
        e_r = piece("forwards", lambda: model(x))
        e_m = torch.empty((total, e_q.shape[1]), dtype=torch.float32, device=dev)
        for g0 in range(0, total, step):
            n = min(step, total - g0)
            imgs = piece("compose", lambda: sbsm.sbsm_compose(x, row_iv, col_iv, g0, n, out=buf[:n]))
            e_m[g0:g0 + n] = piece("forwards", lambda: model(imgs))
        piece("gain_accumulate", lambda: sbsm.sbsm_accumulate(sbsm.sbsm_gain(e_q, e_m, e_r), row_iv, col_iv, ex.input_size))
        torch.cuda.synchronize()
    return {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in pairs.items()}, (e_q, e_m, e_r)


def _float64_form(parent_ex, e_q, e_m, e_r, block=256):
    """The yardstick for the two maps: the parent formulation's arithmetic in float64 on the same fp32 embeddings (direct
    distances, the mask matrix product in blocks of masks)."""
    n, b = parent_ex.N, e_r.shape[0]
    e_q, e_m, e_r = e_q.double(), e_m.double(), e_r.double()
    o_dist = (e_q[:, None] - e_r[None]).norm(dim=2).reshape(-1, 1)
    m_dist = (e_q[:, None] - e_m[None]).norm(dim=2).reshape(-1, n, b).permute(0, 2, 1).reshape(-1, n)
    gain = (m_dist - o_dist).clamp(min=0)
    total = torch.zeros((gain.shape[0], parent_ex._inv_t.shape[0]), dtype=torch.float64, device=gain.device)
    for n0 in range(0, n, block):
        total += gain[:, n0:n0 + block] @ parent_ex._inv_t[:, n0:n0 + block].t().double()
    return (total / parent_ex._count.double()).reshape(-1, *parent_ex.input_size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gpu-batch", type=int, default=250)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from mirx.model import DenseNet121
    from mirx.xai import SBSMBatch
    assert torch.cuda.is_available(), "bench_sbsm needs a GPU"
    dev = torch.device("cuda:0")
    size, window, stride = 224, 24, 5
    torch.manual_seed(0)
    model = DenseNet121().eval().to(dev)
    g = torch.Generator().manual_seed(1)
    xq = torch.randn(1, 3, size, size, generator=g).to(dev)
    xr = torch.randn(1, 3, size, size, generator=g).to(dev)
    with torch.no_grad():
        model(xq)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()

    ex = SBSMBatch(model, (size, size), gpu_batch=a.gpu_batch)
    ex.generate_masks(window, stride, savepath=None)
    native = lambda: ex(xq, xr)                                              # noqa: E731
    peak_native = _peak(native, base)
    assert ex.last_native
    parent_ex = ParentForm(model, (size, size), window, stride, a.gpu_batch, dev)
    parent = lambda: parent_ex(xq, xr)                                       # noqa: E731
    peak_parent = _peak(parent, base)

    for _ in range(a.warmup):
        native()
        parent()
    t_native, t_parent = [], []
    for _ in range(a.reps):
        ms, sal_n = _timed(native)
        t_native.append(round(ms, 3))
        ms, sal_p = _timed(parent)
        t_parent.append(round(ms, 3))
    diff = float((sal_n - sal_p).abs().max())
    split, embeddings = _native_split(ex, model, xq, xr)
    sal_64 = _float64_form(parent_ex, *embeddings)

    def spread(t):
        return round((max(t) - min(t)) / statistics.median(t), 4)
    d = {"device": torch.cuda.get_device_name(0), "model": "DenseNet121", "size": size, "window": window, "stride": stride,
         "N": ex.N, "Q": 1, "B": 1, "gpu_batch": a.gpu_batch, "reps": a.reps, "warmup": a.warmup,
         "ms_native": t_native, "ms_parent_form": t_parent,
         "ms_native_median": round(statistics.median(t_native), 3), "ms_parent_form_median": round(statistics.median(t_parent), 3),
         "spread_native": spread(t_native), "spread_parent_form": spread(t_parent),
         "native_over_parent_form": round(statistics.median(t_native) / statistics.median(t_parent), 4),
         "peak_bytes_native": int(peak_native), "peak_bytes_parent_form": int(peak_parent),
         "ms_native_split": split, "max_abs_native_minus_parent_form": diff,
         "max_abs_native_minus_float64_form": float((sal_n.double() - sal_64).abs().max()),
         "max_abs_parent_form_minus_float64_form": float((sal_p.double() - sal_64).abs().max()),
         "saliency_max": float(np.nanmax(sal_p.cpu().numpy()))}
    line = json.dumps(d)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_sbsm.py: one SBSM pair, native call against the parent formulation, alternating; ms per call, bytes\n")
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
