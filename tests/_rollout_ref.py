"""Attention rollout (the reference's explanations.py AttentionRolloutMedSigLIP) restated in float64 numpy, the tiny stand-in
model the fixture tests/golden/rollout_ref.npz was made on, and its cases.

The stand-in's backbone ignores the pixels: it returns seeded attention tuples (dyadic values, so the head fusions are exact,
with ties planted at each row's k-th smallest fused value), seeded post-LayerNorm tokens, and model(query) a seeded unit
embedding; `projection` is MedSigLIP's Sequential(Linear, LayerNorm, ReLU, Linear) at a tiny width.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

LAYERS, HEADS, GRID, BATCH = 3, 4, 4, 2
N = GRID * GRID
SIZE = (10, 14)                      # the retrieved images' H x W (the map is upsampled to it)
SETUPS = {"proj": dict(d=12, e=6), "same": dict(d=6, e=6)}    # hidden width != / == embedding width
RATIOS = (0.0, 0.5, 0.9)
CASES = tuple(dict(name=f"{s}_{f}_r{int(r * 10)}_{'qg' if qg else 'plain'}", setup=s, fusion=f, ratio=r, qg=qg)
              for s in ("proj",) for f in ("mean", "max", "min") for r in RATIOS for qg in (True, False)) + tuple(
    dict(name=f"same_{f}_r9_qg", setup="same", fusion=f, ratio=0.9, qg=True) for f in ("mean", "max", "min"))


def fuse(att, mode):
    """[B, heads, N, N] -> [B, N, N]"""
    if mode == "mean":
        return att.mean(axis=1)
    if mode == "max":
        return att.max(axis=1)
    if mode == "min":
        return att.min(axis=1)
    raise ValueError(f"Unknown head_fusion mode: {mode!r}")


def row_stage(a, k):
    """a [..., N] (float64 or float32 input, computed in float64): a * (a > k-th smallest) when k > 0, + I, / (sum + 1e-8);
    the diagonal of row i is column i % N."""
    a = np.array(a, np.float64)
    n = a.shape[-1]
    if k > 0:
        thr = np.partition(a, k - 1, axis=-1)[..., k - 1:k]
        a = a * (a > thr)
    rows = a.reshape(-1, n)
    idx = np.arange(rows.shape[0])
    rows[idx, idx % n] += 1.0
    return rows.reshape(a.shape) / (a.sum(axis=-1, keepdims=True) + 1e-8)


def layer_matrix(att, mode, k):
    """One layer's A_l [B, N, N] from its attention probabilities [B, heads, N, N]."""
    return row_stage(fuse(np.asarray(att, np.float64), mode), k)


def resize_bilinear(m, H, W):
    """F.interpolate(mode="bilinear", align_corners=False) of maps [..., h, w] in float64."""
    h, w = m.shape[-2:]

    def axis(n_in, n_out):
        src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.floor(src).astype(int)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, src - i0

    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    top = m[..., y0, :][..., x0] * (1 - lx) + m[..., y0, :][..., x1] * lx
    bot = m[..., y1, :][..., x0] * (1 - lx) + m[..., y1, :][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def importance(mats):
    """mats: per layer [B, N, N] -> (1/N) 1^T A_{L-1} ... A_0, [B, N] (the rollout's mean over rows)."""
    B, n, _ = mats[0].shape
    v = np.full((B, n), 1.0 / n)
    for a in reversed(mats):
        v = np.einsum("bi,bij->bj", v, a)
    return v


def projection(x, p):
    """MedSigLIP's projection Sequential(Linear, LayerNorm(eps 1e-5), ReLU, Linear) in float64."""
    h = x @ p["w0"].T + p["b0"]
    mu = h.mean(-1, keepdims=True)
    var = ((h - mu) ** 2).mean(-1, keepdims=True)
    h = (h - mu) / np.sqrt(var + 1e-5) * p["g1"] + p["be1"]
    return np.maximum(h, 0.0) @ p["w3"].T + p["b3"]


def normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)


def patch_sim(tokens, q_feat, proj=None):
    """clamp(normalize(proj(normalize(tokens))) . q_feat, 0): tokens [B, N, D], q_feat [E]; proj only when D != E."""
    p = normalize(np.asarray(tokens, np.float64))
    if p.shape[-1] != q_feat.shape[-1]:
        p = normalize(projection(p, proj))
    return np.maximum((p * q_feat).sum(-1), 0.0)


def rollout(atts, fusion, ratio, H, W, tokens=None, q_feat=None, proj=None):
    """The explainer's output [B, H, W] from per-layer attentions [B, heads, N, N] (float64)."""
    n = atts[0].shape[-1]
    k = max(1, int(n * ratio)) if ratio > 0.0 else 0
    v = importance([layer_matrix(a, fusion, k) for a in atts])
    if tokens is not None:
        v = v * patch_sim(tokens, q_feat, proj)
    side = int(n ** 0.5)
    return resize_bilinear(v.reshape(-1, side, side), H, W)


# ---- the stand-in and its inputs --------------------------------------------------------------------------------------
def setup_inputs(setup, seed=2029):
    """float64 inputs of a setup: atts [L, B, heads, N, N], tokens [B, N, D], q_feat [E], projection parameters."""
    cfg = SETUPS[setup]
    rng = np.random.default_rng(seed + cfg["d"])
    atts = rng.integers(0, 64, size=(LAYERS, BATCH, HEADS, N, N)).astype(np.float64) / 1024.0
    # plant ties: for every fusion and ratio, two entries above each row's k-th smallest fused value set to it in all heads
    for layer in range(LAYERS):
        for fusion in ("mean", "max", "min"):
            for ratio in RATIOS[1:]:
                k = max(1, int(N * ratio))
                a = fuse(atts[layer], fusion)
                thr = np.partition(a, k - 1, axis=-1)[..., k - 1]
                for b in range(BATCH):
                    for i in range(N):
                        above = np.nonzero(a[b, i] > thr[b, i])[0]
                        for j in rng.permutation(above)[:1]:
                            atts[layer, b, :, i, j] = thr[b, i]
    d, e = cfg["d"], cfg["e"]
    tokens = rng.standard_normal((BATCH, N, d))
    q_feat = normalize(rng.standard_normal(e))
    proj = dict(w0=rng.standard_normal((8, d)) / np.sqrt(d), b0=0.1 * rng.standard_normal(8), g1=1 + 0.1 * rng.standard_normal(8),
                be1=0.1 * rng.standard_normal(8), w3=rng.standard_normal((e, 8)) / np.sqrt(8), b3=0.1 * rng.standard_normal(e))
    return dict(atts=atts, tokens=tokens, q_feat=q_feat, **{f"proj_{k}": v for k, v in proj.items()})


def proj_of(inputs):
    return {k[5:]: v for k, v in inputs.items() if k.startswith("proj_")}


class _Backbone(nn.Module):
    def __init__(self, atts, tokens):
        super().__init__()
        self.atts, self.tokens = atts, tokens

    def forward(self, pixel_values=None, output_attentions=False, return_dict=True):
        b = pixel_values.shape[0]
        return SimpleNamespace(last_hidden_state=self.tokens[:b],
                               attentions=tuple(a[:b] for a in self.atts) if output_attentions else None)


class StandIn(nn.Module):
    """model.backbone(pixel_values, output_attentions=True) -> the seeded attentions and tokens; model(query) -> q_feat
    [1, E]; model.projection a float64 Sequential(Linear, LayerNorm, ReLU, Linear)."""

    def __init__(self, inputs):
        super().__init__()
        t = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in inputs.items()}
        self.backbone = _Backbone(t["atts"], t["tokens"])
        d, e = t["tokens"].shape[-1], t["q_feat"].shape[0]
        self.projection = nn.Sequential(nn.Linear(d, 8), nn.LayerNorm(8), nn.ReLU(), nn.Linear(8, e)).double()
        with torch.no_grad():
            self.projection[0].weight.copy_(t["proj_w0"])
            self.projection[0].bias.copy_(t["proj_b0"])
            self.projection[1].weight.copy_(t["proj_g1"])
            self.projection[1].bias.copy_(t["proj_be1"])
            self.projection[3].weight.copy_(t["proj_w3"])
            self.projection[3].bias.copy_(t["proj_b3"])
        self.q_feat = t["q_feat"]

    def forward(self, x):
        return self.q_feat[None].expand(x.shape[0], -1)


def pixels(b):
    return torch.zeros((b, 3) + SIZE, dtype=torch.float64)


def case_expected(case, inputs):
    atts = list(np.asarray(inputs["atts"]))
    if case["qg"]:
        return rollout(atts, case["fusion"], case["ratio"], *SIZE, inputs["tokens"], inputs["q_feat"], proj_of(inputs))
    return rollout(atts, case["fusion"], case["ratio"], *SIZE)


# ---- the layer kernel's float64 reference, its error bound and the near-tie audit (the GPU tests) ----------------------
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _score_bound(qkv, heads, dh, scale):
    """max over (image, head, i, j) of gamma_dh * scale * sum_d |q_d k_d|: the f32 scores' error bound."""
    b, n, _ = qkv.shape
    x = qkv.double().abs().view(b, n, 3, heads, dh)
    m = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]).max().item()
    return ((dh + 3) * U / (1 - dh * U)) * scale * m               # + 3 u: the scale product and the max subtraction


def _fused64(qkv, heads, dh, scale, fusion):
    """float64 softmax((q k^T) * scale) of the f32 qkv, fused over the heads -> [b, n, n] (torch float64 on the GPU)."""
    b, n, _ = qkv.shape
    x = qkv.to(DEV).double().view(b, n, 3, heads, dh)
    s = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) * scale
    p = torch.softmax(s, dim=-1)
    return {"mean": lambda: p.mean(1), "max": lambda: p.amax(1), "min": lambda: p.amin(1)}[fusion]()


def _audited_expected(F64, got, k, tol):
    """The float64 row stage of F64 [b, n, n] with the kept set the kernel chose (got [b, n, n], its A_l): every entry where
    the two kept sets differ must be a near-tie, |F64 - thr| <= tol * thr.  Returns (expected A_l, number of flips)."""
    n = F64.shape[-1]
    eye = torch.eye(n, dtype=torch.float64, device=F64.device)
    if k == 0:
        mask = torch.ones_like(F64, dtype=torch.bool)
        flips = 0
    else:
        thr = torch.kthvalue(F64, k, dim=-1).values.unsqueeze(-1)
        kept64 = F64 > thr
        mask = got.double() > 0
        off = ~eye.bool()
        mask = torch.where(off, mask, kept64)                       # the diagonal: the float64 decision
        diff = (mask != kept64) & off
        flips = int(diff.sum())
        if flips:
            gap = ((F64 - thr).abs() / thr)[diff]
            assert float(gap.max()) <= tol, (flips, float(gap.max()), tol)
    a = F64 * mask + eye
    return a / (a.sum(-1, keepdim=True) + 1e-8), flips
