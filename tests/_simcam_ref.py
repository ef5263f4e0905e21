"""Float64 restatement of SimCAM (the reference's explanations.py SimCAM / SimCAM_Densenet121 / SimCAM_MedSigLIP) on given
feature rows, in numpy, plus the tiny models the fixture (tests/golden/make_golden_simcam.py) runs the reference's classes on.

Per pair: D = Q R^T (Q, R [h * w, C], rows in row-major position order), s = max(D) + eps, A = relu(D / s);
query map = A summed over retrieved positions, retrieved map = A summed over query positions, or with a point (p0 along H, p1
along W) the bilinear blend of A's rows at the point on the query grid padded by one replicated row / column on each side;
each map resized to H x W by bilinear interpolation with half-pixel centres (align_corners=False, sources clamped at 0).
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn


def resize_bilinear(m, H, W):
    """[..., h, w] -> [..., H, W]: out(y, x) interpolates m at (max((y + .5) h / H - .5, 0), max((x + .5) w / W - .5, 0)), the
    upper neighbour clamped to the last row / column."""
    m = np.asarray(m, dtype=np.float64)
    h, w = m.shape[-2:]

    def axis(n_in, n_out):
        src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        lo = np.floor(src).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        return lo, hi, src - lo

    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    top = m[..., y0, :][..., :, x0] * (1 - lx) + m[..., y0, :][..., :, x1] * lx
    bot = m[..., y1, :][..., :, x0] * (1 - lx) + m[..., y1, :][..., :, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def point_blend(A, h, w, point, H, W):
    """A [h * w (query), h * w (retrieved)] -> [h, w]: the retrieved map at the query point (padded-grid bilinear blend)."""
    gx = (point[0] + 0.5) / H * h + 0.5
    gy = (point[1] + 0.5) / W * w + 0.5
    x0, y0 = int(math.floor(gx)), int(math.floor(gy))
    dx, dy = gx - x0, gy - y0

    def row(px, py):                                  # padded index -> the replicated edge of the query grid
        i = min(max(px - 1, 0), h - 1)
        j = min(max(py - 1, 0), w - 1)
        return A[i * w + j].reshape(h, w)

    out = (row(x0, y0) * (1 - dx) * (1 - dy) + row(x0 + 1, y0) * dx * (1 - dy) + row(x0, y0 + 1) * (1 - dx) * dy
           + row(x0 + 1, y0 + 1) * dx * dy)
    return np.maximum(out, 0.0)


def pair_maps(q, r, h, w, H, W, eps, point=None):
    """One pair: q, r [h * w, C] -> (query map [H, W], retrieved map [H, W]) in float64."""
    D = np.asarray(q, np.float64) @ np.asarray(r, np.float64).T
    with np.errstate(invalid="ignore", divide="ignore"):
        A = D / (D.max() + eps) if not np.isnan(D).any() else np.full_like(D, np.nan)
    A = np.where(np.isnan(A), np.nan, np.maximum(A, 0.0))
    m1 = A.sum(axis=1).reshape(h, w)
    m2 = point_blend(A, h, w, point, H, W) if point is not None else A.sum(axis=0).reshape(h, w)
    return resize_bilinear(m1, H, W), resize_bilinear(m2, H, W)


def simcam(q, rs, h, w, H, W, eps=1e-8, point=None):
    """q [h * w, C], rs [P, h * w, C] -> [P, 2, H, W]"""
    return np.stack([np.stack(pair_maps(q, r, h, w, H, W, eps, point)) for r in rs])


def token_fc(x, weight, bias, hw):
    """The per-position fc: x @ W^T + b / hw."""
    return np.asarray(x, np.float64) @ np.asarray(weight, np.float64).T + np.asarray(bias, np.float64) / hw


def rows_of(fmap):
    """[B, C, h, w] -> [B, h * w, C]"""
    f = np.asarray(fmap, np.float64)
    return f.transpose(0, 2, 3, 1).reshape(f.shape[0], -1, f.shape[1])


# ---- the fixture's models: the target layer's output is a known function of the input ------------------------------------
class PoolNet(nn.Module):
    """SimCAM's model: `pool` (block means, h x w) then `tap` (the target layer: identity, or ReLU for non-negative maps)."""

    def __init__(self, kernel, relu=False):
        super().__init__()
        self.pool = nn.AvgPool2d(kernel)
        self.tap = nn.ReLU() if relu else nn.Identity()

    def forward(self, x):
        return self.tap(self.pool(x)).mean(dim=(2, 3))


def pool_features(kernel):
    """SimCAM_Densenet121's feature module: children `pool` and `relu` (the reference's target name)."""
    return nn.Sequential(OrderedDict(pool=nn.AvgPool2d(kernel), relu=nn.ReLU()))


class _Tower(nn.Module):
    def __init__(self, kernel):
        super().__init__()
        self.pool = nn.AvgPool2d(kernel)
        self.post_layernorm = nn.Identity()

    def forward(self, pixel_values=None):
        f = self.pool(pixel_values)
        return (self.post_layernorm(f.flatten(2).transpose(1, 2)),)


class TokenNet(nn.Module):
    """SimCAM_MedSigLIP's model: `backbone(pixel_values=..)` whose `post_layernorm` sees the block means as tokens [B, N, C]."""

    def __init__(self, kernel):
        super().__init__()
        self.backbone = _Tower(kernel)


def block_means(x, kernel):
    """What the fixture models' target layers see: AvgPool2d(kernel) of x [B, C, H, W] in float64."""
    with torch.no_grad():
        return nn.AvgPool2d(kernel)(torch.as_tensor(np.asarray(x, np.float64))).numpy()


# ---- the fixture's cases (tests/golden/make_golden_simcam.py writes, tests/test_simcam_cpu.py reads) ----------------------
def _pt(name, H, W):
    return {"tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1), "c": (H // 2, W // 2)}[name]


CASES = (
    # SimCAM: 10 x 14 images, 2 x 2 block means -> a 5 x 7 map (3 x 3 blocks: 3 x 4), C = 6
    dict(name="cam_signed", cls="SimCAM", kernel=2, nq=1, nr=3, size=(10, 14), c=6, sign="signed"),
    dict(name="cam_nonneg", cls="SimCAM", kernel=2, nq=1, nr=3, size=(10, 14), c=6, sign="signed", relu=True),
    dict(name="cam_neg", cls="SimCAM", kernel=2, nq=1, nr=2, size=(10, 14), c=6, sign="neg"),
    dict(name="cam_fc", cls="SimCAM", kernel=2, nq=1, nr=3, size=(10, 14), c=6, sign="signed", fc=5),
    dict(name="cam_q2", cls="SimCAM", kernel=2, nq=2, nr=2, size=(10, 14), c=6, sign="signed"),
    dict(name="cam_k3", cls="SimCAM", kernel=3, nq=1, nr=2, size=(10, 14), c=6, sign="signed"),
) + tuple(
    dict(name=f"cam_pt_{p}", cls="SimCAM", kernel=2, nq=1, nr=2, size=(10, 14), c=6, sign="signed", point=_pt(p, 10, 14))
    for p in ("tl", "tr", "bl", "br", "c")
) + (
    # SimCAM_Densenet121: feature module (pool, relu), target "relu"; images 0 and 1 only
    dict(name="dn_plain", cls="SimCAM_Densenet121", kernel=2, nq=1, nr=2, size=(10, 14), c=6, sign="signed"),
    dict(name="dn_fc", cls="SimCAM_Densenet121", kernel=2, nq=1, nr=1, size=(10, 14), c=6, sign="signed", fc=5),
    dict(name="dn_zero", cls="SimCAM_Densenet121", kernel=2, nq=1, nr=1, size=(10, 14), c=6, sign="zero"),
    dict(name="dn_q2", cls="SimCAM_Densenet121", kernel=2, nq=2, nr=1, size=(10, 14), c=6, sign="signed"),
) + tuple(
    dict(name=f"dn_pt_{p}", cls="SimCAM_Densenet121", kernel=2, nq=1, nr=1, size=(10, 14), c=6, sign="signed",
         point=_pt(p, 10, 14))
    for p in ("tl", "tr", "bl", "br", "c")
) + (
    # SimCAM_MedSigLIP: 12 x 12 images, 2 x 2 block means -> 36 tokens
    dict(name="sig_k3", cls="SimCAM_MedSigLIP", kernel=2, nq=1, nr=3, size=(12, 12), c=6, sign="signed"),
    dict(name="sig_k1", cls="SimCAM_MedSigLIP", kernel=2, nq=1, nr=1, size=(12, 12), c=6, sign="signed"),
    dict(name="sig_neg", cls="SimCAM_MedSigLIP", kernel=2, nq=1, nr=2, size=(12, 12), c=6, sign="neg"),
)


def case_inputs(case, gen):
    """Seeded float64 inputs (x_q, x) of a case: 'signed' normal; 'neg' |query| and -|retrieved| (every D <= 0);
    'zero' -|all| (the ReLU map is all zero)."""
    H, W = case["size"]
    xq = torch.randn(case["nq"], case["c"], H, W, generator=gen, dtype=torch.float64)
    x = torch.randn(case["nr"], case["c"], H, W, generator=gen, dtype=torch.float64)
    if case["sign"] == "neg":
        xq, x = xq.abs(), -x.abs()
    elif case["sign"] == "zero":
        xq, x = -xq.abs(), -x.abs()
    return xq, x


def case_model(case, classes, fc=None):
    """(explainer, call) for a case on the given class namespace (the reference's explanations module or mirx.xai)."""
    k = case["kernel"]
    if case["cls"] == "SimCAM":
        model = PoolNet(k, relu=case.get("relu", False)).double().eval()
        return classes.SimCAM(model, model.tap, fc=fc)
    if case["cls"] == "SimCAM_Densenet121":
        feats = pool_features(k)
        model = nn.Sequential(feats, nn.AdaptiveAvgPool2d((1, 1)), *([fc] if fc is not None else [])).double().eval()
        return classes.SimCAM_Densenet121(model, model[0], target_layers=["relu"], fc=model[2] if fc is not None else None)
    model = TokenNet(k).double().eval()
    return classes.SimCAM_MedSigLIP(model, model.backbone.post_layernorm)


def case_expected(case, xq, x, fc_w=None, fc_b=None):
    """The restatement's answer for a case, from the block means its target layer sees."""
    k, (H, W) = case["kernel"], case["size"]
    f = block_means(np.concatenate([xq, x]), k)
    if case.get("relu") or case["cls"] == "SimCAM_Densenet121":
        f = np.maximum(f, 0.0)
    h, w = f.shape[-2:]
    rows = rows_of(f)
    if fc_w is not None:
        rows = token_fc(rows, fc_w, fc_b, h * w)
    pt = case.get("point")
    if case["cls"] == "SimCAM":
        return simcam(rows[0], rows[1:], h, w, H, W, 1e-8, pt)
    if case["cls"] == "SimCAM_Densenet121":
        return simcam(rows[0], rows[1:2], h, w, H, W, 0.0, pt)[0]
    return simcam(rows[0], rows[1:], h, w, H, W, 1e-8)[:, 1]
