"""Float64 restatement of SimAtt's closed form (the reference's explanations.py SimAtt for a model whose tail after the target
map is average pool -> optional fc) on given feature rows, in numpy; the reference's own formulas (autograd) in torch on the same
rows, the float32 yardstick of the kernel's tolerance; and the tiny models / cases the fixture (tests/golden/make_golden_simatt.py)
runs the reference's class on.

rows [B, h * w, C], image 0 the query.  x_b = W mean_pos(rows[b]) + bias (the pooled vector without fc), xn = x / max(|x|, 1e-12),
wt = prod_j |xn_0 - xn_j| over the non-query images (the first factor flipped to 1 - itself in positive mode),
g_b = W^T (sign(x_b) * wt) / (h * w), M_b = resize(relu(rows[b] g_b)).  pairs mode: retrieval k alone against the query.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from _simcam_ref import pool_features, resize_bilinear

ULP32 = 2.0 ** -23             # one float32 ulp of a map's maximum, relative to it
SIGN_MARGIN = 1e-3             # with an fc: min |x[b, d]| >= SIGN_MARGIN * max |x[b, :]| in float64 (no sign can flip in float32)


# ---- the closed form in float64 ---------------------------------------------------------------------------------------
def embedding(rows, fc_w=None, fc_b=None):
    """x [B, D] in float64"""
    pooled = np.asarray(rows, np.float64).mean(axis=1)
    if fc_w is None:
        return pooled
    x = pooled @ np.asarray(fc_w, np.float64).T
    return x + np.asarray(fc_b, np.float64) if fc_b is not None else x


def sign_margin_ok(rows, fc_w, fc_b):
    """The condition on fixtures with an fc: no component of any image's embedding within SIGN_MARGIN of zero (relative)."""
    x = np.abs(embedding(rows, fc_w, fc_b))
    return bool((x.min(axis=1) >= SIGN_MARGIN * x.max(axis=1)).all())


def _maps(rows, x, wt, h, w, H, W, fc_w):
    """rows [n, hw, C], x [n, D], wt [D] -> [n, H, W]"""
    with np.errstate(invalid="ignore"):
        s = np.sign(x) * wt                                                    # sign(0) = 0; NaN stays NaN
        g = (s if fc_w is None else s @ np.asarray(fc_w, np.float64)) / (h * w)
        m = np.einsum("bpc,bc->bp", rows, g)
    m = np.where(np.isnan(m), np.nan, np.maximum(m, 0.0)).reshape(-1, h, w)
    return resize_bilinear(m, H, W)


def simatt(rows, h, w, H, W, fc_w=None, fc_b=None, mode="group", positive=False):
    """group -> [B, H, W]; pairs -> [B - 1, 2, H, W]"""
    rows = np.asarray(rows, np.float64)
    x = embedding(rows, fc_w, fc_b)
    with np.errstate(invalid="ignore"):
        xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
        diff = np.abs(xn[0] - xn[1:])
    if mode == "group":
        if positive and len(diff):
            diff[0] = 1 - diff[0]
        return _maps(rows, x, np.prod(diff, axis=0), h, w, H, W, fc_w)
    out = []
    for k in range(rows.shape[0] - 1):
        wt = 1 - diff[k] if positive else diff[k]
        out.append(_maps(rows[[0, k + 1]], x[[0, k + 1]], wt, h, w, H, W, fc_w))
    return np.stack(out)


# ---- the reference's formulas, autograd included, in torch on given rows (float32 yardstick; also float64) -----------------
def _reference_forward(feats, fc_w, fc_b, positive, H, W):
    feats = feats.clone().requires_grad_(True)
    x = F.adaptive_avg_pool2d(feats, (1, 1)).view(feats.shape[0], -1)
    if fc_w is not None:
        x = F.linear(x, fc_w, fc_b)
    xn = F.normalize(x.detach(), dim=1)
    wt = torch.abs(xn[0] - xn[1:])
    if positive:
        wt[0] = 1 - wt[0]
    wt = torch.prod(wt, dim=0)
    s = torch.matmul(torch.abs(x), wt)
    grads = torch.autograd.grad(torch.unbind(s), feats)[0]
    with torch.no_grad():
        weights = torch.mean(grads, dim=(2, 3))
        M = torch.bmm(weights.unsqueeze(1), feats.reshape(feats.shape[0], feats.shape[1], -1))
        M = M.reshape(feats.shape[0], 1, feats.shape[2], feats.shape[3]).clamp(min=0)
        return F.interpolate(M, size=(H, W), mode="bilinear").squeeze(1)


def ref_torch(rows, h, w, H, W, fc_w=None, fc_b=None, mode="group", positive=False, dtype=torch.float32):
    """The reference's computation on rows [B, h * w, C] (CPU) in `dtype` -> numpy float64 of its result."""
    rows = torch.as_tensor(np.asarray(rows)).to(dtype)
    feats = rows.view(rows.shape[0], h, w, rows.shape[2]).permute(0, 3, 1, 2).contiguous()
    fw = None if fc_w is None else torch.as_tensor(np.asarray(fc_w)).to(dtype)
    fb = None if fc_b is None else torch.as_tensor(np.asarray(fc_b)).to(dtype)
    if mode == "group":
        return _reference_forward(feats, fw, fb, positive, H, W).double().numpy()
    return np.stack([_reference_forward(feats[[0, k + 1]], fw, fb, positive, H, W).double().numpy()
                     for k in range(rows.shape[0] - 1)])


def ref32(rows, h, w, H, W, fc_w=None, fc_b=None, mode="group", positive=False):
    return ref_torch(rows, h, w, H, W, fc_w, fc_b, mode, positive, torch.float32)


def map_errors(got, exp):
    """Per map (the last two axes) max|got - exp| / max|exp| -> a flat list; NaN patterns must agree; an all-zero expected map
    must be matched exactly (ratio 0) or counts as inf."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    errs = []
    for g, e in zip(got.reshape(-1, *got.shape[-2:]), exp.reshape(-1, *exp.shape[-2:])):
        assert np.array_equal(np.isnan(g), np.isnan(e)), "NaN pattern differs"
        if np.isnan(e).all():
            errs.append(0.0)
            continue
        ok = ~np.isnan(e)
        scale, err = float(np.abs(e[ok]).max()), float(np.abs(g[ok] - e[ok]).max())
        errs.append(err / scale if scale > 0 else (0.0 if err == 0 else float("inf")))
    return errs


# ---- seeded kernel inputs ---------------------------------------------------------------------------------------------
def make_rows(seed, b, hw, c, d=None, spread=False):
    """(rows [b, hw, c] float32, fc_w, fc_b) as numpy.  rows are ReLU-like (non-negative, about a third exact zeros), each image
    scaled by its own factor in [0.5, 1.5].
    With an fc (d): W ~ N(0, 1 / c) plus a rank-one term that puts the embedding of the mean pooled vector at t[d], |t[d]| in
    [1, 2] with random signs, and a small bias.  An image's embedding is then t plus a variation of about a tenth of it: no
    component comes near zero (sign_margin_ok is asserted; the seed moves on otherwise), |xn_0 - xn_j| is not a difference of
    nearly equal numbers, and the maps are not clamped away entirely.
    spread: the rows of images 0 and 1 positive and every other image's negative, so that each further factor |xn_0 - xn_j| is
    about 2 / sqrt(c) -- with c = 4 a product over hundreds of images stays inside float32's range."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(seed + 7919 * attempt)
        rows = torch.randn(b, hw, c, generator=g)
        if spread:
            rows = rows.abs() + 0.25
            rows[2:] = -rows[2:]
        else:
            rows = (rows + 0.4).clamp(min=0) * (0.5 + torch.rand(b, 1, 1, generator=g))
        if d is None:
            return rows.numpy(), None, None
        fw = torch.randn(d, c, generator=g) / float(np.sqrt(c))
        pbar = rows.mean(dim=(0, 1))
        t = torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0) * (1.0 + torch.rand(d, generator=g))
        fw = fw + torch.outer(t - fw @ pbar, pbar / (pbar @ pbar))
        fb = 0.05 * torch.randn(d, generator=g)
        if sign_margin_ok(rows.numpy(), fw.numpy(), fb.numpy()):
            return rows.numpy(), fw.numpy(), fb.numpy()
    raise AssertionError("no seed satisfies the sign margin")


# ---- the fixture's models and cases (tests/golden/make_golden_simatt.py writes, tests/test_simatt_cpu.py reads) -------------
KERNEL = 2                     # the feature module is (AvgPool2d(2), ReLU): 10 x 14 images -> a 5 x 7 map
SIZE = (10, 14)
CHANNELS = 6
FC_DIM = 5

CASES = tuple(
    dict(name=f"{n}{'_fc' if fc else ''}", np_=p, nn_=q, fc=fc, zero_channel=z)
    for fc in (False, True)
    for n, p, q, z in (("ap", 1, 0, False), ("an", 0, 1, False), ("triplet", 1, 1, False), ("p1n2", 1, 2, False),
                       ("alone", 0, 0, False), ("p2n1", 2, 1, False))
) + (dict(name="ap_zero_channel", np_=1, nn_=0, fc=False, zero_channel=True),
     dict(name="triplet_zero_channel", np_=1, nn_=1, fc=False, zero_channel=True))


def flat_model(fc=None):
    """compute_saliency.py's recipe on a tiny model: Sequential(features, avgpool[, fc]), target "relu" inside model[0]."""
    return nn.Sequential(pool_features(KERNEL), nn.AdaptiveAvgPool2d((1, 1)), *([fc] if fc is not None else []))


def make_fc(weight, bias):
    fc = nn.Linear(CHANNELS, FC_DIM).double()
    with torch.no_grad():
        fc.weight.copy_(torch.as_tensor(weight))
        fc.bias.copy_(torch.as_tensor(bias))
    return fc


def case_inputs(case, gen):
    """float64 (x_q, x_p or None, x_n or None); zero_channel: channel 2 negative everywhere (dead after the ReLU)."""
    def draw(n):
        if n == 0:
            return None
        x = torch.randn(n, CHANNELS, *SIZE, generator=gen, dtype=torch.float64)
        if case["zero_channel"]:
            x[:, 2] = -x[:, 2].abs()
        return x
    return draw(1), draw(case["np_"]), draw(case["nn_"])


def case_rows(xq, xp, xn):
    """The rows the target layer sees: relu(2 x 2 block means) of cat(x_q, x_p, x_n), [B, h * w, C] float64, and (h, w)."""
    x = torch.cat([torch.as_tensor(np.asarray(t, np.float64)) for t in (xq, xp, xn) if t is not None])
    with torch.no_grad():
        f = torch.relu(nn.AvgPool2d(KERNEL)(x))
    return f.permute(0, 2, 3, 1).reshape(f.shape[0], -1, f.shape[1]).numpy(), tuple(f.shape[-2:])


def case_expected(xq, xp, xn, fc_w=None, fc_b=None):
    rows, (h, w) = case_rows(xq, xp, xn)
    if rows.shape[0] == 1:                                 # no other image: the product over zero rows is all ones
        x = embedding(rows, fc_w, fc_b)
        return _maps(rows, x, np.ones(x.shape[1]), h, w, SIZE[0], SIZE[1], fc_w)
    return simatt(rows, h, w, SIZE[0], SIZE[1], fc_w, fc_b, "group", positive=xp is not None)


# the driver forms that fail in the reference: name -> a builder of (model, feature_module, target_layers) given the classes' fc
class _Wrapper(nn.Module):
    """A model whose feature stack sits one level down (model.backbone[0]), like the reference's ResNet50 / ConvNeXtV2 wrappers."""

    def __init__(self):
        super().__init__()
        self.backbone = nn.Sequential(OrderedDict(stage=pool_features(KERNEL), avgpool=nn.AdaptiveAvgPool2d((1, 1))))

    def forward(self, x):
        return torch.flatten(self.backbone(x), 1)


def failing_form(name, fc=None):
    if name in ("children_seq", "children_seq_fc"):        # Sequential(*model.children()): model[0] = (features, avgpool)
        inner = nn.Sequential(pool_features(KERNEL))
        inner.add_module("avgpool", nn.AdaptiveAvgPool2d((1, 1)))
        model = nn.Sequential(inner, *([fc] if fc is not None else []))
        return model, model[0], ["relu"]
    if name == "nested_none":                              # SimAtt(model, <a nested layer>, target_layers=None)
        model = _Wrapper()
        return model, model.backbone.stage.relu, None
    if name == "direct_none":                              # the feature module a direct child, target_layers=None
        model = flat_model()
        return model, model[0], None
    raise KeyError(name)


FAILING = ("children_seq", "children_seq_fc", "nested_none", "direct_none")
