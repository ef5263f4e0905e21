"""Shared helpers of the terms-convolution tests (mirx_conv_terms, k_conv_t2.hip): terms rows on the host, a float64 reference
of one convolution + folded BatchNorm (+ residual, ReLU) on an h x w map, and the launch-and-compare routine with the project's
three bounds.  Every geometry is (h, w); nothing here assumes a square map."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

DEV = "cuda"


def _pow2_scale(b):
    """2^(14 - floor(log2 b)) per element of b (float64 tensor), 1 where b == 0."""
    e = torch.floor(torch.log2(torch.where(b > 0, b, torch.ones_like(b))))
    return torch.where(b > 0, torch.exp2(14 - e), torch.ones_like(b))


def _to_terms(x, dev=None):
    """x float64 [n, rows, c] -> (terms rows fp16 [n * rows, 2 c], scale row, range row) on `dev` (the GPU by default), image b
    scaled by the power of two that puts its max |x| in [2^14, 2^15), and the exactly represented values (float64) the kernel
    reads."""
    from mirx.model import _terms_of
    dev = DEV if dev is None else dev
    n, rows, c = x.shape
    amax = x.abs().reshape(n, -1).amax(dim=1)
    s = _pow2_scale(amax)
    t = torch.cat([_terms_of(x[b].float(), float(s[b])).reshape(rows, 2 * c) for b in range(n)])
    return (t.to(dev), s.float().to(dev), amax.float().to(dev)), _decode(t, s, n)


def _decode(t, s, n):
    """terms rows [n * rows, 2 c] (any device), scale row [n] -> float64 [n, rows, c]."""
    t = t.cpu()
    rows = t.shape[0] // n
    c = t.shape[1] // 2
    v = t.view(n, rows, c // 32, 2, 32).double()
    return ((v[:, :, :, 0] + v[:, :, :, 1]) / s.cpu().double().view(n, 1, 1, 1)).reshape(n, rows, c)


def _conv_bn(cin, cout, k, s, seed):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(cin, cout, k, stride=s, padding=(k - 1) // 2, bias=False)
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * math.sqrt(2.0 / (cin * k * k)))
        bn.weight.copy_(0.75 + 0.5 * torch.rand(cout, generator=g))
        bn.bias.copy_(0.1 * torch.randn(cout, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(cout, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(cout, generator=g))
    return conv.eval(), bn.eval()


def _out_hw(hw, k, s):
    """(ho, wo) of include/mirx.h: p = (k - 1) / 2, ho = (h + 2 p - k) / s + 1."""
    p = (k - 1) // 2
    return (hw[0] + 2 * p - k) // s + 1, (hw[1] + 2 * p - k) // s + 1


def _ref_conv(xd, conv, bn, hw, res_d=None, relu=False):
    """float64: xd [n, h * w, cin] -> [n, ho * wo, cout]; hw = (h, w)"""
    with torch.no_grad():
        return _ref_conv_(xd, conv, bn, hw, res_d, relu)


def _ref_conv_(xd, conv, bn, hw, res_d, relu):
    n, _, cin = xd.shape
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.double() - bn.running_mean.double() * scale
    w = conv.weight.detach().double() * scale.view(-1, 1, 1, 1)
    xi = xd.view(n, hw[0], hw[1], cin).permute(0, 3, 1, 2)
    y = F.conv2d(xi, w, stride=conv.stride, padding=conv.padding) + shift.view(1, -1, 1, 1)
    y = y.permute(0, 2, 3, 1).reshape(n, -1, w.shape[0])
    if res_d is not None:
        y = y + res_d
    return F.relu(y) if relu else y


def _input(n, hw, c, seed, mags):
    """float64 [n, h * w, c], image b of magnitude mags[b % len(mags)]"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hw[0] * hw[1], c, generator=g, dtype=torch.float64)
    x = x * torch.tensor([mags[b % len(mags)] for b in range(n)], dtype=torch.float64).view(n, 1, 1)
    return x


def _kernel_out_scale(x_range, wsum, bmax, res_range=None):
    """y_scale as k_conv_t2 evaluates it: bound_b = x_range[b] * w_abs_sum + bias_abs_max (+ res_range[b]) in fp32, one rounding
    per operation (the library is built without contraction), then 2^(14 - floor(log2 bound_b)) from the exponent field
    (mirx_device.h, range_scales).  x_range / res_range: fp32 rows of finite values; -> float32 numpy row."""
    xr = x_range.detach().cpu().numpy().astype(np.float32)
    bound = xr * np.float32(wsum) + np.float32(bmax)
    bound = bound + (res_range.detach().cpu().numpy().astype(np.float32) if res_range is not None else np.float32(0.0))
    assert bound.dtype == np.float32 and np.isfinite(bound).all()
    e = ((bound.view(np.uint32) >> 23) & 0xff).astype(np.int64) - 127
    return np.where(e < -100, 1.0, np.exp2((14 - e).astype(np.float64))).astype(np.float32)


def _run_and_check(shape, n, seed, mags, res, relu, report=None):
    """shape = (cin, cout, k, stride, h, w).  One launch with both outputs against float64: fp32 rows within 1e-6 max |ref_b| per
    image, decoded terms rows within 2^-20 bound_b, y_range[b] within 1e-6 of max |ref_b|, y_scale[b] exactly the power of two
    of bound_b.  -> the largest error / bound of the launch for each of the three bounds (for a test to print)."""
    from mirx.model import _conv_terms_weights, conv_terms
    cin, cout, k, s, h, w = shape
    conv, bn = _conv_bn(cin, cout, k, s, seed)
    cw = _conv_terms_weights(conv.to(DEV), bn.to(DEV))
    xg, xd = _to_terms(_input(n, (h, w), cin, seed + 1, mags))
    ho, wo = _out_hw((h, w), k, s)
    rg = rd = None
    if res:
        rg, rd = _to_terms(_input(n, (ho, wo), cout, seed + 2, mags[::-1]))
    yt, ys, yr, y, h2, w2 = conv_terms(cw, xg, h, w, res=rg, relu=relu, terms_out=True, fp32_out=True)
    torch.cuda.synchronize()
    assert (h2, w2) == (ho, wo)
    ref = _ref_conv(xd, conv.cpu(), bn.cpu(), (h, w), rd, relu)
    yf = y.cpu().double().view(n, ho * wo, cout)
    ydec = _decode(yt, ys, n)
    wsum = float(cw["wsum"])
    want_ys = _kernel_out_scale(xg[2], wsum, cw["bmax"], rg[2] if res else None)
    assert np.array_equal(ys.cpu().numpy(), want_ys), (shape, n, ys.cpu().numpy(), want_ys)
    xr, rr, yrc = xg[2].cpu(), (rg[2].cpu() if res else None), yr.cpu()
    worst = {"fp32": 0.0, "terms": 0.0, "range": 0.0}
    for b in range(n):
        mref = float(ref[b].abs().max())
        err = float((yf[b] - ref[b]).abs().max())
        assert err <= 1e-6 * mref, (shape, n, b, err / mref)
        bound = float(xr[b]) * wsum + cw["bmax"] + (float(rr[b]) if res else 0.0)
        terr = float((ydec[b] - ref[b]).abs().max())
        assert terr <= 2.0 ** -20 * bound, (shape, n, b, terr / bound)
        assert abs(float(yrc[b]) - mref) <= 1e-6 * mref, (shape, b, float(yrc[b]), mref)
        if report is not None:
            report.append(bound / mref)
        worst = {"fp32": max(worst["fp32"], err / (1e-6 * mref)), "terms": max(worst["terms"], terr / (2.0 ** -20 * bound)),
                 "range": max(worst["range"], abs(float(yrc[b]) - mref) / (1e-6 * mref))}
    return worst
