"""The helpers of the terms-convolution tests, checked where they are about to be trusted, with no kernel involved: the float64
reference convolution against a plain loop written from include/mirx.h (mirx_conv_terms), the host terms rows against the values
they encode, and a float64 restatement of the kernel's sum from the two operand images (pixel terms rows, weight terms rows)."""
import numpy as np
import pytest
import torch

from _convterms_ref import (_conv_bn, _decode, _input, _kernel_out_scale, _out_hw, _pow2_scale, _ref_conv,
                            _to_terms)

# the tiny geometries of test_conv_terms_edges_gpu.py
GEOMETRIES = [(1, 1), (2, 2), (1, 40), (40, 1), (3, 5), (5, 3), (7, 7), (13, 13), (9, 14), (25, 13)]
KS = [(3, 1), (3, 2), (1, 1), (1, 2)]


def _loop_conv(x, wf, bias, hw, k, s, res, relu):
    """y[b, oy, ox, o] = relu?( sum_{ky, kx, c} x[b, s oy + ky - p, s ox + kx - p, c] W[o, ky, kx, c] + bias[o] (+ res) ),
    p = (k - 1) / 2, ho = (h + 2 p - k) / s + 1; taps outside the map read zeros.  numpy float64, one pixel and tap at a time."""
    n, _, cin = x.shape
    h, w = hw
    p = (k - 1) // 2
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    cout = wf.shape[0]
    xm = x.reshape(n, h, w, cin)
    y = np.zeros((n, ho, wo, cout))
    for b in range(n):
        for oy in range(ho):
            for ox in range(wo):
                acc = np.zeros(cout)
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = s * oy + ky - p, s * ox + kx - p
                        if 0 <= iy < h and 0 <= ix < w:
                            acc += wf[:, :, ky, kx] @ xm[b, iy, ix]
                y[b, oy, ox] = acc + bias
    y = y.reshape(n, ho * wo, cout)
    if res is not None:
        y = y + res
    return np.maximum(y, 0.0) if relu else y


@torch.no_grad()
def _folded(conv, bn):
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.double() - bn.running_mean.double() * scale
    return (conv.weight.detach().double() * scale.view(-1, 1, 1, 1)).numpy(), shift.detach().numpy()


@pytest.mark.parametrize("k,s", KS, ids=lambda v: str(v))
@pytest.mark.parametrize("hw", GEOMETRIES, ids=lambda v: "%dx%d" % v)
def test_reference_conv_matches_the_formula(hw, k, s):
    cin, cout, n = 5, 6, 2
    conv, bn = _conv_bn(cin, cout, k, s, 100 + hw[0])
    x = _input(n, hw, cin, 7, (1e-3, 1e3))
    ho, wo = _out_hw(hw, k, s)
    res = _input(n, (ho, wo), cout, 8, (1e3, 1e-3))
    wf, bias = _folded(conv, bn)
    for r, relu in ((None, False), (res, True)):
        got = _ref_conv(x, conv, bn, hw, r, relu).numpy()
        want = _loop_conv(x.numpy(), wf, bias, hw, k, s, None if r is None else r.numpy(), relu)
        assert got.shape == want.shape == (n, ho * wo, cout)
        for b in range(n):
            assert np.abs(got[b] - want[b]).max() <= 1e-13 * np.abs(want[b]).max(), (hw, k, s, b)


def test_out_hw_of_the_odd_chains():
    """100 x 100 -> 25 -> 13 -> 7 -> 4 and 36 x 52 -> 9 x 13 -> 5 x 7 -> 3 x 4 -> 2 x 2 (k 3 and k 1 agree at stride 2)"""
    for k in (1, 3):
        assert [_out_hw((v, v), k, 2)[0] for v in (25, 13, 7)] == [13, 7, 4]
        assert [_out_hw(v, k, 2) for v in ((9, 13), (5, 7), (3, 4))] == [(5, 7), (3, 4), (2, 2)]
        assert _out_hw((1, 40), k, 2) == (1, 20) and _out_hw((1, 1), k, 2) == (1, 1) and _out_hw((9, 14), k, 1) == (9, 14)


@pytest.mark.parametrize("c", [32, 96, 160])
def test_terms_rows_round_trip(c):
    n, rows = 5, 13
    x = _input(n, (1, rows), c, c, (1e-3, 1.0, 1e3, 7.0))
    x[4] = 0.0                                              # an all-zero image: scale exactly 1
    (t, s, r), xd = _to_terms(x, "cpu")
    assert t.shape == (n * rows, 2 * c) and t.dtype == torch.float16
    assert torch.equal(s.double(), _pow2_scale(x.abs().reshape(n, -1).amax(dim=1))) and float(s[4]) == 1.0
    assert torch.equal(_decode(t, s, n), xd)
    for b in range(n):
        rng = float(r[b])
        assert rng == float(x[b].float().abs().max())
        assert float((xd[b] - x[b]).abs().max()) <= 2.0 ** -21 * rng, b
        if rng > 0:
            assert 2.0 ** 14 <= rng * float(s[b]) < 2.0 ** 15


def test_kernel_out_scale_is_the_power_of_two_of_the_fp32_bound():
    xr = torch.tensor([1e-3, 1.0, 1e3, 0.0, 3.0])
    rr = torch.tensor([2.0, 0.5, 0.0, 0.0, 1.0])
    got = _kernel_out_scale(xr, 7.5, 0.25, rr)
    b = (xr * 7.5 + 0.25 + rr).double()
    assert np.array_equal(got, _pow2_scale(b).float().numpy())
    assert got[4] == 2.0 ** (14 - 4) and _kernel_out_scale(torch.zeros(1), 3.0, 0.0)[0] == 1.0
    # one fp32 rounding per operation: 2^24 - 1 + 0.5 rounds up to 2^24, an exponent above the exact sum's
    assert _kernel_out_scale(torch.tensor([2.0 ** 24 - 1]), 1.0, 0.5)[0] == 2.0 ** (14 - 24)


@pytest.mark.parametrize("hw,k,s", [((3, 5), 3, 2), ((2, 2), 3, 1), ((5, 3), 1, 2), ((1, 1), 3, 1)], ids=str)
@pytest.mark.parametrize("cin,cout", [(32, 32), (32, 96), (96, 160), (64, 192)], ids=str)
def test_kernel_sum_restated_from_both_operand_images(hw, k, s, cin, cout):
    """oscale[o] / x_scale[b] * sum over (ky, kx, c) of the pixel terms times the weight terms, + bias, in float64 from the images
    the kernel reads (the weight image of _conv_terms_weights: K order (ky, kx, c), rows padded with zeros to a multiple of 128)
    within 1e-6 max |ref_b| of the reference."""
    from mirx.model import _conv_terms_weights
    n = 3
    conv, bn = _conv_bn(cin, cout, k, s, 31)
    cw = _conv_terms_weights(conv, bn)
    assert (cw["k"], cw["s"], cw["cin"], cw["cout"]) == (k, s, cin, cout)
    wt = cw["wt"]
    kdim = k * k * cin
    rows = wt.shape[0]
    assert rows % 128 == 0 and rows - 128 < cout <= rows and wt.numel() == rows * 2 * kdim
    w2 = wt.view(rows, kdim // 32, 2, 32).double().sum(dim=2).reshape(rows, k, k, cin)      # [o, ky, kx, c] of W * ws
    assert not w2[cout:].any()
    (xt, xs, xr), xd = _to_terms(_input(n, hw, cin, 32, (1e-3, 1.0, 1e3)), "cpu")
    xv = xt.view(n, hw[0], hw[1], cin // 32, 2, 32).double().sum(dim=4).reshape(n, hw[0], hw[1], cin)   # s_b * x
    h, w = hw
    p = (k - 1) // 2
    ho, wo = _out_hw(hw, k, s)
    acc = torch.zeros(n, ho, wo, rows, dtype=torch.float64)
    for oy in range(ho):
        for ox in range(wo):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = s * oy + ky - p, s * ox + kx - p
                    if 0 <= iy < h and 0 <= ix < w:
                        acc[:, oy, ox] += xv[:, iy, ix] @ w2[:, ky, kx].t()
    y = acc[..., :cout] * cw["osc"].double() / xs.double().view(n, 1, 1, 1) + cw["bias"].double()
    ref = _ref_conv(xd, conv, bn, hw)
    y = y.reshape(n, ho * wo, cout)
    for b in range(n):
        mref = float(ref[b].abs().max())
        assert float((y[b] - ref[b]).abs().max()) <= 1e-6 * mref, (b, float((y[b] - ref[b]).abs().max()) / mref)
    # the host constants of the output bound
    wf, bias = _folded(conv, bn)
    assert abs(cw["wsum"] - np.abs(wf).reshape(cout, -1).sum(axis=1).max()) <= 1e-5 * cw["wsum"]
    assert abs(cw["bmax"] - np.abs(bias).max()) <= 1e-6
