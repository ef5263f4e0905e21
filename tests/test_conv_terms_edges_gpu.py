"""mirx_conv_terms (k_conv_t2.hip) and its glue kernels off ResNet-50's 224 x 224 geometry: h != w, odd inputs under stride 2,
maps down to 1 x 1 (128 images in one pixel tile), cin / 32 in {1, 3, 5}, cout that leaves an output tile partly empty -- both
outputs of every launch against float64 with the project's bounds (_convterms_ref._run_and_check), and the kernel's promises
(an image's bits do not depend on its batch mates; a non-finite image stays contained) at those shapes."""
import pytest
import torch
import torch.nn.functional as F

from _convterms_ref import DEV, _conv_bn, _decode, _input, _out_hw, _pow2_scale, _run_and_check, _to_terms

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 1), (2, 2), (1, 40), (40, 1), (3, 5), (5, 3), (7, 7), (13, 13), (9, 14), (25, 13)]
ODD = [(3, 5), (5, 3), (7, 7), (13, 13), (9, 14), (25, 13)]          # an odd side of more than one pixel
KS = [(3, 1), (3, 2), (1, 1), (1, 2)]
CHANNELS = [(32, 32), (32, 96), (96, 64), (160, 128), (64, 160), (64, 192)]
TINY = [(1, 1), (2, 2)]                                              # also with layer4's (512, 512) and with n = 130

# (h, w, k, stride, cin, cout, n): a covering list, not the product
CASES = [
    (1, 1, 3, 1, 32, 32, 1), (1, 1, 3, 2, 32, 96, 37), (1, 1, 1, 1, 96, 64, 3), (1, 1, 1, 2, 160, 128, 1),
    (2, 2, 3, 1, 32, 96, 3), (2, 2, 3, 2, 96, 64, 1), (2, 2, 1, 1, 160, 128, 37), (2, 2, 1, 2, 64, 160, 3),
    (1, 40, 3, 1, 96, 64, 37), (1, 40, 3, 2, 160, 128, 3), (1, 40, 1, 1, 64, 160, 1), (1, 40, 1, 2, 64, 192, 37),
    (40, 1, 3, 1, 160, 128, 1), (40, 1, 3, 2, 64, 160, 37), (40, 1, 1, 1, 64, 192, 3), (40, 1, 1, 2, 32, 32, 1),
    (3, 5, 3, 1, 64, 160, 3), (3, 5, 3, 2, 64, 192, 1), (3, 5, 1, 1, 32, 32, 37), (3, 5, 1, 2, 32, 96, 3),
    (5, 3, 3, 1, 64, 192, 37), (5, 3, 3, 2, 32, 32, 3), (5, 3, 1, 1, 32, 96, 1), (5, 3, 1, 2, 96, 64, 37),
    (7, 7, 3, 1, 32, 32, 1), (7, 7, 3, 2, 32, 96, 37), (7, 7, 1, 1, 96, 64, 3), (7, 7, 1, 2, 160, 128, 1),
    (13, 13, 3, 1, 32, 96, 3), (13, 13, 3, 2, 96, 64, 1), (13, 13, 1, 1, 160, 128, 37), (13, 13, 1, 2, 64, 160, 3),
    (9, 14, 3, 1, 96, 64, 37), (9, 14, 3, 2, 160, 128, 3), (9, 14, 1, 1, 64, 160, 1), (9, 14, 1, 2, 64, 192, 37),
    (25, 13, 3, 1, 160, 128, 1), (25, 13, 3, 2, 64, 160, 37), (25, 13, 1, 1, 64, 192, 3), (25, 13, 1, 2, 32, 32, 1),
    # layer4's widths on the maps an 8 x 8 image produces, and more than 128 images in a tile
    (1, 1, 3, 1, 512, 512, 130), (1, 1, 3, 2, 512, 512, 3), (1, 1, 1, 1, 512, 512, 37), (1, 1, 1, 2, 512, 512, 130),
    (2, 2, 3, 1, 512, 512, 130), (2, 2, 3, 2, 512, 512, 37), (2, 2, 1, 1, 512, 512, 3), (2, 2, 1, 2, 512, 512, 130),
    (1, 1, 1, 1, 64, 160, 130), (1, 1, 3, 2, 64, 192, 130), (2, 2, 3, 2, 32, 32, 130), (2, 2, 1, 1, 96, 64, 130),
]


def _covering_holds():
    """the conditions the list was built to: a later edit cannot thin it out unnoticed"""
    assert len(set(CASES)) == len(CASES)
    for g in GEOMETRIES:
        mine = [c for c in CASES if c[:2] == g]
        assert len({c[4:6] for c in mine}) >= 2, g                            # at least two channel pairs per geometry
        assert {c[2:4] for c in mine} == set(KS), g                           # every (k, stride) with every geometry
        assert {1, 3, 37} <= {c[6] for c in mine}, g                          # every batch size with every geometry
    for p in CHANNELS:
        mine = [c for c in CASES if c[4:6] == p]
        assert len({c[:2] for c in mine}) >= 4, p                             # at least four geometries per channel pair
        assert any(c[:2] in ODD and c[2:4] == (3, 2) for c in mine), p        # .. one of them an odd input under k 3 stride 2
        assert any(c[2:4] == (1, 2) for c in mine), p                         # .. and one k 1 stride 2
    for g in TINY:
        mine = [c for c in CASES if c[:2] == g]
        assert {c[2:4] for c in mine if c[4:6] == (512, 512)} == set(KS), g
        assert {c[2:4] for c in mine if c[6] == 130} == set(KS), g
    assert all(c[:2] in TINY for c in CASES if c[4:6] == (512, 512) or c[6] == 130)
    assert all(c[:2] in GEOMETRIES and c[2:4] in KS and c[4:6] in CHANNELS + [(512, 512)] for c in CASES)


_covering_holds()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_k%ds%d_c%d-%d_n%d" % c)
def test_conv_terms_edge_geometries(case):
    """plain and +residual +ReLU, images of magnitudes 1e-3 / 1 / 1e3 cycled, both outputs of one launch against float64"""
    h, w, k, s, cin, cout, n = case
    loose = []
    a = _run_and_check((cin, cout, k, s, h, w), n, 11, (1e-3, 1.0, 1e3), res=False, relu=False, report=loose)
    b = _run_and_check((cin, cout, k, s, h, w), n, 12, (1e3, 1e-3, 1.0), res=True, relu=True, report=loose)
    print("case", case, "bound / max|y| %.1f .. %.1f," % (min(loose), max(loose)), "largest error / bound:",
          ", ".join("%s %.3f" % (key, max(a[key], b[key])) for key in a))


# ---- the kernel's promises at these shapes ----------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rows_of(t, b, rows):
    """image b of a (terms rows, scale row, range row) triple"""
    return t[0][b * rows:(b + 1) * rows], t[1][b:b + 1], t[2][b:b + 1]


def _image_out(out, b, rows):
    """(terms rows, y_scale, y_range, fp32 rows) of image b of a launch"""
    yt, ys, yr, y = out[:4]
    return yt[b * rows:(b + 1) * rows], ys[b:b + 1], yr[b:b + 1], y[b * rows:(b + 1) * rows]


# (h, w, k, stride, cin, cout, n, a NaN image, an image of range 1e30): 128 images in the first tile and 2 in the second; six
# output pixels per image, so that 16-pixel accumulator columns and 128-pixel tiles straddle images
PROMISE = [(1, 1, 3, 1, 512, 512, 130, 126, 129), (3, 5, 3, 2, 96, 64, 37, 7, 20)]


def _promise_setup(case):
    from mirx.model import _conv_terms_weights
    h, w, k, s, cin, cout, n = case[:7]
    conv, bn = _conv_bn(cin, cout, k, s, 41)
    cw = _conv_terms_weights(conv.to(DEV), bn.to(DEV))
    x = _input(n, (h, w), cin, 42, (1e-3, 1.0, 1e3))
    ho, wo = _out_hw((h, w), k, s)
    rg, _ = _to_terms(_input(n, (ho, wo), cout, 43, (1e3, 1e-3, 1.0)))
    return cw, x, rg, ho * wo


@pytest.mark.parametrize("case", PROMISE, ids=lambda c: "%dx%d_n%d" % (c[0], c[1], c[6]))
def test_batch_independence_at_kernel_level(case):
    """images 0, 127 / 128 (either side of a tile boundary at 1 x 1) and the last, launched alone: every output bit-identical"""
    from mirx.model import conv_terms
    h, w, n = case[0], case[1], case[6]
    cw, x, rg, hwo = _promise_setup(case)
    xg, _ = _to_terms(x)
    full = conv_terms(cw, xg, h, w, res=rg, relu=True, terms_out=True, fp32_out=True)
    for b in sorted({0, 127 % n, 128 % n, n - 1}):
        one = conv_terms(cw, _rows_of(xg, b, h * w), h, w, res=_rows_of(rg, b, hwo), relu=True, terms_out=True, fp32_out=True)
        for got, want in zip(_image_out(one, 0, hwo), _image_out(full, b, hwo)):
            assert _same_bits(got, want), (case, b)
    assert torch.isfinite(full[2]).all() and bool((full[2] > 0).all())


@pytest.mark.parametrize("case", PROMISE, ids=lambda c: "%dx%d_n%d" % (c[0], c[1], c[6]))
def test_containment_at_kernel_level(case):
    """one image's terms built from NaN (scale and range NaN, as the device writes them), one with range 1e30: every other image's
    four outputs keep their bits, the NaN image's range and rows are non-finite"""
    from mirx.model import conv_terms
    h, w, n, nan, big = case[0], case[1], case[6], case[7], case[8]
    cw, x, rg, hwo = _promise_setup(case)
    xg, _ = _to_terms(x)
    clean = conv_terms(cw, xg, h, w, res=rg, relu=True, terms_out=True, fp32_out=True)
    bad = x.clone()
    bad[nan] = float("nan")
    bad[big] = x[big] * (1e30 / float(x[big].abs().max()))
    bg, _ = _to_terms(bad)
    bg[1][nan] = float("nan")
    assert abs(float(bg[2][big]) / 1e30 - 1.0) < 1e-6 and bool(torch.isnan(bg[2][nan]))
    dirty = conv_terms(cw, bg, h, w, res=rg, relu=True, terms_out=True, fp32_out=True)
    for b in range(n):
        if b in (nan, big):
            continue
        for got, want in zip(_image_out(dirty, b, hwo), _image_out(clean, b, hwo)):
            assert _same_bits(got, want), (case, b)
    yt, ys, yr, y = _image_out(dirty, nan, hwo)
    assert not torch.isfinite(yr).any() and not torch.isfinite(ys).any()
    assert not torch.isfinite(y).any() and not torch.isfinite(yt.float()).any()


def test_outputs_one_at_a_time():
    """a terms-only and an fp32-only launch against the launch that writes both (cout = 96: the wide arm, a quarter empty)"""
    from mirx.model import _conv_terms_weights, conv_terms
    h, w, k, s, cin, cout, n = 5, 3, 3, 2, 32, 96, 3
    conv, bn = _conv_bn(cin, cout, k, s, 51)
    cw = _conv_terms_weights(conv.to(DEV), bn.to(DEV))
    xg, _ = _to_terms(_input(n, (h, w), cin, 52, (1e-3, 1.0, 1e3)))
    ho, wo = _out_hw((h, w), k, s)
    rg, _ = _to_terms(_input(n, (ho, wo), cout, 53, (1e3, 1e-3, 1.0)))
    yt, ys, yr, y, _, _ = conv_terms(cw, xg, h, w, res=rg, relu=True, terms_out=True, fp32_out=True)
    t_yt, t_ys, t_yr, t_y, _, _ = conv_terms(cw, xg, h, w, res=rg, relu=True, terms_out=True, fp32_out=False)
    f_yt, f_ys, f_yr, f_y, _, _ = conv_terms(cw, xg, h, w, res=rg, relu=True, terms_out=False, fp32_out=True)
    assert t_y is None and f_yt is None and f_ys is None
    assert _same_bits(t_yt, yt) and _same_bits(t_ys, ys) and _same_bits(t_yr, yr)
    assert _same_bits(f_y, y) and _same_bits(f_yr, yr)
    assert bool((yr > 0).all())


# ---- glue kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [32, 64, 96])
@pytest.mark.parametrize("hw", [1, 63, 64, 65, 130])
def test_nchw_to_terms_tails_and_batch_stride(hw, c):
    """p >= hw tail, one to three channel groups per wave, images c * hw + 8 floats apart with NaN in the gap; image 4 all zero
    and image 5 with a range row of 0 (scale exactly 1, small integers come back exactly)"""
    from mirx import _lib
    from mirx.model import _ptr, _stream
    n = 6
    g = torch.Generator().manual_seed(4 + hw + c)
    x = torch.randn(n, c, hw, generator=g) * torch.tensor([1e-3, 1.0, 1e3, 7.0, 0.0, 1.0]).view(n, 1, 1)
    x[5] = torch.randint(-4, 5, (c, hw), generator=g).float()
    buf = torch.full((n, c * hw + 8), float("nan"))
    buf[:, :c * hw] = x.reshape(n, -1)
    bg = buf.to(DEV)
    rng = x.abs().reshape(n, -1).amax(dim=1)
    rng[5] = 0.0
    rg = rng.to(DEV)
    xt = torch.full((n * hw, 2 * c), float("nan"), dtype=torch.float16, device=DEV)
    sc = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mirx_nchw_to_terms(_ptr(bg), c * hw + 8, n, c, hw, _ptr(rg), _ptr(sc), _ptr(xt), _stream(bg.device)))
    torch.cuda.synchronize()
    assert torch.isfinite(xt.float()).all()                      # every element written, nothing from the gap
    assert torch.equal(sc.cpu().double(), _pow2_scale(rng.double()))
    assert float(sc[4]) == 1.0 and float(sc[5]) == 1.0
    dec = _decode(xt, sc, n)
    ref = x.double().permute(0, 2, 1)
    for b in range(5):
        assert float((dec[b] - ref[b]).abs().max()) <= 2.0 ** -21 * float(rng[b]), b
    assert torch.equal(dec[5], ref[5]) and not dec[4].any()


def _gap(x, normalize):
    from mirx import _lib
    from mirx.model import _ptr, _stream
    n, hw, c = x.shape
    xg = x.to(DEV)
    y = torch.full((n, c), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mirx_gap_nhwc_l2norm(_ptr(xg), n, hw, c, normalize, _ptr(y), _stream(xg.device)))
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("hw,c", [(1, 4), (1, 2048), (6, 1028), (49, 2048), (130, 96)])
def test_gap_nhwc_head_shapes(hw, c, normalize):
    """one thread with work (c = 4), a second trip of the channel loop (c = 1028), one pixel, 130 pixels; an all-zero image under
    normalisation gives 0 (the 1e-12 clamp), a NaN image leaves the rows of the others as they were"""
    n = 6
    x = torch.randn(n, hw, c, generator=torch.Generator().manual_seed(5 + hw + c)).abs()
    x = x * torch.tensor([1e-3, 1.0, 0.0, 1e3, 7.0, 1.0]).view(n, 1, 1)
    y = _gap(x, normalize)
    ref = x.double().mean(dim=1)
    if normalize:
        ref = F.normalize(ref, dim=1)
    assert not y[2].any() and not ref[2].any()
    for b in range(n):
        assert float((y[b].double() - ref[b]).abs().max()) <= 1e-6 * float(ref[b].abs().max()), b
    bad = x.clone()
    bad[3] = float("nan")
    yb = _gap(bad, normalize)
    keep = [0, 1, 2, 4, 5]
    assert _same_bits(yb[keep], y[keep])
    assert not torch.isfinite(yb[3]).any()
