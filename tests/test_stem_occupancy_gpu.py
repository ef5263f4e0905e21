"""The two-fp16-term stem (k_stem_h2) after its LDS diet: weights through a two-buffer DMA ring, the conv tile one channel
block at a time over the patch and the ring, the 8-bit table in a ring buffer.  Both entry points are called at kernel
level on 224 x 224 images, the size the model feeds them, at batches 1 (one image, plain order), 3 (the plain-order branch
of the XCD re-deal) and 9 (eight re-dealt images and one in plain order).

Tolerance against the float64 restatement: atol 2e-4, rtol 1e-4 -- what tests/test_model_gpu.py::test_stem_kernel asks
of the stem kernels on the same map."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import densenet as OD

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 9)
NMAX = max(BATCHES)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Stem:
    """Seed-0 DenseNet-121 stem weights out of the model's inference cache, and the two launches."""

    def __init__(self):
        from mirx import _lib
        from mirx.model import DenseNet121
        torch.manual_seed(0)
        m = DenseNet121().eval()
        sd = OD.randomize_bn_stats(m.state_dict(), seed=1)
        m.load_state_dict(sd)
        self.sd = {k: v.cpu() for k, v in sd.items()}
        self.m = m.cuda()
        self.lib, self.check = _lib.load(), _lib.check
        cache = self.m._cache()
        if "conv0_w2" not in cache:
            self.m._prepare_h2(cache)
        self.w2, self.osc = cache["conv0_w2"]
        self.sc, self.sh = cache["norm0"]
        torch.cuda.synchronize()

    def normalise(self, u):
        """ToTensor + Normalize with host operations on a host tensor, as the reference applies them (a device division by
        the scalar 255 is a multiplication by its reciprocal: other bits)"""
        assert not u.is_cuda
        return self.m.normalize_uint8(u)

    def _out(self, n):
        # NaN-filled: a pooled value the kernel fails to write shows
        return torch.full((n, 64, 56, 56), float("nan"), device="cuda"), torch.zeros(n, device="cuda")

    def run(self, x):
        """float entry point on normalised fp32 images -> (pooled map, range row), both on the host"""
        x = x.cuda().contiguous()
        n = x.shape[0]
        rin = x.abs().amax(dim=(1, 2, 3)).contiguous()
        y, rout = self._out(n)
        self.check(self.lib.mirx_stem_conv7_bn_relu_pool_split2h_into(_vp(x), _vp(self.w2), _vp(self.osc), _vp(self.sc),
                                                                      _vp(self.sh), n, 224, 224, _vp(y), 64 * 56 * 56,
                                                                      _vp(rin), _vp(rout), None), "stem")
        torch.cuda.synchronize()
        return y.cpu(), rout.cpu()

    def run_u8(self, u):
        """uint8 entry point on raw bytes (a host tensor); the input range is that of the normalised tensor"""
        n = u.shape[0]
        rin = self.normalise(u).abs().amax(dim=(1, 2, 3)).cuda().contiguous()
        u = u.cuda().contiguous()
        y, rout = self._out(n)
        self.check(self.lib.mirx_stem_conv7_bn_relu_pool_split2h_u8_into(_vp(u), _vp(self.m.input_mean), _vp(self.m.input_std),
                                                                         _vp(self.w2), _vp(self.osc), _vp(self.sc), _vp(self.sh),
                                                                         n, 224, 224, _vp(y), 64 * 56 * 56, _vp(rin), _vp(rout),
                                                                         None), "stem_u8")
        torch.cuda.synchronize()
        return y.cpu(), rout.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def stem():
    return _Stem()


@pytest.fixture(scope="module")
def images():
    return torch.randn(NMAX, 3, 224, 224, generator=torch.Generator().manual_seed(224))


@pytest.fixture(scope="module")
def reference(stem, images):
    """conv2d 7x7 / 2 p3, folded norm0, ReLU, max-pool 3 / 2 / 1 in float64 on the CPU, once for the largest batch (ranges are
    per image: image b of a smaller batch has the same reference)"""
    sd, p = stem.sd, OD.PFX
    g, b_ = sd[p + "norm0.weight"].double(), sd[p + "norm0.bias"].double()
    mu, var = sd[p + "norm0.running_mean"].double(), sd[p + "norm0.running_var"].double()
    scale = g / torch.sqrt(var + 1e-5)
    shift = b_ - mu * scale
    c = F.conv2d(images.double(), sd[p + "conv0.weight"].double(), None, stride=2, padding=3)
    c = F.relu(c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    return F.max_pool2d(c, kernel_size=3, stride=2, padding=1)


@pytest.fixture(scope="module")
def clean9(stem, images):
    return stem.run(images)


@pytest.mark.parametrize("n", BATCHES)
def test_stem_matches_float64(stem, images, reference, n):
    y, rout = stem.run(images[:n])
    err = (y.double() - reference[:n]).abs()
    print(f"STEM_OCC n={n} max abs err {float(err.max()):.3e} at max |ref| {float(reference[:n].abs().max()):.3e}")
    torch.testing.assert_close(y, reference[:n].float(), atol=2e-4, rtol=1e-4)
    # the range row is the largest pooled value of every image, to the bit
    assert _same_bits(rout, y.amax(dim=(1, 2, 3)))


@pytest.mark.parametrize("n", BATCHES)
def test_uint8_entry_point_is_bit_identical_to_the_float_one(stem, n):
    u = torch.randint(0, 256, (n, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(8 + n))
    y8, r8 = stem.run_u8(u)
    yf, rf = stem.run(stem.normalise(u))
    assert not torch.isnan(yf).any()
    assert _same_bits(y8, yf)
    assert _same_bits(r8, rf)


def test_ranges_are_per_image(stem, images, clean9):
    y0, r0 = clean9
    x = images.clone()
    x[4] *= 40.0
    y, r = stem.run(x)
    keep = [b for b in range(NMAX) if b != 4]
    assert _same_bits(y[keep], y0[keep]) and _same_bits(r[keep], r0[keep])
    assert not _same_bits(y[4], y0[4])


def test_repeated_launches_give_the_same_bits(stem, images, clean9):
    """the half tile lies over the patch and the ring, the table over a ring buffer, and the chunks hand over at barriers:
    a race there would show as bits that change from launch to launch"""
    y0, r0 = clean9
    u = torch.randint(0, 256, (NMAX, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(99))
    y80, r80 = stem.run_u8(u)
    for _ in range(20):
        y, r = stem.run(images)
        assert _same_bits(y, y0) and _same_bits(r, r0)
        y8, r8 = stem.run_u8(u)
        assert _same_bits(y8, y80) and _same_bits(r8, r80)


def test_a_non_finite_image_is_contained(stem, images, clean9):
    y0, r0 = clean9
    x = images.clone()
    x[8, 1, 100, 17] = float("inf")                       # image 8: the one in plain order
    x[2, 0, 0, 0] = float("-inf")                         # image 2: a re-dealt one
    y, r = stem.run(x)
    for b in (2, 8):
        assert torch.isnan(y[b]).all() and torch.isnan(r[b])
    keep = [b for b in range(NMAX) if b not in (2, 8)]
    assert _same_bits(y[keep], y0[keep]) and _same_bits(r[keep], r0[keep])
