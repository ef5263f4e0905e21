"""mirx.sbsm on the GPU: the three kernels against torch's own product (compose, bit for bit) and the float64 restatement
(tests/_sbsm_ref.py), and SBSMBatch end to end -- the reference's chunks, the path it reports, its result and its memory.

Tolerances:
  compose     bit equality with masks.float()[:, None] * x[None]: one IEEE product per value.
  gain        rtol = atol = 2e-13 against the restatement on unit-norm rows: reordering a D-term fp64 sum costs at most
              D * 2^-53 = 1.1e-13 at D = 1024, and distances of unit rows are at most 2.
  accumulate  at most 1 float32 ulp from the restatement rounded to float32 (both are one rounding of fp64 sums of non-negative
              terms that differ in order only), NaN positions identical.
  end to end  1 ulp against the restatement fed the recorded embeddings (plumbing); atol 3e-5 against the CPU oracle on
              DenseNet121 (tests/test_xai_gpu.py's derivation: fp32 embeddings of two implementations, 1e-5 each).
"""
import numpy as np
import pytest
import torch

import _sbsm_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _intervals(h, w, window, stride):
    from mirx.sbsm import window_intervals
    row_iv, col_iv = window_intervals((h, w), window, stride)
    return torch.from_numpy(row_iv).to(DEV), torch.from_numpy(col_iv).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- compose ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_sbsm_compose_is_torchs_product_bit_for_bit(geom, c):
    from mirx.sbsm import sbsm_compose
    h, w, window, stride = geom
    b = 2
    g = torch.Generator().manual_seed(h * 100 + c)
    x = torch.randn(b, c, h, w, generator=g)
    # negative values, zeros of both signs, inf and NaN at the first pixels (inside the clipped first windows), at the centre
    # and at the last pixels: every window set here has masks that cover and masks that miss each of them
    for (yy, xx) in ((0, 0), (h // 2, w // 2), (h - 1, w - 1)):
        x[0, 0, yy, xx] = float("inf")
        x[1, 0, yy, xx] = float("nan")
        x[0, c - 1, yy, (xx + 1) % w] = -float("inf")
        x[1, c - 1, yy, (xx + 1) % w] = -0.0
        x[0, 0, (yy + 1) % h, xx] = 0.0
    masks = torch.from_numpy(R.sliding_window_masks((h, w), window, stride)).to(DEV)
    n_masks = masks.shape[0]
    x = x.to(DEV)
    want = (masks.float()[:, None] * x[None]).reshape(n_masks * b, c, h, w)                  # n-major: row n * B + b
    assert bool(torch.isnan(want).sum() > torch.isnan(x).sum() * n_masks)                    # inf * 0 made new NaNs
    row_iv, col_iv = _intervals(*geom)
    for g0, n in ((0, n_masks * b), (5, 7), (n_masks * b - 1, 1), (3, 0), (n_masks * b, 0)):
        got = sbsm_compose(x, row_iv, col_iv, g0, n)
        assert got.shape == (n, c, h, w) and got.dtype == torch.float32
        assert torch.equal(_bits(got), _bits(want[g0:g0 + n])), (geom, c, g0, n)
    buf = torch.full((9, c, h, w), 7.0, device=DEV)                                           # into a caller's buffer, a view of it
    out = sbsm_compose(x, row_iv, col_iv, 5, 7, out=buf[1:8])
    assert out.data_ptr() == buf[1:8].data_ptr() and torch.equal(_bits(buf[1:8]), _bits(want[5:12]))
    assert bool((buf[0] == 7.0).all()) and bool((buf[8] == 7.0).all())                       # nothing written around it
    with pytest.raises(ValueError):
        sbsm_compose(x, row_iv, col_iv, n_masks * b - 1, 2)
    with pytest.raises(ValueError):
        sbsm_compose(x.cpu(), row_iv, col_iv, 0, 1)


# ---- gain -------------------------------------------------------------------------------------------------------------------
def _unit_rows(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen, dtype=torch.float64), dim=1).float()


@pytest.mark.parametrize("d", [1, 10, 64, 257, 1024])
@pytest.mark.parametrize("b,q", [(1, 1), (3, 1), (3, 2), (1, 2)])
def test_sbsm_gain_matches_the_restatement(d, b, q):
    from mirx.sbsm import sbsm_gain
    n_masks = 13
    gen = torch.Generator().manual_seed(1000 * d + 10 * b + q)
    # masked embeddings close to the unmasked ones, as occlusion leaves them: gains are small differences of distances
    e_r = _unit_rows(b, d, gen)
    e_m = torch.nn.functional.normalize(e_r.double().repeat(n_masks, 1) + 0.05 * torch.randn(n_masks * b, d, generator=gen,
                                                                                               dtype=torch.float64), dim=1).float()
    e_q = _unit_rows(q, d, gen)
    want = R.gain(e_q.numpy(), e_m.numpy(), e_r.numpy())
    got = sbsm_gain(e_q.to(DEV), e_m.to(DEV), e_r.to(DEV))
    assert got.shape == (q * b, n_masks) and got.dtype == torch.float64
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"SBSM_GAIN pair d={d} b={b} q={q} max|err|={err:.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-13, atol=2e-13)
    again = sbsm_gain(e_q.to(DEV), e_m.to(DEV), e_r.to(DEV))
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                        # repeated calls are bit-identical
    if q == 1:                                                                                # self-similarity needs Q == B
        e_s = _unit_rows(b, d, gen)
        want = R.gain(e_s.numpy(), e_m.numpy())
        got = sbsm_gain(e_s.to(DEV), e_m.to(DEV))
        assert got.shape == (b, n_masks)
        err = float(np.abs(got.cpu().numpy() - want).max())
        print(f"SBSM_GAIN self d={d} b={b} max|err|={err:.3e}")
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-13, atol=2e-13)


def test_sbsm_gain_exact_zeros_and_nan():
    from mirx.sbsm import sbsm_gain
    gen = torch.Generator().manual_seed(5)
    d, b, n_masks = 70, 2, 4
    e_q, e_r = _unit_rows(2, d, gen), _unit_rows(b, d, gen)
    e_m = _unit_rows(n_masks * b, d, gen)
    e_m[1 * b + 0] = e_q[0]                      # mask 1 on image 0 equals query 0: self gain exactly 0
    e_m[2 * b + 1] = e_r[1]                      # mask 2 on image 1 equals the unmasked image: pair gain exactly 0
    e_m[3 * b + 1] = 0.5 * (e_q[1] + e_r[1])     # strictly closer to query 1 than the unmasked image: m_dist < o_dist
    e_m[0 * b + 0, 3] = float("nan")
    self_gain = sbsm_gain(e_q.to(DEV), e_m.to(DEV)).cpu().numpy()
    assert self_gain[0, 1] == 0.0 and np.isnan(self_gain[0, 0]) and np.isfinite(self_gain[1]).all()
    pair = sbsm_gain(e_q.to(DEV), e_m.to(DEV), e_r.to(DEV)).cpu().numpy()                     # rows q * B + b
    want = R.gain(e_q.numpy(), e_m.numpy(), e_r.numpy())
    assert pair[0 * b + 1, 2] == 0.0 and pair[1 * b + 1, 2] == 0.0
    assert want[1 * b + 1, 3] == 0.0 and pair[1 * b + 1, 3] == 0.0
    assert np.isnan(pair[0 * b + 0, 0]) and np.isnan(pair[1 * b + 0, 0])
    assert np.array_equal(np.isnan(pair), np.isnan(want))
    np.testing.assert_allclose(pair, want, rtol=2e-13, atol=2e-13, equal_nan=True)
    e_r[0, 0] = float("nan")                                                                  # a NaN unmasked row: its gains are NaN
    pair = sbsm_gain(e_q.to(DEV), e_m.to(DEV), e_r.to(DEV)).cpu().numpy()
    assert np.isnan(pair[[0, 2]]).all() and np.isfinite(pair[[1, 3]]).all()


# ---- accumulate -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_sbsm_accumulate_matches_the_restatement(geom, rows):
    _accumulate_case(geom, rows)


def test_sbsm_accumulate_at_the_drivers_geometry():
    _accumulate_case((224, 224, 24, 5), 2)                                                    # nr = nc = 49


def _accumulate_case(geom, rows):
    from mirx.sbsm import sbsm_accumulate
    h, w, window, stride = geom
    masks = R.sliding_window_masks((h, w), window, stride)
    n_masks = masks.shape[0]
    gen = torch.Generator().manual_seed(h + rows)
    gain = torch.rand(rows, n_masks, generator=gen, dtype=torch.float64) * 0.3                # non-negative, like clamped gains
    gain[:, ::5] = 0.0
    want = R.weighted_avg(masks, gain.numpy()).astype(np.float32)
    row_iv, col_iv = _intervals(*geom)
    got = sbsm_accumulate(gain.to(DEV), row_iv, col_iv, (h, w))
    assert got.shape == (rows, h, w) and got.dtype == torch.float32
    got_np = got.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got_np), nan)
    uncovered = (masks[:, 0] == 1).all(axis=0)
    assert np.array_equal(nan, np.broadcast_to(uncovered, nan.shape))
    if geom == (22, 30, 5, 7):
        assert int(uncovered.sum()) == 360                                                    # per map
    ulp = R.ulp_diff32(got_np[~nan], want[~nan])
    print(f"SBSM_ACC geom={geom} rows={rows} ulp={ulp}")
    assert ulp <= 1
    again = sbsm_accumulate(gain.to(DEV), row_iv, col_iv, (h, w))
    assert torch.equal(_bits(got), _bits(again))


# ---- end to end -------------------------------------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """Records each call's batch size and output around a model."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.sizes, self.outputs = [], []

    def forward(self, x):
        y = self.inner(x)
        self.sizes.append(x.shape[0])
        self.outputs.append(y.detach().clone())
        return y


class _Normalize(torch.nn.Module):
    def forward(self, x):
        return torch.nn.functional.normalize(x, dim=1)


def _tiny_cuda_model(h, w, d=10):
    torch.manual_seed(2)
    return torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * h * w, d), _Normalize()).eval().to(DEV)


@pytest.mark.parametrize("pair", [False, True])
def test_sbsm_batch_native_plumbing(pair, tmp_path):
    from mirx.xai import SBSMBatch
    from oracle import xai as ox
    h, w, window, stride = 32, 40, 24, 5
    b = q = 2
    gpu_batch = 7
    model = _Recorder(_tiny_cuda_model(h, w))
    gen = torch.Generator().manual_seed(8)
    xq = torch.randn(q, 3, h, w, generator=gen).to(DEV)
    xr = torch.randn(b, 3, h, w, generator=gen).to(DEV) if pair else None
    masks = R.sliding_window_masks((h, w), window, stride)
    n_masks = masks.shape[0]
    ex = SBSMBatch(model, (h, w), gpu_batch=gpu_batch)
    ex.generate_masks(window, stride, savepath=None)
    got = ex(xq, xr)
    assert ex.last_native is True
    assert got.shape == ((q * b if pair else b), h, w) and got.dtype == torch.float32 and got.is_cuda
    head = 2 if pair else 1                                                # the query's call, and the unmasked images' for pairs
    sizes = model.sizes[head:]
    total = n_masks * b
    assert model.sizes[:head] == [q, b][:head]
    assert sum(sizes) == total and sizes[:-1] == [gpu_batch] * (len(sizes) - 1) and sizes[-1] == total - gpu_batch * (len(sizes) - 1)
    assert 0 < sizes[-1] <= gpu_batch and max(sizes) <= gpu_batch          # the reference's chunks [i, i + gpu_batch)
    e_q = model.outputs[0].cpu().numpy()
    e_r = model.outputs[1].cpu().numpy() if pair else None
    e_m = torch.cat(model.outputs[head:]).cpu().numpy()
    want = R.saliency(masks, e_q, e_m, e_r).astype(np.float32)
    got_np = got.cpu().numpy()
    assert not np.isnan(want).any() and not np.isnan(got_np).any()
    ulp = R.ulp_diff32(got_np, want)
    print(f"SBSM_E2E pair={pair} ulp={ulp}")
    assert ulp <= 1
    # the masks stay readable, and reading them does not change the path
    assert ex.masks.shape == (n_masks, 1, h, w) and np.array_equal(ex.masks.cpu().numpy(), masks)
    assert torch.equal(_bits(ex(xq, xr)), _bits(got)) and ex.last_native is True
    # a grid file is recognised ...
    np.save(tmp_path / "m.npy", masks)
    ex2 = SBSMBatch(model, (h, w), gpu_batch=gpu_batch)
    ex2.load_masks(str(tmp_path / "m.npy"))
    assert torch.equal(_bits(ex2(xq, xr)), _bits(got)) and ex2.last_native is True
    # ... a file with one pixel flipped is not: the torch path serves it
    flipped = masks.copy()
    flipped[17, 0, 2, 3] ^= 1
    np.save(tmp_path / "f.npy", flipped)
    ex3 = SBSMBatch(model, (h, w), gpu_batch=gpu_batch)
    ex3.load_masks(str(tmp_path / "f.npy"))
    got3 = ex3(xq, xr)
    assert ex3.last_native is False
    cpu_model = lambda t: model.inner.cpu()(t)                              # noqa: E731
    try:
        with torch.no_grad():
            want3 = ox.sbsm_batch(cpu_model, flipped, xq.cpu(), None if xr is None else xr.cpu(), gpu_batch=gpu_batch)
    finally:
        model.inner.to(DEV)
    np.testing.assert_allclose(got3.cpu().numpy(), want3.numpy(), rtol=0, atol=3e-5)


def test_sbsm_batch_native_on_the_mirx_embedder():
    """The existing DenseNet121 64 x 64 case (tests/test_xai_gpu.py) with Q = B = 2 pairs and gpu_batch = 7."""
    from mirx.model import DenseNet121
    from mirx.xai import SBSMBatch, sliding_window_masks
    from oracle import xai as ox
    from oracle import densenet as OD
    torch.manual_seed(3)
    size = 64
    m = DenseNet121().eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    xq = torch.randn(2, 3, size, size, generator=g)
    xr = torch.randn(2, 3, size, size, generator=g)
    masks = sliding_window_masks((size, size), 24, 16)
    want = ox.sbsm_batch(lambda t: OD.embed(t, sd), masks, xq, xr, gpu_batch=7)
    ex = SBSMBatch(m.to(DEV), (size, size), gpu_batch=7)
    ex.generate_masks(24, 16, savepath=None)
    got = ex(xq.to(DEV), xr.to(DEV))
    assert ex.last_native is True and got.shape == want.shape == (4, size, size)
    print(f"SBSM_DENSENET max|err|={float((got.cpu() - want).abs().max()):.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=0, atol=3e-5)


class _Pool(torch.nn.Module):
    def forward(self, x):
        return x.mean(dim=(2, 3))


def test_sbsm_batch_native_memory_at_224():
    """224 x 224, window 24, stride 5 (N = 2401), gpu_batch = 250: one chunk of masked images is 150.5 MB; the masks and their
    dense [HW, N] image, which the call once needed on the device, are 602 MB.  A condition, not a measurement: the rise of the
    peak over the call stays under 256 MB."""
    from mirx.xai import SBSMBatch
    ex = SBSMBatch(_Pool(), (224, 224), gpu_batch=250)
    ex.generate_masks(24, 5, savepath=None)
    assert ex.N == 2401
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    sal = ex(x)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    print(f"SBSM_MEM rise={rise / 1e6:.1f} MB")
    assert ex.last_native is True and sal.shape == (1, 224, 224)
    assert bool(torch.isfinite(sal).all())                                 # every pixel is covered at stride < window
    assert rise < 256e6
