"""mirx.insdel on the GPU: the four kernels against the float64 / numpy restatement (tests/_insdel_ref.py) and the whole job
against the per-(pair, mode) CausalMetric.evaluate it batches.

Tolerances.
  steps     exact int32 equality with np.flip(np.argsort(kind="stable")).
  compose   bit equality with torch.where (int32 views, so a NaN payload counts).
  blur      every error is max|got - f64| / max|f64| per image against a float64 correlation; e_ref is that error of float32
            F.conv2d with the gkern weights on the same input and device; the kernel is allowed 4 * e_ref plus one float32 ulp
            (DESIGN 23's rule).  Each case prints `INSDEL_BLUR <case> e_ref=.. native=.. bound=..` before it asserts
            (profiles/r16_insdel_accuracy.txt is that output).  Per pixel as well: |got - f64| <= 0.5 ulp32(f64) + 2 klen^2
            2^-53 (|k| * |x|), R.blur_pixel_bound -- the design's "correctly rounded up to klen^2 2^-53", no measured number.
  curves    1e-12 against numpy float64: both take the cosine of the same float32 rows in float64; only the summation order of
            at most 1024 terms differs.
  job       2e-6 on scores and AUC against CausalMetric.evaluate with conv2d substrates: the bound tests/test_xai_gpu.py sets
            between two chunkings of that path (float32 embeddings at other batch sizes, its float32 cosine)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _insdel_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tile():
    from mirx import _lib
    return _lib.load().mirx_rank_sort_tile()


# ---- steps ------------------------------------------------------------------------------------------------------------------
_maps = R.saliency_maps                                   # name -> [k, hw] float32: the four map kinds


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("hw", [1, 2, 63, 64, 65, 4095, 4096, 4097, 224 * 224])
def test_steps_equal_the_stable_argsort(hw, k):
    from mirx.insdel import insdel_steps
    assert _tile() == 4096                                  # 4095 / 4096 / 4097 are the sort's tile edges
    for name, sal in _maps(k, hw, 100 + hw % 97 + k).items():
        dsal = sal.to(DEV)
        for step in (1, 7, hw, hw + 5):
            got = insdel_steps(dsal, step)
            assert got.dtype == torch.int32 and got.shape == (k, hw)
            assert np.array_equal(got.cpu().numpy(), R.steps_ref(sal.numpy(), step)), (name, step)


def test_steps_limits():
    from mirx.insdel import insdel_steps
    with pytest.raises(ValueError):
        insdel_steps(torch.zeros(1, 4, device=DEV), 0)
    with pytest.raises(ValueError):
        insdel_steps(torch.zeros(1, (1 << 20) + 1, device=DEV), 1)
    with pytest.raises(ValueError):
        insdel_steps(torch.zeros(4, dtype=torch.float32, device=DEV), 1)


# ---- compose ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [7, 32])
def test_compose_is_bit_equal_to_where(s):
    from mirx.insdel import insdel_compose
    hw, k, step = s * s, 3, (10 if s == 7 else 100)
    n_steps = math.ceil(hw / step)
    per = n_steps + 1
    g = torch.Generator().manual_seed(s)
    sal = torch.rand(k, hw, generator=g)
    t = torch.from_numpy(R.steps_ref(sal.numpy(), step)).to(DEV)
    bank = torch.randn(2 * k, 3, hw, generator=g)
    bank[0, 1, 5] = float("nan")
    bank[4, 2, hw - 1] = -float("nan")
    bank = bank.to(DEV)
    # curve j: start, finish, row -- -1 (the zero image) as finish (0, 4) and as start (1), rows in another order than curves
    start = torch.tensor([0, -1, 2, 3, 4, 5], dtype=torch.int32, device=DEV)
    finish = torch.tensor([-1, 1, 5, 0, -1, 2], dtype=torch.int32, device=DEV)
    row = torch.tensor([0, 0, 2, 1, 1, 2], dtype=torch.int32, device=DEV)
    total = 6 * per
    chunks = [(0, total), (per // 2, 2 * per), (per - 1, per + 2), (3, 1), (total - 2, 2), (per + 1, 0)]
    assert per // 2 > 0 and (per // 2 + 2 * per - 1) // per == 2          # the second chunk starts and ends mid-curve, spans three
    for g0, n in chunks:
        got = insdel_compose(t, bank, start, finish, row, n_steps, g0, n)
        want = R.compose_ref(t, bank, start, finish, row, n_steps, g0, n)
        assert got.shape == (n, 3, hw)
        assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), (g0, n)
    full = insdel_compose(t, bank, start, finish, row, n_steps, 0, total).view(6, per, 3, hw)
    assert torch.isnan(full[0, 0, 1, 5]) and torch.equal(full[0, -1], torch.zeros_like(full[0, -1]))
    assert torch.equal(full[1, 0], torch.zeros_like(full[1, 0])) and torch.equal(full[1, -1].view(torch.int32), bank[1].view(torch.int32))
    with pytest.raises(ValueError):
        insdel_compose(t, bank, start, finish, row, n_steps, total - 1, 2)


# ---- blur -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,klen", [(7, 7, 51), (32, 32, 11), (50, 70, 51), (224, 224, 51)])
def test_blur_accuracy_and_batch_invariance(h, w, klen):
    from mirx.insdel import blur2d_same
    from mirx.xai import GaussianBlur, gkern
    nsig = math.sqrt(50) if klen == 51 else math.sqrt(5)
    g = torch.Generator().manual_seed(h * 1000 + w + klen)
    x = torch.randn(3, 3, h, w, generator=g)
    x[1] = x[1].abs() * 3.0 + 1.0                           # an all-positive image: no cancellation hides an error
    blur = GaussianBlur(klen, nsig)
    exp = R.blur_f64(x, blur.kernel2d)
    dx = x.to(DEV)
    ref32 = F.conv2d(dx, gkern(klen, nsig).to(DEV), padding=klen // 2)
    e_ref = max(R.image_errors(ref32, exp))
    bound = 4 * e_ref + R.ULP32
    got3 = blur(dx)
    assert blur.last_native and got3.shape == x.shape
    ones = [blur2d_same(dx[i:i + 1], blur.kernel2d) for i in range(3)]
    for n, got in ((3, got3), (1, torch.cat(ones))):
        errs = R.image_errors(got, exp)
        print(f"INSDEL_BLUR h={h} w={w} klen={klen} n={n} e_ref={e_ref:.3e} native={max(errs):.3e} bound={bound:.3e}")
        assert max(errs) <= bound, (errs, e_ref)
    assert torch.equal(got3.view(torch.int32), torch.cat(ones).view(torch.int32))        # n = 3 is three n = 1 calls, bit for bit
    # per pixel: half a float32 ulp of the float64 value plus the two float64 sums' own error (R.blur_pixel_bound)
    exc, at = R.blur_pixel_excess(got3, x, blur.kernel2d, exp)
    print(f"INSDEL_BLUR h={h} w={w} klen={klen} gkern per-pixel max|err|/bound={exc:.6f} at {at}")
    assert exc <= 1.0, (exc, at)
    # a kernel that is neither symmetric nor separable: the correlation, not the convolution, and no rank-1 shortcut
    k2 = torch.randn(klen, klen, generator=g)
    got = blur2d_same(dx[:1], k2)
    exp2 = R.blur_f64(x[:1], k2)
    assert max(R.image_errors(got, exp2)) <= R.ULP32
    exc, at = R.blur_pixel_excess(got, x[:1], k2, exp2)
    print(f"INSDEL_BLUR h={h} w={w} klen={klen} random per-pixel max|err|/bound={exc:.6f} at {at}")
    assert exc <= 1.0, (exc, at)


def test_blur_limits():
    from mirx.insdel import blur2d_same
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    for shape in ((4, 4), (65, 65), (5, 3)):
        with pytest.raises(ValueError):
            blur2d_same(x, torch.zeros(shape))
    assert torch.equal(blur2d_same(x[:0], torch.ones(3, 3)), x[:0])
    one = torch.zeros(1, 1, 5, 6, device=DEV)
    one[0, 0, 2, 3] = 1.0
    k = torch.arange(9.0).reshape(3, 3)
    assert torch.equal(blur2d_same(one, k)[0, 0, 1:4, 2:5].cpu(), k.flip(0, 1))          # cross-correlation of a dirac


# ---- curves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, 14, 225])
@pytest.mark.parametrize("d,curves", [(1, 1), (7, 2), (64, 5), (1024, 3)])
def test_curves_match_numpy_float64(d, curves, n_steps):
    from mirx.insdel import insdel_scores
    g = torch.Generator().manual_seed(d * 7 + curves + n_steps)
    per = n_steps + 1
    q = torch.randn(1, d, generator=g)
    r = torch.randn(curves * per, d, generator=g)
    # planted rows: clearly negative and clearly positive cosines, a value above 1 is impossible but 1 itself is there, one zero row
    r[0] = -2.0 * q[0]
    r[per - 1] = 3.0 * q[0]
    r[(curves * per) // 2] = -0.5 * q[0] + (0.01 * torch.randn(d, generator=g) if d > 1 else 0.0)
    zero_at = curves * per - 1
    r[zero_at] = 0.0
    cos = F.cosine_similarity(q.double(), r.double())
    keep = (cos.abs() >= 1e-3) | (torch.arange(curves * per) == zero_at)                 # float32 and float64 agree on every sign
    r[~keep] = q[0] * 0.25
    exp_scores, exp_auc, exp_zero = R.curves_ref(q.numpy(), r.numpy(), curves, n_steps)
    assert exp_zero.sum() >= 2 or d == 1
    scores, auc, zero = insdel_scores(q.to(DEV), r.to(DEV), curves, n_steps)
    assert scores.dtype == torch.float64 and auc.dtype == torch.float64 and zero.dtype == torch.int64
    np.testing.assert_allclose(scores.cpu().numpy(), exp_scores, rtol=0, atol=1e-12)
    np.testing.assert_allclose(auc.cpu().numpy(), exp_auc, rtol=0, atol=1e-12)
    assert np.array_equal(zero.cpu().numpy(), exp_zero)
    assert scores.cpu().numpy().reshape(-1)[zero_at] == 0.0 and scores.cpu().numpy().reshape(-1)[0] == 0.0


# ---- the job ----------------------------------------------------------------------------------------------------------------
_MODEL = {}


def _densenet():
    if "m" not in _MODEL:
        from mirx.model import DenseNet121
        torch.manual_seed(11)
        _MODEL["m"] = DenseNet121().eval().to(DEV)
    return _MODEL["m"]


def _parent_curves(model, x_q, x_r, sal, step, size):
    """CausalMetric.evaluate per (pair, mode) with conv2d substrates: the loop insdel_curves replaces."""
    from mirx.xai import CausalMetric, gkern
    kern = gkern(51, math.sqrt(50)).to(DEV)
    subs = {"del": torch.zeros_like, "ins": lambda x: F.conv2d(x, kern, padding=25)}
    out = {}
    for k in range(x_r.shape[0]):
        for mi, mode in enumerate(("del", "ins")):
            out[k, mi] = CausalMetric(model, mode, step, subs[mode], input_size=size).evaluate(x_q, x_r[k:k + 1], sal[k])
    return out


@pytest.mark.parametrize("size,step,k", [(64, 300, 3), (224, 6272, 2)])
def test_job_matches_causal_metric_per_pair(size, step, k):
    from mirx.xai import insdel_curves
    model = _densenet()
    g = torch.Generator().manual_seed(size)
    x_q = torch.randn(1, 3, size, size, generator=g).to(DEV)
    x_r = torch.randn(k, 3, size, size, generator=g).to(DEV)
    sal = R.distinct_saliency(k, size * size, size + 1).reshape(k, size, size)
    assert R.tie_free(sal)
    res = insdel_curves(model, x_q, x_r, sal, step, input_size=size)
    assert res.last_native and res.modes == ("del", "ins")
    n_steps = math.ceil(size * size / step)
    assert res.scores.shape == (k, 2, n_steps + 1)
    want = _parent_curves(model, x_q, x_r, sal, step, size)
    for (ki, mi), (auc, scores, zero) in want.items():
        err = float(np.abs(res.scores[ki, mi] - scores).max())
        print(f"INSDEL_JOB size={size} k={ki} mode={res.modes[mi]} max|d score|={err:.3e} |d auc|={abs(res.auc[ki, mi] - auc):.3e}")
        assert err <= 2e-6 and abs(res.auc[ki, mi] - auc) <= 2e-6
        assert res.zero_counter[ki, mi] == zero
    small = insdel_curves(model, x_q, x_r, torch.from_numpy(sal).to(DEV), step, max_batch=5)      # device saliency, 5-image chunks
    assert small.last_native
    np.testing.assert_allclose(small.scores, res.scores, rtol=0, atol=2e-6)
    np.testing.assert_allclose(small.auc, res.auc, rtol=0, atol=2e-6)
    assert np.array_equal(small.zero_counter, res.zero_counter)


def test_insdel_forward_equals_its_evaluate():
    from mirx.xai import InsDel
    size, k = 64, 2
    model = _densenet()
    g = torch.Generator().manual_seed(3)
    x_q = torch.randn(1, 3, size, size, generator=g)
    hits = [torch.randn(1, 3, size, size, generator=g) for _ in range(k)]
    sal = R.distinct_saliency(k, size * size, 9).reshape(k, size, size)
    metric = InsDel(model, DEV, input_size=size)
    ins_avg, del_avg, z_ins, z_del = metric.forward(x_q, hits, [sal[i] for i in range(k)])
    assert metric.last_native and len(ins_avg) == len(del_avg) == len(z_ins) == len(z_del) == k
    for i in range(k):
        s_del, s_ins, third, fourth = metric.evaluate(sal[i], hits[i])
        assert abs(s_del - del_avg[i]) <= 2e-6 and abs(s_ins - ins_avg[i]) <= 2e-6
        assert (third, fourth) == (z_ins[i], z_del[i])


def test_plain_torch_module_takes_the_native_glue():
    from mirx.xai import CausalMetric, GaussianBlur, insdel_curves

    class Plain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(3 * 8 * 8, 16)

        def forward(self, x):
            return {"embedding": self.fc(F.avg_pool2d(x, 4).flatten(1))}

    torch.manual_seed(5)
    size, k, step = 32, 2, 100
    model = Plain().eval().to(DEV)
    g = torch.Generator().manual_seed(6)
    x_q = torch.randn(1, 3, size, size, generator=g).to(DEV)
    x_r = torch.randn(k, 3, size, size, generator=g).to(DEV)
    sal = R.distinct_saliency(k, size * size, 2).reshape(k, size, size)
    blur = GaussianBlur(11, math.sqrt(5))
    res = insdel_curves(model, x_q, x_r, sal, step, substrates={"ins": blur}, max_batch=7)
    assert res.last_native and blur.last_native
    for ki in range(k):
        for mi, mode in enumerate(("del", "ins")):
            sub = torch.zeros_like if mode == "del" else blur
            auc, scores, zero = CausalMetric(model, mode, step, sub, input_size=size).evaluate(x_q, x_r[ki:ki + 1], sal[ki])
            np.testing.assert_allclose(res.scores[ki, mi], scores, rtol=0, atol=2e-6)
            assert abs(res.auc[ki, mi] - auc) <= 2e-6 and res.zero_counter[ki, mi] == zero
