"""mirx.insdel on the GPU past the first trip of every loop: the shapes at which k_id_auc's chunk loop, k_id_compose's image and
group loops, the misaligned-pointer fallback, the blur's largest and smallest kernels and the 32-bit sort's tile and segment
counts do what tests/test_insdel_gpu.py never makes them do.  Every case asserts the precondition that puts it on the path it
is named for.  References: tests/_insdel_ref.py (float64 / numpy), nothing here restates the code under test.

Tolerances.
  curves    1e-12 on scores and AUC, counters exact (the suite's rule).  The sequential float64 sum of 5001 scores in [0, 1]
            and numpy's pairwise sum differ by about 1e-16 after the division by n_steps; a cosine of D = 65 537 float32
            terms reordered moves by D * 2^-53 relative to sum|a b| / (|a| |b|) <= 1, 7e-12 at the very worst and ~1e-16 for
            random rows.
  blur      per pixel |got - f64| <= 0.5 ulp32(f64) + 2 klen^2 2^-53 (|k| * |x|) (R.blur_pixel_bound: the design's claim, no
            measured number); n = 2 bit-equal to two n = 1 calls; klen = 1 bit-equal to float32(float64(k) * float64(x)).
            Each case prints `INSDEL_BLUR ...` before it asserts (profiles/r16_insdel_accuracy.txt).
  compose   bit equality (int32 views) with torch.where; guard bytes around `out` unchanged.
  steps     exact int32 equality with np.flip(np.argsort(kind="stable")) // step."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _insdel_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

AUC_CHUNK = 2048                 # k_id_auc's LDS staging buffer, in scores
COMPOSE_MAX_GRID_Y = 65535       # k_id_compose: grid.y = min(n, 65535), then an image loop
COMPOSE_MAX_GRID_X = 1024        # grid.x = min(ceil(groups / 256), 1024), then a group loop
THREADS = 256
GUARD = 0xA5


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. curves --------------------------------------------------------------------------------------------------------------
def _curve_rows(q, r, plants, g):
    """Plant clearly negative cosines at the flat rows `plants`, then apply the suite's rule |cos| >= 1e-3 to the rest so
    that float32 and float64 agree on every sign."""
    for i in plants:
        r[i] = -2.0 * q[0]
    cos = F.cosine_similarity(q.double(), r.double())
    r[cos.abs() < 1e-3] = q[0] * 0.25
    return F.cosine_similarity(q.double(), r.double())


def _check_curves(q, r, curves, n_steps):
    from mirx.insdel import insdel_scores
    exp_scores, exp_auc, exp_zero = R.curves_ref(q.numpy(), r.numpy(), curves, n_steps)
    scores, auc, zero = insdel_scores(q.to(DEV), r.to(DEV), curves, n_steps)
    scores, auc, zero = scores.cpu().numpy(), auc.cpu().numpy(), zero.cpu().numpy()
    print(f"INSDEL_CURVES d={q.shape[1]} n_steps={n_steps} max|d score|={np.abs(scores - exp_scores).max():.3e} "
          f"max|d auc|={np.abs(auc - exp_auc).max():.3e} zero={zero.tolist()}")
    np.testing.assert_allclose(scores, exp_scores, rtol=0, atol=1e-12)
    np.testing.assert_allclose(auc, exp_auc, rtol=0, atol=1e-12)
    assert np.array_equal(zero, exp_zero)
    return exp_zero


@pytest.mark.parametrize("per", [2047, 2048, 2049, 4096, 4097, 5001])
def test_curves_across_the_auc_chunk(per):
    """n_steps + 1 scores per curve around and past k_id_auc's 2048-entry chunk: the sum, the first and last score and the
    negative counter have to carry across trips."""
    d, curves, n_steps = 7, 2, per - 1
    trips = (per + AUC_CHUNK - 1) // AUC_CHUNK
    assert trips == {2047: 1, 2048: 1, 2049: 2, 4096: 2, 4097: 3, 5001: 3}[per] and (trips > 1) == (n_steps + 1 > AUC_CHUNK)
    g = torch.Generator().manual_seed(per)
    q = torch.randn(1, d, generator=g)
    r = torch.randn(curves * per, d, generator=g)
    # negatives in the first chunk, in the last chunk and on both sides of 2047 | 2048; other places per curve, so the two
    # counters differ
    in_curve = [[0, 5, AUC_CHUNK - 1, AUC_CHUNK, per - 1], [1, AUC_CHUNK - 2, AUC_CHUNK - 1, AUC_CHUNK, AUC_CHUNK + 1, per - 2, per - 1]]
    plants = [c * per + i for c in range(curves) for i in in_curve[c] if 0 <= i < per]
    cos = _curve_rows(q, r, plants, g)
    assert bool((cos.abs() >= 1e-3).all())
    neg = (cos < 0).reshape(curves, per).numpy()
    last0 = (trips - 1) * AUC_CHUNK
    assert neg[:, :AUC_CHUNK].any(axis=1).all() and neg[:, last0:].any(axis=1).all() and neg[0, 0] and neg[:, per - 1].all()
    assert all(neg[:, i].all() for i in (AUC_CHUNK - 1, AUC_CHUNK) if i < per)
    exp_zero = _check_curves(q, r, curves, n_steps)
    assert np.array_equal(exp_zero, neg.sum(axis=1))
    if trips > 1:                                                       # the counter of the first trip alone would be another number
        assert (neg[:, AUC_CHUNK:].sum(axis=1) > 0).all()


@pytest.mark.parametrize("d", [4097, 65537])
def test_curves_at_wide_embeddings(d):
    """k_id_cos: 65 and 1025 lane-strided trips per wave (the suite stops at 16)."""
    curves, n_steps = 2, 2
    g = torch.Generator().manual_seed(d)
    q = torch.randn(1, d, generator=g)
    r = torch.randn(curves * (n_steps + 1), d, generator=g)
    r[3] = -0.5 * q[0] + 0.01 * torch.randn(d, generator=g)
    cos = _curve_rows(q, r, [0], g)
    assert bool((cos.abs() >= 1e-3).all()) and int((cos < 0).sum()) >= 2
    _check_curves(q, r, curves, n_steps)


# ---- 2. blur ----------------------------------------------------------------------------------------------------------------
def _blur_lds_bytes(klen):
    """klen^2 fp64 taps and a (32 + klen - 1)-row fp32 patch whose row stride is that side made odd."""
    side = 32 + klen - 1
    return klen * klen * 8 + side * (side | 1) * 4


@pytest.mark.parametrize("h,w,klen", [(40, 45, 63), (33, 70, 63), (1, 1, 63), (3, 5, 3), (37, 3, 51), (33, 33, 1), (64, 64, 63)])
def test_blur_at_its_kernel_and_image_edges(h, w, klen):
    """klen = 63 is the one size above the 64 KiB default of dynamic LDS; klen = 1 has no neighbours; w < 4 leaves a thread's
    four-pixel group partly outside the image; (33, 70) and (40, 45) end a tile after 1, 6, 8 and 13 pixels."""
    from mirx.insdel import blur2d_same
    assert (_blur_lds_bytes(klen) > 65536) == (klen == 63) and _blur_lds_bytes(63) == 67472 and _blur_lds_bytes(51) == 48032
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + klen)
    x = torch.randn(2, 3, h, w, generator=g)
    x[1] = x[1].abs() * 3.0 + 1.0                           # an all-positive image: no cancellation hides an error
    k2 = torch.randn(klen, klen, generator=g)               # neither symmetric nor separable
    exp = R.blur_f64(x, k2)
    dx = x.to(DEV)
    got = blur2d_same(dx, k2)
    assert got.shape == x.shape and got.dtype == torch.float32
    ones = torch.cat([blur2d_same(dx[i:i + 1], k2) for i in range(2)])
    exc, at = R.blur_pixel_excess(got, x, k2, exp)
    print(f"INSDEL_BLUR h={h} w={w} klen={klen} n=2 random per-pixel max|err|/bound={exc:.6f} at {at} "
          f"image errors={max(R.image_errors(got, exp)):.3e}")
    assert torch.equal(_bits(got), _bits(ones))             # n = 2 is two n = 1 calls, bit for bit
    assert exc <= 1.0, (exc, at)
    if klen == 1:
        want = (k2.double()[0, 0] * x.double()).float()     # one exact float64 product, one rounding
        assert torch.equal(_bits(got.cpu()), _bits(want))


# ---- 3. compose -------------------------------------------------------------------------------------------------------------
def _guarded(n_elems, lead_bytes, dtype=torch.float32):
    """-> (a contiguous `dtype` view of n_elems elements that starts lead_bytes into a 0xA5-filled byte buffer, the buffer)."""
    raw = torch.full((n_elems * 4 + 64,), GUARD, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0 and lead_bytes % 4 == 0 and 0 < lead_bytes <= 32
    return raw[lead_bytes:lead_bytes + n_elems * 4].view(dtype), raw


def _guards_intact(raw, n_elems, lead_bytes):
    return bool((raw[:lead_bytes] == GUARD).all()) and bool((raw[lead_bytes + n_elems * 4:] == GUARD).all())


@pytest.mark.parametrize("hw", [4, 3])
def test_compose_past_65535_images(hw):
    """grid.y = min(n, 65535): images 65535 .. n - 1 are the second trip of the image loop.  hw = 4 takes the 16-byte
    instantiation, hw = 3 the scalar one."""
    from mirx.insdel import insdel_compose
    n_steps, curves, k, n_bank = 4, 13200, 3, 4
    per = n_steps + 1
    total = curves * per
    assert total > COMPOSE_MAX_GRID_Y and (hw % 4 == 0) == (hw == 4)
    g = torch.Generator().manual_seed(hw)
    t = torch.from_numpy(R.steps_ref(torch.rand(k, hw, generator=g).numpy(), 1)).to(DEV)       # ranks 0 .. hw - 1
    bank = torch.randn(n_bank, 3, hw, generator=g)
    bank[1, 0, 0] = float("nan")
    bank[3, 2, hw - 1] = -float("nan")
    bank = bank.to(DEV)
    start = torch.randint(-1, n_bank, (curves,), generator=g, dtype=torch.int32).to(DEV)
    finish = torch.randint(-1, n_bank, (curves,), generator=g, dtype=torch.int32).to(DEV)
    row = torch.randint(0, k, (curves,), generator=g, dtype=torch.int32).to(DEV)
    assert int((start == -1).sum()) > 0 and int((finish == -1).sum()) > 0
    assert t.data_ptr() % 16 == 0 and bank.data_ptr() % 16 == 0
    for g0, n in ((0, total), (65530, 20)):
        out, raw = _guarded(n * 3 * hw, 16)                 # 0xA5 everywhere: an image the kernel skips does not pass by luck
        got = insdel_compose(t, bank, start, finish, row, n_steps, g0, n, out=out).view(n, 3, hw)
        want = R.compose_ref(t, bank, start, finish, row, n_steps, g0, n)
        assert torch.equal(_bits(got), _bits(want)), (hw, g0, n)
        assert _guards_intact(raw, n * 3 * hw, 16)


@pytest.mark.parametrize("hw", [1 << 20, (1 << 20) - 1])
def test_compose_at_the_largest_images(hw):
    """grid.x = min(ceil(groups / 256), 1024).  Scalar path at hw = 2^20 - 1: 1 048 575 groups, every thread loops four times.
    16-byte path at hw = 2^20, the limit: 262 144 groups = 1024 * 256 exactly, the grid's exact fit -- under hw <= 2^20 the
    16-byte instantiation can never take a second trip, so this is its last group, not a wrap."""
    from mirx.insdel import INSDEL_MAX_HW, insdel_compose
    n_steps, curves, k, n_bank = 4, 2, 2, 3
    groups = hw // 4 if hw % 4 == 0 else hw
    if hw % 4:
        assert groups > COMPOSE_MAX_GRID_X * THREADS
    else:
        assert groups == COMPOSE_MAX_GRID_X * THREADS and hw == INSDEL_MAX_HW
    g = torch.Generator().manual_seed(hw % 1000)
    t = torch.randint(0, n_steps + 1, (k, hw), generator=g, dtype=torch.int32)
    t[:, 0], t[:, hw - 1] = 0, 1                            # the first and last pixel flip inside the chunk below
    t = t.to(DEV)
    bank = torch.randn(n_bank, 3, hw, generator=g)
    bank[0, 0, 0], bank[0, 2, hw - 1] = float("nan"), -float("nan")
    bank[2, 1, 0], bank[2, 1, hw - 1] = -float("nan"), float("nan")
    bank = bank.to(DEV)
    start = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    finish = torch.tensor([2, -1], dtype=torch.int32, device=DEV)
    row = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    assert t.data_ptr() % 16 == 0 and bank.data_ptr() % 16 == 0
    for g0, n in ((1, 2), (4, 2)):                          # steps 1, 2 of curve 0; the last image of curve 0 and the first of curve 1
        out, raw = _guarded(n * 3 * hw, 16)
        got = insdel_compose(t, bank, start, finish, row, n_steps, g0, n, out=out).view(n, 3, hw)
        want = R.compose_ref(t, bank, start, finish, row, n_steps, g0, n)
        assert torch.equal(_bits(got), _bits(want)), (hw, g0, n)
        assert _guards_intact(raw, n * 3 * hw, 16)
        assert bool(torch.isnan(got[:, :, 0]).any()) and bool(torch.isnan(got[:, :, hw - 1]).any())


@pytest.mark.parametrize("which", ["out", "bank", "t"])
def test_compose_misaligned_buffer_takes_the_scalar_path(which):
    """hw % 4 == 0, but one buffer starts 4 bytes off 16-byte alignment: the launcher falls back to the scalar instantiation,
    which has to give the bits of the aligned call and write nothing outside `out`."""
    from mirx.insdel import insdel_compose
    hw, n_steps, k, n_bank = 1024, 8, 2, 3
    per = n_steps + 1
    g = torch.Generator().manual_seed(17)
    t_h = torch.from_numpy(R.steps_ref(torch.rand(k, hw, generator=g).numpy(), hw // n_steps))
    bank_h = torch.randn(n_bank, 3, hw, generator=g)
    bank_h[1, 1, 0], bank_h[2, 0, hw - 1] = float("nan"), -float("nan")
    start = torch.tensor([0, -1, 2], dtype=torch.int32, device=DEV)
    finish = torch.tensor([1, 0, -1], dtype=torch.int32, device=DEV)
    row = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    g0, n = per // 2, 2 * per                               # starts and ends mid-curve, spans all three
    t, bank = t_h.to(DEV), bank_h.to(DEV)
    aligned = insdel_compose(t, bank, start, finish, row, n_steps, g0, n)
    assert torch.equal(_bits(aligned), _bits(R.compose_ref(t, bank, start, finish, row, n_steps, g0, n)))
    lead = {"out": 4, "bank": 16, "t": 16}[which]
    out, raw = _guarded(n * 3 * hw, lead)
    if which == "bank":
        bank, _ = _guarded(n_bank * 3 * hw, 4)
        bank = bank.view(n_bank, 3, hw).copy_(bank_h)
    if which == "t":
        t, _ = _guarded(k * hw, 4, torch.int32)
        t = t.view(k, hw).copy_(t_h)
    ptrs = {"out": out.data_ptr(), "bank": bank.data_ptr(), "t": t.data_ptr()}
    assert hw % 4 == 0 and ptrs[which] % 16 == 4 and all(p % 16 == 0 for name, p in ptrs.items() if name != which)
    got = insdel_compose(t, bank, start, finish, row, n_steps, g0, n, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(got.view(n, 3, hw)), _bits(aligned))
    assert _guards_intact(raw, n * 3 * hw, lead)


# ---- 4. steps ---------------------------------------------------------------------------------------------------------------
def _tile():
    from mirx import _lib
    return _lib.load().mirx_rank_sort_tile()


def _check_steps(k, hw, steps, seed):
    from mirx.insdel import insdel_steps
    for name, sal in R.saliency_maps(k, hw, seed).items():
        rank = R.steps_ref(sal.numpy(), 1)                  # the stable argsort once per map; a step only divides the rank
        dsal = sal.to(DEV)
        for step in steps:
            got = insdel_steps(dsal, step)
            assert got.dtype == torch.int32 and got.shape == (k, hw)
            assert np.array_equal(got.cpu().numpy(), rank // np.int32(step)), (name, step)


@pytest.mark.parametrize("hw", [65535, 65536, 65537, (1 << 20) - 1, 1 << 20])
def test_steps_up_to_the_largest_map(hw):
    """The 32-bit sort at 16, 17 and 256 tiles per segment (the suite stops at 13): 65 536 = 16 tiles exactly, 2^20 the limit."""
    from mirx.insdel import INSDEL_MAX_HW
    tile = _tile()
    assert tile == 4096 and (hw + tile - 1) // tile in (16, 17, 256) and hw <= INSDEL_MAX_HW == 256 * tile
    _check_steps(2, hw, (1, 1000, hw), hw % 101)


@pytest.mark.parametrize("k,hw", [(65535, 3), (300, 4097)])
def test_steps_at_many_segments(k, hw):
    """K = 65535 is the segment limit (grid.y of every sort launch); K = 300 at hw = 4097 is 600 tiles, one of them of one key."""
    from mirx.insdel import INSDEL_MAX_K
    assert k <= INSDEL_MAX_K and (k == INSDEL_MAX_K or hw == _tile() + 1)
    _check_steps(k, hw, (1, 1000, hw), k % 89)
