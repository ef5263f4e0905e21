"""mirx.sbsm on the GPU on the branches and loop trips tests/test_sbsm_gpu.py never reaches: 16-byte groups that run on into
the next channel, the image loop past grid.y = 65535, the group loop past grid.x = 1024, the misaligned-pointer fallback, the
gain kernel at the widest embeddings and the accumulate kernels' row loop.  Every case asserts the precondition that puts it
on the path it is named for.

Tolerances (the suite's):
  compose     bit equality with torch's own product masks.float()[:, None] * x[None]; guard bytes around `out` unchanged.
  gain        rtol = atol = 2e-13 against the float64 restatement on unit-norm rows.
  accumulate  at most 1 float32 ulp from the restatement rounded to float32, NaN positions identical."""
import numpy as np
import pytest
import torch

import _sbsm_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MAX_GRID_Y = 65535               # k_sb_compose / k_sb_cols / k_sb_rows: grid.y = min(n or rows, 65535), then a loop
MAX_GRID_X = 1024                # k_sb_compose: grid.x = min(ceil(groups / 256), 1024), then a group loop
THREADS = 256
GUARD = 0xA5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev_iv(row_iv, col_iv):
    return torch.from_numpy(np.ascontiguousarray(row_iv)).to(DEV), torch.from_numpy(np.ascontiguousarray(col_iv)).to(DEV)


def _window_iv(h, w, window, stride):
    """The geometry's intervals (mirx.sbsm.window_intervals), checked against the reference's masks before they are used."""
    from mirx.sbsm import window_intervals
    row_iv, col_iv = window_intervals((h, w), window, stride)
    masks = R.sliding_window_masks((h, w), window, stride)
    assert np.array_equal(R.masks_of_intervals(row_iv, col_iv, (h, w)), masks)
    return row_iv, col_iv, masks


def _guarded(n_elems, lead_bytes):
    """-> (a contiguous float32 view of n_elems elements that starts lead_bytes into a 0xA5-filled byte buffer, the buffer)."""
    raw = torch.full((n_elems * 4 + 64,), GUARD, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0 and lead_bytes % 4 == 0 and 0 < lead_bytes <= 32
    return raw[lead_bytes:lead_bytes + n_elems * 4].view(torch.float32), raw


def _guards_intact(raw, n_elems, lead_bytes):
    return bool((raw[:lead_bytes] == GUARD).all()) and bool((raw[lead_bytes + n_elems * 4:] == GUARD).all())


def _product(masks, x, g0, n):
    """Images [g0, g0 + n) of torch's product, n-major (row m * B + b), computed for the masks the chunk touches only."""
    b = x.shape[0]
    m0, m1 = g0 // b, (g0 + n + b - 1) // b
    m = torch.from_numpy(masks[m0:m1]).to(x.device)
    full = (m.float()[:, None] * x[None]).reshape((m1 - m0) * b, *x.shape[1:])
    return full[g0 - m0 * b:g0 - m0 * b + n]


# ---- 5. compose: groups that cross a channel end ----------------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w,window,stride", [(2, 9, 50, 24, 16), (4, 21, 27, 8, 3), (4, 5, 5, 3, 2)])
def test_sbsm_compose_groups_cross_channel_ends(c, h, w, window, stride):
    """H * W % 4 != 0 with C * H * W % 4 == 0: the 16-byte instantiation runs, and the group that holds a channel's last pixels
    goes on with row 0 of the next channel (the `++yy == h` reset)."""
    from mirx.sbsm import sbsm_compose
    hw, chw, b = h * w, c * h * w, 2
    assert hw % 4 != 0 and chw % 4 == 0
    assert (h, w, window, stride) in R.GEOMETRIES or (h, w, window, stride) == (5, 5, 3, 2)
    row_iv, col_iv, masks = _window_iv(h, w, window, stride)
    assert row_iv[0, 0] == 0 and col_iv[0, 0] == 0 and row_iv[-1, 1] == h and col_iv[-1, 1] == w   # windows on both sides of a channel end
    g = torch.Generator().manual_seed(chw)
    x = torch.randn(b, c, h, w, generator=g)
    flat = x.view(b, chw)
    for ch in range(c - 1):                                 # the last two pixels of a channel and the first two of the next
        e = (ch + 1) * hw
        flat[0, e - 2], flat[0, e - 1], flat[0, e], flat[0, e + 1] = float("inf"), float("nan"), -float("inf"), -0.0
        flat[1, e - 2], flat[1, e - 1], flat[1, e], flat[1, e + 1] = -0.0, -float("inf"), float("nan"), float("inf")
    assert all(((ch + 1) * hw) % 4 for ch in range(c - 1))                                           # every channel end is inside a group
    x = x.to(DEV)
    n_masks = masks.shape[0]
    total = n_masks * b
    drow, dcol = _dev_iv(row_iv, col_iv)
    assert x.data_ptr() % 16 == 0
    want_all = _product(masks, x, 0, total)
    assert bool(torch.isnan(want_all).sum() > torch.isnan(x).sum() * n_masks)                        # inf * 0 made new NaNs
    for g0, n in ((0, total), (total // 2 - 1, 5)):
        got = sbsm_compose(x, drow, dcol, g0, n)
        assert got.data_ptr() % 16 == 0 and got.shape == (n, c, h, w)
        assert torch.equal(_bits(got), _bits(want_all[g0:g0 + n])), (g0, n)


# ---- 6. compose: wraps and the fallback --------------------------------------------------------------------------------------
def test_sbsm_compose_past_65535_images():
    """grid.y = min(n, 65535): 260 x 260 intervals are 67 600 masks of a 4 x 4 image, one job in one call."""
    from mirx.sbsm import check_intervals, masks_from_intervals, sbsm_compose
    h = w = 4
    sub = np.array([(lo, hi) for lo in range(4) for hi in range(lo + 1, 5)], dtype=np.int32)
    assert sub.shape == (10, 2)                             # the non-empty sub-intervals of [0, 4)
    row_iv = np.tile(sub, (26, 1))
    col_iv = np.roll(np.tile(sub, (26, 1)), 3, axis=0)      # another phase than the rows
    check_intervals(row_iv, col_iv, (h, w))                 # duplicates are legal
    masks = masks_from_intervals(row_iv, col_iv, (h, w))
    assert np.array_equal(masks, R.masks_of_intervals(row_iv, col_iv, (h, w)))
    total = masks.shape[0]
    assert total == 67600 and total > MAX_GRID_Y
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 1, h, w, generator=g)
    x[0, 0, 0, 0], x[0, 0, 1, 2], x[0, 0, 3, 3], x[0, 0, 2, 1] = float("inf"), float("nan"), -float("inf"), -0.0
    x = x.to(DEV)
    drow, dcol = _dev_iv(row_iv, col_iv)
    for g0, n in ((0, total), (65530, 20)):
        out, raw = _guarded(n * h * w, 16)                  # 0xA5 everywhere: an image the kernel skips does not pass by luck
        got = sbsm_compose(x, drow, dcol, g0, n, out=out)
        assert torch.equal(_bits(got.view(n, 1, h, w)), _bits(_product(masks, x, g0, n))), (g0, n)
        assert _guards_intact(raw, n * h * w, 16)


@pytest.mark.parametrize("c,h,w", [(3, 600, 600), (3, 301, 301)])
def test_sbsm_compose_past_the_group_grid(c, h, w):
    """grid.x = min(ceil(groups / 256), 1024): 270 000 16-byte groups at 600 x 600, 271 803 scalar ones at 301 x 301; the
    threads of the first blocks take a second group."""
    from mirx.sbsm import sbsm_compose
    chw = c * h * w
    groups = chw // 4 if chw % 4 == 0 else chw
    assert groups > MAX_GRID_X * THREADS and (chw % 4 == 0) == (h == 600)
    row_iv, col_iv, masks = _window_iv(h, w, h // 3, h // 4)
    g = torch.Generator().manual_seed(h)
    x = torch.randn(1, c, h, w, generator=g)
    x[0, 0, 0, 0], x[0, c - 1, h - 1, w - 1], x[0, 1, h // 2, w // 2] = float("inf"), -float("inf"), float("nan")
    x = x.to(DEV)
    drow, dcol = _dev_iv(row_iv, col_iv)
    g0, n = masks.shape[0] - 3, 3                           # the last row of windows: it covers the bottom of every channel
    assert x.data_ptr() % 16 == 0 and row_iv[-1, 1] == h and col_iv[-1, 1] == w
    got = sbsm_compose(x, drow, dcol, g0, n)
    want = _product(masks, x, g0, n)
    assert torch.equal(_bits(got), _bits(want))
    assert bool((got[:, 0, 0, 0] == float("inf")).all()) and bool(torch.isnan(got[n - 1, c - 1, h - 1, w - 1]))
    # the tail of the image is what the second trip writes: it is masked in every image here, so a plain copy of x would not pass
    tail = slice(MAX_GRID_X * THREADS * (4 if chw % 4 == 0 else 1), chw)
    for i in range(n):
        assert not torch.equal(_bits(want.reshape(n, chw)[i, tail]), _bits(x.reshape(chw)[tail]))


@pytest.mark.parametrize("which", ["x", "out"])
def test_sbsm_compose_misaligned_buffer_takes_the_scalar_path(which):
    """C * H * W % 4 == 0, but x or out starts 4 bytes off 16-byte alignment: the scalar instantiation has to give the bits of
    the aligned call and write nothing outside `out`."""
    from mirx.sbsm import sbsm_compose
    c, (h, w, window, stride) = 3, R.GEOMETRIES[1]
    assert (h, w) == (32, 40) and c * h * w % 4 == 0
    b = 2
    row_iv, col_iv, masks = _window_iv(h, w, window, stride)
    g = torch.Generator().manual_seed(32)
    x_h = torch.randn(b, c, h, w, generator=g)
    x_h[0, 0, 0, 0], x_h[1, 2, h - 1, w - 1], x_h[0, 1, h // 2, w // 2], x_h[1, 0, 3, 3] = float("inf"), float("nan"), -0.0, -float("inf")
    x = x_h.to(DEV)
    drow, dcol = _dev_iv(row_iv, col_iv)
    g0, n = 5, 2 * masks.shape[0] - 9
    aligned = sbsm_compose(x, drow, dcol, g0, n)
    assert torch.equal(_bits(aligned), _bits(_product(masks, x, g0, n)))
    lead = 4 if which == "out" else 16
    out, raw = _guarded(n * c * h * w, lead)
    if which == "x":
        x, _ = _guarded(b * c * h * w, 4)
        x = x.view(b, c, h, w).copy_(x_h)
    assert (x if which == "x" else out).data_ptr() % 16 == 4 and (out if which == "x" else x).data_ptr() % 16 == 0
    got = sbsm_compose(x, drow, dcol, g0, n, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(got.view(n, c, h, w)), _bits(aligned))
    assert _guards_intact(raw, n * c * h * w, lead)


# ---- 7. gain ----------------------------------------------------------------------------------------------------------------
def _unit_rows(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen, dtype=torch.float64), dim=1).float()


@pytest.mark.parametrize("d", [4097, 16383, 16384])
@pytest.mark.parametrize("b,q", [(1, 1), (3, 2)])
def test_sbsm_gain_at_the_widest_embeddings(d, b, q):
    """65, 256 and 256 lane-strided trips per wave with a ragged and a full last trip; 16 384 is the limit."""
    from mirx.sbsm import SBSM_MAX_D, sbsm_gain
    assert d <= SBSM_MAX_D and (d == SBSM_MAX_D or d % 64)
    n_masks = 13
    gen = torch.Generator().manual_seed(d + 10 * b + q)
    e_r = _unit_rows(b, d, gen)
    e_m = torch.nn.functional.normalize(e_r.double().repeat(n_masks, 1) + 0.05 * torch.randn(n_masks * b, d, generator=gen,
                                                                                               dtype=torch.float64), dim=1).float()
    e_q = _unit_rows(q, d, gen)
    e_s = _unit_rows(b, d, gen)                             # self-similarity needs Q == B
    for name, eq, er, rows in (("pair", e_q, e_r, q * b), ("self", e_s, None, b)):
        want = R.gain(eq.numpy(), e_m.numpy(), None if er is None else er.numpy())
        got = sbsm_gain(eq.to(DEV), e_m.to(DEV), None if er is None else er.to(DEV))
        assert got.shape == (rows, n_masks) and got.dtype == torch.float64
        print(f"SBSM_GAIN {name} d={d} b={b} q={q} max|err|={float(np.abs(got.cpu().numpy() - want).max()):.3e}")
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-13, atol=2e-13)
        assert float(want.max()) > 0.0


# ---- 8. accumulate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [65535, 65537])
def test_sbsm_accumulate_past_65535_rows(rows):
    """gy = min(rows, 65535) in k_sb_cols and k_sb_rows: rows 65535 and 65536 are served by the second trip of blocks 0 and 1."""
    from mirx.sbsm import sbsm_accumulate
    assert (rows > MAX_GRID_Y) == (rows == 65537)
    h, w = 3, 2
    row_iv = np.array([[0, 2], [1, 3]], dtype=np.int32)     # nr = 2: row 1 is covered twice
    col_iv = np.array([[0, 1]], dtype=np.int32)             # nc = 1: column 1 is uncovered, NaN
    masks = R.masks_of_intervals(row_iv, col_iv, (h, w))
    gen = torch.Generator().manual_seed(rows)
    gain = torch.rand(rows, 2, generator=gen, dtype=torch.float64) * 0.3
    for i, r in enumerate(r for r in (0, 65534, 65535, 65536) if r < rows):                     # a distinct value per planted row
        gain[r, 0], gain[r, 1] = 10.0 + i, 20.0 + i
    want = R.weighted_avg(masks, gain.numpy()).astype(np.float32)
    drow, dcol = _dev_iv(row_iv, col_iv)
    got = sbsm_accumulate(gain.to(DEV), drow, dcol, (h, w)).cpu().numpy()
    assert got.shape == (rows, h, w)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.broadcast_to(np.array([False, True]), nan.shape)) and np.array_equal(np.isnan(got), nan)
    ulp = R.ulp_diff32(got[~nan], want[~nan])
    print(f"SBSM_ACC rows={rows} ulp={ulp}")
    assert ulp <= 1
    for i, r in enumerate(r for r in (0, 65534, 65535, 65536) if r < rows):
        assert got[r, 0, 0] == 10.0 + i and got[r, 2, 0] == 20.0 + i and got[r, 1, 0] == 15.0 + i
