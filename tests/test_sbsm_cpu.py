"""mirx.sbsm without a GPU: the window geometry as intervals, the recognition of a window grid in a mask file, the wrappers'
argument rules and SBSMBatch's choice of path; and the float64 restatement (tests/_sbsm_ref.py) against the restatement that
keeps the reference's tensors (oracle/xai.py:sbsm_batch) -- that last test touches no mirx code."""
import numpy as np
import pytest
import torch

import _sbsm_ref as R


def _zero_rectangles(masks):
    """Per mask the bounding rectangle of its zero set, after checking that the zero set IS that rectangle."""
    out = []
    for m in masks[:, 0]:
        ys, xs = np.nonzero(m == 0)
        r0, r1, c0, c1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
        want = np.ones_like(m)
        want[r0:r1, c0:c1] = 0
        assert np.array_equal(m, want)
        out.append((r0, r1, c0, c1))
    return out


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_window_intervals_are_the_zero_sets(geom):
    from mirx.sbsm import masks_from_intervals, window_intervals
    from mirx.xai import sliding_window_masks
    h, w, window, stride = geom
    masks = sliding_window_masks((h, w), window, stride)
    assert np.array_equal(masks, R.sliding_window_masks((h, w), window, stride))
    row_iv, col_iv = window_intervals((h, w), window, stride)
    assert row_iv.dtype == col_iv.dtype == np.int32 and row_iv.shape[1] == col_iv.shape[1] == 2
    nr, nc = len(row_iv), len(col_iv)
    assert nr * nc == masks.shape[0]
    rects = _zero_rectangles(masks)
    for i in range(nr):
        for j in range(nc):
            assert rects[i * nc + j] == (row_iv[i, 0], row_iv[i, 1], col_iv[j, 0], col_iv[j, 1])
    assert np.array_equal(masks_from_intervals(row_iv, col_iv, (h, w)), masks)


def test_geometry_table():
    """The N column of the geometry table and the uncovered pixels of the gapped case."""
    from mirx.sbsm import window_intervals
    ns = [len(r) * len(c) for r, c in (window_intervals(g[:2], g[2], g[3]) for g in R.GEOMETRIES)]
    assert ns == [99, 132, 12, 8]
    masks = R.sliding_window_masks((22, 30), 5, 7)
    covered = (masks[:, 0] == 0).any(axis=0)
    assert int((~covered).sum()) == 22 * 30 - 12 * 25 == 360                    # per map: the 12 windows are disjoint
    assert np.isnan(R.weighted_avg(masks, np.ones((1, 12)))[0][~covered]).all()
    assert (R.weighted_avg(masks, np.ones((1, 12)))[0][covered] == 1.0).all()
    with pytest.raises(ValueError):
        window_intervals((8, 8), 0, 1)
    with pytest.raises(ValueError):
        window_intervals((8, 8), 3, 0)


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_grid_of_masks_round_trip(geom):
    from mirx.sbsm import grid_of_masks, window_intervals
    h, w, window, stride = geom
    masks = R.sliding_window_masks((h, w), window, stride)
    row_iv, col_iv = window_intervals((h, w), window, stride)
    for m in (masks, masks[:, 0]):
        got = grid_of_masks(m)
        assert got is not None
        assert got[0].dtype == got[1].dtype == np.int32
        assert np.array_equal(got[0], row_iv) and np.array_equal(got[1], col_iv)


def test_grid_of_masks_rejects_what_is_no_grid():
    from mirx.sbsm import grid_of_masks
    masks = R.sliding_window_masks((32, 40), 24, 5)
    inside = masks.copy()
    inside[7, 0, 3, 3] ^= 1                                     # a pixel of a window switched back on
    outside = masks.copy()
    ys, xs = np.nonzero(masks[7, 0])
    outside[7, 0, ys[-1], xs[-1]] = 0                           # a pixel far from the window switched off
    swapped = masks.copy()
    swapped[[3, 20]] = swapped[[20, 3]]
    assert not np.array_equal(swapped[3], masks[3])
    ell = masks.copy()
    ell[5, 0] = 1
    ell[5, 0, 2:10, 2:5] = 0
    ell[5, 0, 7:10, 2:12] = 0                                   # an L-shaped zero set
    two = masks.copy()
    two[0, 0, 0, 0] = 2
    for bad in (inside, outside, swapped, ell, two, masks.astype(np.float32), masks[:0], np.ones_like(masks)):
        assert grid_of_masks(bad) is None
    assert grid_of_masks(masks) is not None


def test_wrappers_reject_bad_arguments_without_a_gpu():
    """Every rule but the last (CUDA tensors) is checked before the device is: each is exercised here by its own message."""
    from mirx.sbsm import sbsm_accumulate, sbsm_compose, sbsm_gain
    x = torch.zeros(2, 3, 8, 10)
    riv = torch.tensor([[0, 3], [2, 8]], dtype=torch.int32)
    civ = torch.tensor([[0, 4], [3, 7], [6, 10]], dtype=torch.int32)          # N = 6, the job has 12 images
    cases = [
        (lambda: sbsm_compose(x.double(), riv, civ, 0, 1), "float32"),
        (lambda: sbsm_compose(x[0], riv, civ, 0, 1), "4-d"),
        (lambda: sbsm_compose(x[:, :, :, ::2], riv, civ, 0, 1), "contiguous"),
        (lambda: sbsm_compose(x.numpy(), riv, civ, 0, 1), "tensor"),
        (lambda: sbsm_compose(x, riv.long(), civ, 0, 1), "int32"),
        (lambda: sbsm_compose(x, riv, civ.reshape(-1), 0, 1), "2-d"),
        (lambda: sbsm_compose(x, riv, civ.t().contiguous(), 0, 1), r"\[n, 2\]"),
        (lambda: sbsm_compose(x, riv, civ.repeat(1, 2)[:, ::2], 0, 1), "contiguous"),
        (lambda: sbsm_compose(x, riv, civ, -1, 1), "outside the job"),
        (lambda: sbsm_compose(x, riv, civ, 0, -1), "outside the job"),
        (lambda: sbsm_compose(x, riv, civ, 12, 1), "outside the job"),
        (lambda: sbsm_compose(x, riv, civ, 5, 8), "outside the job"),
        (lambda: sbsm_compose(x, riv, civ, 0, 2, out=torch.zeros(1, 3, 8, 10)), "out must hold"),
        (lambda: sbsm_compose(x, riv, civ, 0, 1, out=torch.zeros(1, 3, 8, 10, dtype=torch.float64)), "float32"),
        (lambda: sbsm_compose(x, riv, civ, 0, 1), "CUDA"),
        (lambda: sbsm_compose(x, riv, civ, 12, 0), "CUDA"),                   # an empty range at the end is in range
        (lambda: sbsm_gain(torch.zeros(2, 4).double(), torch.zeros(12, 4)), "float32"),
        (lambda: sbsm_gain(torch.zeros(2, 4), torch.zeros(12, 4, 1)), "2-d"),
        (lambda: sbsm_gain(torch.zeros(2, 8)[:, ::2], torch.zeros(12, 4)), "contiguous"),
        (lambda: sbsm_gain(torch.zeros(2, 4), torch.zeros(12, 5)), "width"),
        (lambda: sbsm_gain(torch.zeros(2, 4), torch.zeros(13, 4)), r"N \* B"),
        (lambda: sbsm_gain(torch.zeros(2, 4), torch.zeros(12, 4), torch.zeros(5, 4)), r"N \* B"),
        (lambda: sbsm_gain(torch.zeros(2, 16385), torch.zeros(12, 16385)), "16384"),
        (lambda: sbsm_gain(torch.zeros(0, 4), torch.zeros(12, 4)), "Q, B >= 1"),
        (lambda: sbsm_gain(torch.zeros(2, 4), torch.zeros(12, 4)), "CUDA"),
        (lambda: sbsm_gain(torch.zeros(2, 4), torch.zeros(12, 4), torch.zeros(3, 4)), "CUDA"),
        (lambda: sbsm_accumulate(torch.zeros(2, 6), riv, civ, (8, 10)), "float64"),
        (lambda: sbsm_accumulate(torch.zeros(6, dtype=torch.float64), riv, civ, (8, 10)), "2-d"),
        (lambda: sbsm_accumulate(torch.zeros(2, 12, dtype=torch.float64)[:, ::2], riv, civ, (8, 10)), "contiguous"),
        (lambda: sbsm_accumulate(torch.zeros(2, 5, dtype=torch.float64), riv, civ, (8, 10)), "gain must be"),
        (lambda: sbsm_accumulate(torch.zeros(2, 6, dtype=torch.float64), riv, civ, (2048, 1024)), "2\\^20"),
        (lambda: sbsm_accumulate(torch.zeros(2, 6, dtype=torch.float64), riv, civ, 8), "input_size"),
        (lambda: sbsm_accumulate(torch.zeros(2, 6, dtype=torch.float64), riv.float(), civ, (8, 10)), "int32"),
        (lambda: sbsm_accumulate(torch.zeros(2, 6, dtype=torch.float64), riv, civ, (8, 10)), "CUDA"),
    ]
    for call, message in cases:
        with pytest.raises(ValueError, match=message):
            call()


def test_check_intervals():
    from mirx.sbsm import check_intervals
    ok = np.array([[0, 3], [2, 8]], dtype=np.int32)
    check_intervals(ok, ok, (8, 8))
    for bad in (ok.astype(np.int64), ok.reshape(-1), np.array([[3, 3]], dtype=np.int32), np.array([[-1, 2]], dtype=np.int32),
                np.array([[4, 9]], dtype=np.int32), np.zeros((0, 2), dtype=np.int32)):
        with pytest.raises(ValueError):
            check_intervals(bad, ok, (8, 8))
        with pytest.raises(ValueError):
            check_intervals(ok, bad, (8, 8))


def _tiny_net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1),
                               torch.nn.Flatten()).eval()


@pytest.mark.parametrize("pair", [False, True])
def test_sbsm_batch_on_the_cpu_is_not_native(pair, tmp_path):
    """The CPU keeps the torch path (and its result): last_native is False, masks stays readable, a grid file is recognised."""
    from mirx.xai import SBSMBatch
    from oracle import xai as ox
    net = _tiny_net()
    g = torch.Generator().manual_seed(4)
    xq, xr = torch.randn(2, 3, 32, 40, generator=g), torch.randn(2, 3, 32, 40, generator=g)
    masks = R.sliding_window_masks((32, 40), 24, 5)
    ex = SBSMBatch(net, (32, 40), gpu_batch=7)
    assert ex.masks is None and ex.last_native is False
    ex.generate_masks(24, 5, savepath=str(tmp_path / "m.npy"))
    assert ex.N == 132 and ex._masks_t is None and ex._inv_t is None            # nothing of size N * HW yet
    assert np.array_equal(np.load(tmp_path / "m.npy"), masks)
    with torch.no_grad():
        want = ox.sbsm_batch(net, masks, xq, xr if pair else None, gpu_batch=7)
    got = ex(xq, xr if pair else None)
    assert ex.last_native is False
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-7)    # tests/test_xai_cpu.py's tolerance
    assert ex.masks.dtype == torch.uint8 and np.array_equal(ex.masks.numpy(), masks)
    ex2 = SBSMBatch(net, (32, 40), gpu_batch=7)
    ex2.load_masks(str(tmp_path / "m.npy"))
    assert ex2._intervals is not None and ex2.N == 132
    assert torch.equal(ex2(xq, xr if pair else None), got) and ex2.last_native is False
    flipped = masks.copy()
    flipped[5, 0, 0, 0] ^= 1
    np.save(tmp_path / "f.npy", flipped)
    ex3 = SBSMBatch(net, (32, 40), gpu_batch=7)
    ex3.load_masks(str(tmp_path / "f.npy"))
    assert ex3._intervals is None and np.array_equal(ex3.masks.numpy(), flipped)


@pytest.mark.parametrize("geom", [R.GEOMETRIES[1], R.GEOMETRIES[2]])
@pytest.mark.parametrize("pair", [False, True])
def test_restatement_matches_the_reference_tensors_in_float64(geom, pair):
    """tests/_sbsm_ref.py against oracle/xai.py:sbsm_batch, both in float64 on a tiny torch model; no mirx code runs.
    Tolerance: torch.cdist may take its matrix-product form (|a|^2 + |b|^2 - 2ab), whose float64 error in the SQUARED distance
    is at most about (D + 3) 2^-53 (|a|^2 + |b|^2); a distance is then off by at most the root of that, < 4e-8 for D = 8 and
    rows of norm <= 1 (the model's outputs are normalised), and the map is a mean of clamped differences of two distances:
    atol 1e-7.  The oracle returns its map rounded to float32: rtol 2^-24.  NaN positions (the uncovered pixels of the gapped
    geometry) must be equal."""
    from oracle import xai as ox
    h, w, window, stride = geom
    net = _tiny_net().double()
    model = lambda t: torch.nn.functional.normalize(net(t), dim=1)               # noqa: E731
    g = torch.Generator().manual_seed(6)
    xq = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64)
    xr = torch.randn(3, 3, h, w, generator=g, dtype=torch.float64) if pair else None
    masks = R.sliding_window_masks((h, w), window, stride)
    with torch.no_grad():
        want = ox.sbsm_batch(model, masks, xq, xr, gpu_batch=7).numpy()
        x = xq if xr is None else xr
        stack = (torch.from_numpy(masks)[:, None] * x[None]).reshape(-1, 3, h, w)          # n-major: row n * B + b
        e_q, e_m = model(xq).numpy(), model(stack).numpy()
        e_r = model(xr).numpy() if pair else None
    got = R.saliency(masks, e_q, e_m, e_r)
    assert got.shape == want.shape == ((6 if pair else 2), h, w)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want).any() == (geom == R.GEOMETRIES[2])
    np.testing.assert_allclose(got, want.astype(np.float64), rtol=2.0 ** -24, atol=1e-7, equal_nan=True)
