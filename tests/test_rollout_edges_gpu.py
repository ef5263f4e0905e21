"""The k_rollout.hip kernels off the SigLIP tower's geometry, against float64 only (_rollout_ref and float64 torch): the generic
head_dim layer kernel (tail-only, block + tail, no tail, the limit), head counts whose splits are uneven or short, the
pipelined tile loop at every count of tiles at which a wave idles or leaves at another break, constructed scores that overflow
or underflow a softmax with a wrong row maximum, the row stage on wrapped diagonals, negatives and signed zeros, the chain and
finish on non-square grids, even and odd layer counts, downscales and identity sizes, and bit-identical batches and chunks at a
geometry no tower has.  Every case prints its figures (`EDGE ...`) before it asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rollout_ref as R
from _rollout_ref import _audited_expected, _fused64, _score_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
CONFIGS = [("mean", 0.9), ("max", 0.0), ("min", 0.0)]            # section 2: the discard with mean, none with max / min


def _layer_slot1(qkv, heads, dh, fusion, k):
    """mirx_rollout_layer into slot 1 of a NaN-filled 2-layer workspace -> A_1 [b, n, n]; slot 0 and everything behind the
    split scratch (the chain partials and the importance) must still be NaN."""
    from mirx.rollout import rollout_layer, workspace_floats
    b, n, _ = qkv.shape
    nn_ = b * n * n
    ws = torch.full((workspace_floats(2, b, n),), float("nan"), device=DEV)
    rollout_layer(qkv.to(DEV), heads, dh ** -0.5, fusion, k, 1, 2, ws)
    got = ws[nn_:2 * nn_].view(b, n, n)
    assert not torch.isnan(got).any()
    assert torch.isnan(ws[:nn_]).all(), "layer 0's slot was written"
    assert ws.numel() == 6 * nn_ + 17 * b * n and torch.isnan(ws[6 * nn_:]).all(), "the chain / importance tail was written"
    return got


def _layer_tol(qkv, heads, dh):
    n = qkv.shape[1]
    eb = _score_bound(qkv, heads, dh, dh ** -0.5)
    return 2 * eb * (1 + 2 * eb) + (n + heads + 4) * U            # the fused value's relative error bound


def _check_layer(tag, n, dh, heads, b, fusion, ratio):
    gen = torch.Generator().manual_seed(n * 7 + dh + heads)
    qkv = torch.randn(b, n, 3 * heads * dh, generator=gen)
    k = max(1, int(n * ratio)) if ratio > 0 else 0
    got = _layer_slot1(qkv, heads, dh, fusion, k)
    tol = _layer_tol(qkv, heads, dh)
    exp, flips = _audited_expected(_fused64(qkv, heads, dh, dh ** -0.5, fusion), got, k, tol)
    err = ((got.double() - exp).abs() / (exp + 1e-30)).max().item()
    cap = b * n * n // 1000
    print(f"EDGE {tag} n{n} d{dh} h{heads} b{b} {fusion} k{k}: err {err:.3e} tol {tol:.3e} err/tol {err / tol:.3f} flips {flips} cap {cap}")
    assert flips <= cap, (flips, cap)
    assert err <= tol + 2 * (n + 4) * U, (err, tol)


# ---- 1. the generic head_dim kernel -----------------------------------------------------------------------------------
GENERIC_GEOMS = [(1, 4, 1, 2), (15, 20, 3, 2), (17, 12, 5, 1), (65, 8, 1, 1), (33, 32, 9, 2), (80, 100, 7, 1), (257, 128, 6, 1)]


@pytest.mark.parametrize("n,dh,heads,b", GENERIC_GEOMS, ids=[f"n{n}_d{d}_h{h}_b{b}" for n, d, h, b in GENERIC_GEOMS])
@pytest.mark.parametrize("fusion", ["mean", "max", "min"])
@pytest.mark.parametrize("ratio", [0.0, 0.9])
def test_generic_head_dim_matches_float64(n, dh, heads, b, fusion, ratio):
    _check_layer("s1", n, dh, heads, b, fusion, ratio)


# ---- 2. head splits and tile-loop edges on the compiled head_dims -----------------------------------------------------
@pytest.mark.parametrize("heads", [1, 3, 5, 6, 7, 9])
@pytest.mark.parametrize("dh,n", [(64, 40), (72, 33)])
@pytest.mark.parametrize("fusion,ratio", CONFIGS)
def test_head_splits_match_float64(heads, dh, n, fusion, ratio):
    _check_layer("s2-heads", n, dh, heads, 1 + heads % 2, fusion, ratio)


TILE_NS = [1, 17, 40, 64, 65, 128, 129, 192, 200]                # ntiles 1, 2, 3, 4, 5, 8, 9, 12, 13


@pytest.mark.parametrize("n", TILE_NS)
@pytest.mark.parametrize("dh", [64, 72])
@pytest.mark.parametrize("fusion,ratio", CONFIGS)
def test_tile_loop_edges_match_float64(n, dh, fusion, ratio):
    _check_layer("s2-tiles", n, dh, 2, 1 + TILE_NS.index(n) % 2, fusion, ratio)


# ---- 3. scores that need the row maximum ------------------------------------------------------------------------------
def _constructed_qkv(n, dh, heads, peaked):
    """One image whose scores are A_i K[j, d_i] + B_i (row i of head h reads d_i = (i + h) % (dh - 1); K[:, dh - 1] = 1 carries
    B_i).  Flat rows: K uniform in [-1, 1], A_i in {1, 30}.  Peaked rows: A_i = 60, K = +1 at the one key
    p_i = (0, 63, 64, n - 1)[i % (dh - 1) % 4] (the same key in every head) and in [-1, -0.5] at every other key.  B_i cycles
    over 0, +200, -200: it cancels in the softmax, and overflows or underflows one that does not subtract the row maximum."""
    gen = torch.Generator().manual_seed(n + dh + heads)
    scale = dh ** -0.5
    x = torch.randn(n, 3, heads, dh, generator=gen)
    planted = (0, 63, 64, n - 1)
    i = torch.arange(n)
    a = torch.full((n,), 60.0) if peaked else torch.tensor([1.0, 30.0])[i % 2]
    bias = torch.tensor([0.0, 200.0, -200.0])[i % 3]
    for h in range(heads):
        if peaked:
            kk = -0.5 - 0.5 * torch.rand(n, dh, generator=gen)
            for d in range(dh - 1):
                kk[planted[(d - h) % (dh - 1) % 4], d] = 1.0
        else:
            kk = 2.0 * torch.rand(n, dh, generator=gen) - 1.0
        kk[:, dh - 1] = 1.0
        q = torch.zeros(n, dh)
        q[i, (i + h) % (dh - 1)] = a / scale
        q[:, dh - 1] = bias / scale
        x[:, 0, h], x[:, 1, h] = q, kk
    return x.reshape(1, n, 3 * heads * dh).contiguous()


@pytest.mark.parametrize("n,dh,heads", [(130, 72, 3), (130, 20, 2), (70, 8, 5)])
@pytest.mark.parametrize("fusion", ["mean", "max", "min"])
@pytest.mark.parametrize("rows", ["flat", "peaked"])
def test_softmax_needs_the_row_maximum(n, dh, heads, fusion, rows):
    qkv = _constructed_qkv(n, dh, heads, rows == "peaked")
    got = _layer_slot1(qkv, heads, dh, fusion, 0).double()
    tol = _layer_tol(qkv, heads, dh)
    exp, _ = _audited_expected(_fused64(qkv, heads, dh, dh ** -0.5, fusion), got, 0, tol)
    big = exp >= 2.0 ** -100                     # below it the f32 exponential may be denormal: no relative accuracy there
    err = ((got - exp).abs() / exp)[big].max().item()
    small_max = got[~big].max().item() if (~big).any() else 0.0
    print(f"EDGE s3 n{n} d{dh} h{heads} {fusion} {rows}: err {err:.3e} tol {tol:.3e} err/tol {err / tol:.3f} "
          f"min exp {exp.min().item():.2e} entries below 2^-100: {int((~big).sum())}, largest got there {small_max:.2e}")
    if rows == "peaked":
        assert big.any(-1).all() and (~big).any(-1).all()           # every row has its peak and its underflowing entries
    else:
        assert big.all()
    assert err <= tol + 2 * (n + 4) * U, (err, tol)
    assert (got[~big] >= 0).all() and small_max <= 2.0 ** -99


# ---- 4. the row stage -------------------------------------------------------------------------------------------------
ROW_CASES = [(37, 16, 8), (5, 1, 1), (5, 1, 0), (9, 64, 32), (9, 65, 64), (130, 64, 1)]


def _row_content(rows, n, k, rng):
    """Dyadic values (every row sum is exact in f32, so rows with negatives lose nothing to cancellation), by row % 6:
    0, 5 tie-heavy positives; 1 all negative; 2 -0.0, +0.0 and positives; 3 exactly max(k, 1) negatives, so that the k-th
    smallest is negative; 4 ties planted at the threshold."""
    a = (rng.integers(1, 40, size=(rows, n)) / 64.0).astype(np.float32)
    for r in range(rows):
        kind = r % 6
        if kind == 1:
            a[r] = -a[r]
        elif kind == 2:
            a[r, 0::3] = -0.0
            a[r, 1::3] = 0.0
        elif kind == 3:
            neg = rng.permutation(n)[:max(k, 1)]
            a[r, neg] = -a[r, neg]
        elif kind == 4 and k > 0:
            a[r, rng.permutation(n)[:3]] = np.partition(a[r], k - 1)[k - 1]
    return a


@pytest.mark.parametrize("rows,n,k", ROW_CASES, ids=[f"r{r}_n{n}_k{k}" for r, n, k in ROW_CASES])
def test_row_stage_wrapped_diagonal_and_signs(rows, n, k):
    from mirx.rollout import rollout_rows_
    a = _row_content(rows, n, k, np.random.default_rng(rows + n + k))
    assert np.signbit(a[2, 0]) and a[1].max() < 0
    got = rollout_rows_(torch.from_numpy(a.copy()).to(DEV), k).cpu().numpy()
    keep = a > np.partition(a, k - 1, axis=1)[:, k - 1:k] if k > 0 else np.ones_like(a, bool)
    if k > 0:
        assert np.partition(a[3], k - 1)[k - 1] < 0
    idx = np.arange(rows)
    off = np.ones_like(keep)
    off[idx, idx % n] = False
    assert np.array_equal((got != 0) & off, keep & (a != 0) & off)
    exp = R.row_stage(a, k)
    err = np.abs(got - exp).max(axis=1) / np.abs(exp).max(axis=1)
    print(f"EDGE s4 rows{rows} n{n} k{k}: err {err.max():.3e} bound {(n + 8) * U:.3e} err/bound {err.max() / ((n + 8) * U):.3f}")
    assert np.abs(got - exp).max() <= (n + 8) * U * np.abs(exp).max()
    assert (err <= (n + 8) * U).all(), err.max()                    # per row too: the sums are exact, no row hides behind another


# ---- 5. chain and finish ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(2, 8), (5, 3), (1, 7), (1, 1), (3, 3)])
@pytest.mark.parametrize("L", [1, 2, 5])
def test_chain_and_finish_off_the_square(h, w, L):
    from mirx.rollout import rollout_finish, workspace_floats
    n, b, negated = h * w, 3, 1
    gen = torch.Generator().manual_seed(100 * h + 10 * w + L)
    mats = torch.rand(L, b, n, n, generator=gen) * (torch.rand(L, b, n, n, generator=gen) > 0.8)
    mats = mats + torch.eye(n)
    mats = mats / mats.sum(-1, keepdim=True)
    ws = torch.full((workspace_floats(L, b, n),), float("nan"), device=DEV)       # the matrices and nothing else
    ws[:L * b * n * n] = mats.reshape(-1).to(DEV)
    v = R.importance(list(mats.double().numpy()))
    sizes = [(3 * h + 2, 2 * w + 5), (max(1, h // 2), max(1, w // 2)), (1, 1), (h, w), (17, w + 3)]
    worst = 0.0
    for e in (None, 1, 6, 70):
        bound = (L * (n + 4) + 16) * U                              # f32 sums of non-negative terms: the chain's bound
        imp, keep = v, np.arange(b)
        if e is not None:
            patches = F.normalize(torch.randn(b, n, e, generator=gen), dim=-1)
            query = F.normalize(torch.randn(e, generator=gen), dim=0)
            dots = (patches * query).sum(-1)
            patches[negated] = patches[negated] * torch.where(dots[negated] > 0, -1.0, 1.0)[:, None]    # every dot negative
            patches[0, 0] = patches[0, 0] * (1.0 if dots[0, 0] > 0 else -1.0)    # image 0 keeps one positive dot
            sim = np.maximum((patches.double().numpy() * query.double().numpy()).sum(-1), 0)
            assert (sim[negated] == 0).all() and sim.max() > 0
            imp = v * sim
            bound += (e + 2) * U / sim.max()                        # the dot of unit vectors: |error| <= e u
            keep = np.array([i for i in range(b) if i != negated])
        for size in sizes:
            if e is None:
                out = rollout_finish(ws, L, b, h, w, size)
            else:
                out = rollout_finish(ws, L, b, h, w, size, patches.to(DEV), query.to(DEV))
                assert (out[negated] == 0).all()
            exp = R.resize_bilinear(imp.reshape(b, h, w), *size)
            # the bound is relative to the largest cell of the map; an output that subsamples the map may miss that cell (one
            # sample at (1, 1), possibly a cell whose similarity is 0), so there the map's own maximum is the scale
            ref = exp[keep] if size[0] >= h and size[1] >= w else imp[keep]
            err = np.abs(out.cpu().numpy() - exp)[keep].max() / np.abs(ref).max()
            worst = max(worst, err / bound)
            assert err <= bound, (e, size, err, bound)
    assert torch.equal(ws[:L * b * n * n].view(L, b, n, n).cpu(), mats)          # the finish leaves the matrices alone
    print(f"EDGE s5 grid {h}x{w} L{L}: largest err/bound {worst:.3f}")


# ---- 6. bit-identity off the tower's geometry -------------------------------------------------------------------------
@pytest.mark.parametrize("fusion,k", [("max", 72), ("mean", 72), ("min", 0)])
def test_batches_and_chunks_are_bit_identical_off_the_tower(fusion, k):
    from mirx.rollout import rollout_maps, workspace_floats
    n, dh, heads, L, e = 80, 100, 7, 2, 24
    gen = torch.Generator().manual_seed(6)
    qkvs = [torch.randn(3, n, 3 * heads * dh, generator=gen).to(DEV) for _ in range(L)]
    patches = F.normalize(torch.randn(3, n, e, generator=gen), dim=-1).to(DEV)
    query = F.normalize(torch.randn(e, generator=gen), dim=0).to(DEV)
    args = (heads, dh ** -0.5, fusion, k, 8, 10, (21, 13))
    three = rollout_maps(qkvs, *args, patches=patches, query=query)
    assert torch.isfinite(three).all() and (three > 0).any()
    for i in range(3):
        one = rollout_maps([q[i:i + 1].contiguous() for q in qkvs], *args, patches=patches[i:i + 1].contiguous(), query=query)
        assert torch.equal(one[0], three[i])
    per = workspace_floats(L, 1, n)
    for budget in (per, 2 * per + 5):                               # chunks of 1 and 2 images
        assert torch.equal(rollout_maps(qkvs, *args, patches=patches, query=query, budget=budget), three)
