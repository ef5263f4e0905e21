"""GPU checks of mirx.ath: the Hamming search against the CPU oracle (ids and distances exactly equal), tie-heavy galleries, argument
checks, batch independence; the metric functions against the reference's fixture; the native ATHNet against the float64
restatement (tolerance: DESIGN 18), its batch independence, NaN containment, the absence of library ops and the weight cache."""
import os

import numpy as np
import pytest
import torch

import _ath_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "ath_ref.npz"))
TOL = 1e-5              # of the output scale (max |output| of the float64 restatement); DESIGN 18


def _bits(n, bits, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, bits), generator=g) < p).float()


def _check(q, g, k, exclude=None):
    from mirx.ath import hamming_topk
    ex = None if exclude is None else torch.as_tensor(exclude, dtype=torch.int64)
    d, i = hamming_topk(q.to(DEV), g.to(DEV), k, exclude_ids=None if ex is None else ex.to(DEV))
    od, oi = R.hamming_topk(q.numpy(), g.numpy(), k, None if ex is None else ex.numpy())
    assert d.dtype == torch.int32 and i.dtype == torch.int64 and tuple(d.shape) == (q.shape[0], k)
    np.testing.assert_array_equal(i.cpu().numpy(), oi)
    np.testing.assert_array_equal(d.cpu().numpy(), od)
    return d, i


# ---- Hamming search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 31, 32, 33, 36, 64, 65, 128, 1024])
@pytest.mark.parametrize("n,k", [(1, 1), (7, 7), (100, 10), (1000, 100), (4099, 1024), (65537, 10)])
def test_hamming_matches_oracle(bits, n, k):
    if bits == 1024 and n == 65537:
        n = 20011
    q = _bits(5, bits, seed=bits * 7 + n)
    g = _bits(n, bits, seed=bits * 13 + n + 1)
    g[n // 3] = q[0]                                         # an exact hit
    _check(q, g, k)
    if n > k:
        ex = torch.randint(0, n, (5,), generator=torch.Generator().manual_seed(n)).tolist()
        ex[0] = n // 3
        ex[1] = -1                                           # excludes nothing
        _check(q, g, k, ex)


def test_hamming_one_million_rows():
    q = _bits(6, 36, seed=1)
    g = _bits(1 << 20, 36, seed=2)
    _check(q, g, 100)
    _check(q, g, 10, [5, 17, 1 << 19, -1, 0, (1 << 20) - 1])


def test_hamming_k_equals_n_with_exclusion_refused():
    from mirx.ath import hamming_topk
    g = _bits(20, 36, seed=3)
    with pytest.raises(ValueError):
        hamming_topk(g[:2].to(DEV), g.to(DEV), 20, exclude_ids=torch.tensor([0, 3], device=DEV))
    _check(g[:2], g, 19, [0, 3])
    _check(g[:2], g, 20, [-1, 99])                          # exclusions outside the gallery leave every row


def test_tie_all_rows_identical():
    g = _bits(1, 36, seed=4).repeat(50000, 1)
    for k in (1, 10, 1024):
        d, i = _check(_bits(3, 36, seed=5), g, k)
        assert (i.cpu() == torch.arange(k)).all()


def test_tie_sixty_percent_equal_to_query():
    q = _bits(4, 64, seed=6)
    n = 70001
    g = _bits(n, 64, seed=7)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(8))
    hit = perm[: int(0.6 * n)]
    g[hit] = q[0]
    g[perm[int(0.6 * n): int(0.6 * n) + 2000]] = q[1]
    for k in (1, 10, 100, 1024):
        _check(q, g, k)
        _check(q, g, k, [int(hit.min()), -1, 0, 5])


def test_tie_all_zero_codes():
    g = torch.zeros((9000, 33))
    d, i = _check(torch.zeros((2, 33)), g, 1024)
    assert (d.cpu() == 0).all()
    _check(torch.ones((2, 33)), g, 100, [0, 8999])


def test_tie_rows_at_kth_distance_straddle_slices():
    # rows at distance 1 every 997 rows over a gallery of many slices, everything else far away: the k-th distance's rows spread
    # over slices, and m < (rows at d*) forces the in-order cut to cross slice boundaries
    n, bits = 300007, 64
    q = torch.zeros((3, bits))
    g = torch.ones((n, bits))
    at = torch.arange(0, n, 997)
    g[at] = 0
    g[at, 5] = 1
    g[12345] = 0                                           # one row at distance 0
    for k in (10, 100, 250, 302):
        _check(q, g, k)
        _check(q, g, k, [12345, int(at[3]), -1])


def test_hamming_input_dtypes():
    q, g = _bits(3, 40, seed=9), _bits(500, 40, seed=10)
    from mirx.ath import hamming_topk
    ref = hamming_topk(q.to(DEV), g.to(DEV), 20)
    for cast in (lambda t: t.to(torch.uint8), lambda t: t.bool()):
        out = hamming_topk(cast(q).to(DEV), cast(g).to(DEV), 20)
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


def test_hamming_bad_arguments():
    from mirx.ath import hamming_topk
    q, g = _bits(2, 36, seed=11).to(DEV), _bits(10, 36, seed=12).to(DEV)
    with pytest.raises(ValueError):
        hamming_topk(q, g, 11)
    with pytest.raises(ValueError):
        hamming_topk(torch.zeros((2, 1025), device=DEV), torch.zeros((10, 1025), device=DEV), 5)
    with pytest.raises(ValueError):
        hamming_topk(torch.zeros((2, 0), device=DEV), torch.zeros((10, 0), device=DEV), 5)
    with pytest.raises(ValueError):
        hamming_topk(q, g, 1025)
    for bad in (0.5, 2.0, -1.0, float("nan")):
        gb = g.clone()
        gb[3, 7] = bad
        with pytest.raises(ValueError, match="only 0 and 1"):
            hamming_topk(q, gb, 5)
    gu = g.to(torch.uint8)
    gu[0, 0] = 2
    with pytest.raises(ValueError, match="only 0 and 1"):
        hamming_topk(q.to(torch.uint8), gu, 5)


def test_hamming_batch_independent():
    from mirx.ath import hamming_topk
    g = _bits(100003, 36, seed=13).to(DEV)
    qs = _bits(4096, 36, seed=14).to(DEV)
    qs[100:2100] = g[5000]                                   # many tied queries among random ones
    d_all, i_all = hamming_topk(qs, g, 10)
    for j in (0, 150, 4095):
        d1, i1 = hamming_topk(qs[j:j + 1], g, 10)
        assert torch.equal(d1[0], d_all[j]) and torch.equal(i1[0], i_all[j])
    d2, i2 = hamming_topk(qs, g, 10)
    assert torch.equal(d2, d_all) and torch.equal(i2, i_all)


# ---- metric functions ----------------------------------------------------------------------------------------------------------
def _close(mine, ref):
    assert set(mine) == {int(k) for k in ref}
    for k, v in ref.items():
        for name, val in v.items():
            assert abs(mine[int(k)][name] - val) <= 1e-12, (k, name, mine[int(k)][name], val)


@pytest.mark.parametrize("case,binary", [("l2", False), ("bin", True), ("tie", True)])
def test_metrics_match_reference_fixture(case, binary):
    import json
    from mirx.ath import compute_metrics, compute_retrieval_metrics
    t = {k: torch.from_numpy(Z[f"{case}_{k}"]) for k in ("q", "g", "ql", "gl", "logits")}
    cm = compute_metrics(t["q"], t["ql"], t["g"], t["gl"], t["logits"], [1, 5, 10], binary)
    ref = json.loads(str(Z[f"met_{case}_cm"]))
    assert abs(cm["classification_acc"] - ref["classification_acc"]) <= 1e-12
    _close(cm["retrieval"], ref["retrieval"])
    rm = compute_retrieval_metrics(t["q"], t["ql"], t["g"], t["gl"], [1, 5, 10], binary)
    _close(rm, json.loads(str(Z[f"met_{case}_rm"])))


def test_metrics_refuse_non_binary_codes():
    from mirx.ath import compute_metrics
    q = torch.from_numpy(Z["bin_q"]).clone()
    q[0, 0] = 0.5
    with pytest.raises(ValueError):
        compute_metrics(q, torch.from_numpy(Z["bin_ql"]), torch.from_numpy(Z["bin_g"]), torch.from_numpy(Z["bin_gl"]),
                        torch.from_numpy(Z["bin_logits"]), [1, 5], True)


# ---- native ATHNet -------------------------------------------------------------------------------------------------------------
def _sd(m):
    return R.fixture_state_dict(Z, m)


def _net(m):
    from mirx.ath import ATHNet
    hs, nc, s = (int(v) for v in Z[f"{m}_cfg"])
    net = ATHNet(hs, nc, input_size=s)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in _sd(m).items()}, strict=True)
    return net.eval().to(DEV)


def _images(b, s, seed):
    return torch.rand((b, 3, s, s), generator=torch.Generator().manual_seed(seed))


def test_extract_codes_logits_labels_matches_fixture():
    from mirx.ath import extract_codes_logits_labels
    x, lab = R.fixture_images(Z, "m0"), torch.from_numpy(Z["m0_labels"])
    loader = [(x[:2], lab[:2]), (x[2:], lab[2:])]
    c, lg, lb = extract_codes_logits_labels(_net("m0"), loader, DEV, True)
    assert c.device.type == lg.device.type == lb.device.type == "cpu"
    scale = float(np.abs(Z["ext_logits"]).max())
    assert float((lg.double() - torch.from_numpy(Z["ext_logits"])).abs().max()) <= TOL * scale
    raw = Z["m0_codes"]
    ok = np.abs(raw) > TOL * np.abs(raw).max()
    np.testing.assert_array_equal(c.numpy()[ok], Z["ext_codes"][ok])
    assert torch.equal(lb, torch.from_numpy(Z["ext_labels"]))


@pytest.mark.parametrize("m", ["m0", "m1", "m2"])
@pytest.mark.parametrize("b", [1, 3, 64])
def test_native_forward_matches_float64(m, b):
    net = _net(m)
    s = int(Z[f"{m}_cfg"][2])
    x = _images(b, s, seed=b + s)
    if b <= 3 and Z[f"{m}_x4"].shape[0] >= b:
        x = R.fixture_images(Z, m)[:b]
    with torch.no_grad():
        c, lg = net(x.to(DEV))
    rc, rl = R.forward(_sd(m), x)
    for mine, ref in ((c, rc), (lg, rl)):
        scale = float(ref.abs().max())
        err = float((mine.double().cpu() - ref).abs().max())
        assert err <= TOL * scale, (m, b, err, scale)
    # binary codes: equal to the float64 signs except entries within the bound of 0 (listed)
    bound = TOL * float(rc.abs().max())
    near = (rc.abs() <= bound)
    assert int(near.sum()) <= max(1, rc.numel() // 1000), [(i, j, float(rc[i, j])) for i, j in near.nonzero().tolist()]
    assert torch.equal((c.cpu() >= 0)[~near], (rc >= 0)[~near])


def test_native_batch_independent_and_nan_contained():
    net = _net("m0")
    x = _images(64, 64, seed=21).to(DEV)
    with torch.no_grad():
        c, lg = net(x)
        for sl in (slice(0, 1), slice(5, 9), slice(63, 64)):
            c1, l1 = net(x[sl].contiguous())
            assert torch.equal(c1, c[sl]) and torch.equal(l1, lg[sl])
        xn = x.clone()
        xn[7, 1, 10, 10] = float("nan")
        cn, ln = net(xn)
    keep = torch.ones(64, dtype=torch.bool)
    keep[7] = False
    assert torch.equal(cn[keep], c[keep]) and torch.equal(ln[keep], lg[keep])
    assert torch.isnan(cn[7]).any()


def test_native_forward_has_no_library_ops():
    from torch.profiler import ProfilerActivity, profile
    net = _net("m2")
    x = _images(2, 256, seed=22).to(DEV)
    with torch.no_grad():
        net(x)
    with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
        net(x)
    names = {e.name for e in prof.events()}
    banned = ("conv", "convolution", "linear", "mm", "addmm", "matmul", "max_pool", "avg_pool", "mean", "sigmoid")
    bad = [nm for nm in names if nm.startswith("aten::") and any(nm[6:] == b or nm[6:].startswith(b) or nm[6:] == "_" + b
                                                                 for b in banned)]
    assert not bad, bad


def test_native_cache_follows_weights():
    net = _net("m1")
    s = int(Z["m1_cfg"][2])
    x = _images(3, s, seed=23)

    def check():
        with torch.no_grad():
            c, lg = net(x.to(DEV))
        sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in net.state_dict().items()}
        rc, rl = R.forward(sd, x)
        assert float((c.double().cpu() - rc).abs().max()) <= TOL * float(rc.abs().max())
        assert float((lg.double().cpu() - rl).abs().max()) <= TOL * float(rl.abs().max())
        return c

    c0 = check()
    with torch.no_grad():
        net.net1[0].net[3].weight.mul_(1.3)
    c1 = check()
    assert not torch.equal(c0, c1)
    with torch.no_grad():
        net.net2[0].net[1].running_var.mul_(2.0)
    c2 = check()
    assert not torch.equal(c1, c2)
    with torch.no_grad():
        net.hashlayer.bias.add_(0.25)
    c3 = check()
    assert not torch.equal(c2, c3)
    net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in _sd("m1").items()})
    c4 = check()
    assert torch.equal(c4, c0)


def test_eager_path_outside_the_gate():
    net = _net("m0")
    x = R.fixture_images(Z, "m0").to(DEV)
    net.train()
    c, _ = net(x)                                            # training mode: the torch graph (batch statistics)
    assert c.requires_grad
    net.eval()
    with torch.no_grad():
        ce, _ = net.forward_eager(x)
        cn, _ = net(x)
    assert float((ce - cn).abs().max()) <= TOL * float(ce.abs().max())
