"""ConvNeXtV2_SRA / ConvNeXtV2_PCAM on the MI355X: the attention-pooling head kernels (mirx_sra_head_nhwc, mirx_pcam_head_nhwc) on
the reference's own fixture and against float64, their batch independence, containment and argument checks, and both models end
to end against the float64 restatement in _sra_ref."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _sra_ref import embed_pcam, embed_sra, pcam_head, randomize, sra_head

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sra_pcam_heads.npz")


def _lib():
    from mirx import _lib as L
    return L


def _ptr(t):
    from mirx.model import _ptr as p
    return p(t)


def _st():
    from mirx.model import _stream
    return _stream(torch.device(DEV))


def _rows(x):
    """NCHW [n, c, h, w] -> device fp32 rows [n * h * w, c] (the backbone's channels-last stream)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).float().contiguous().to(DEV)


def _sra_kernel(x, w, nw, nb, lam, normalize):
    n, c = x.shape[:2]
    hw = x.shape[2] * x.shape[3]
    t, wd, g, b = _rows(x), w.reshape(-1, c).float().contiguous().to(DEV), nw.float().to(DEV), nb.float().to(DEV)
    y = torch.empty((n, c), dtype=torch.float32, device=DEV)
    L = _lib()
    L.check(L.load().mirx_sra_head_nhwc(_ptr(t), n, hw, c, _ptr(wd), wd.shape[0], _ptr(g), _ptr(b), 1e-6, lam, int(normalize), _ptr(y),
                                        _st()))
    torch.cuda.synchronize()
    return y.cpu()


def _pcam_kernel(x, w, bias, nw, nb, lam, normalize, logits=True):
    n, c = x.shape[:2]
    hw = x.shape[2] * x.shape[3]
    k = w.shape[0]
    t, wd, bd = _rows(x), w.reshape(k, c).float().contiguous().to(DEV), bias.float().contiguous().to(DEV)
    g, b = nw.float().to(DEV), nb.float().to(DEV)
    y = torch.empty((n, c), dtype=torch.float32, device=DEV)
    lg = torch.full((n, k), float("nan"), dtype=torch.float32, device=DEV)
    L = _lib()
    L.check(L.load().mirx_pcam_head_nhwc(_ptr(t), n, hw, c, _ptr(wd), _ptr(bd), k, _ptr(g), _ptr(b), 1e-6, lam, int(normalize), _ptr(y),
                                         _ptr(lg) if logits else None, _st()))
    torch.cuda.synchronize()
    return y.cpu(), lg.cpu()


def _close(got, want, normalized, tol=1e-6):
    err = float((got.double() - want).abs().max())
    bound = tol if normalized else tol * float(want.abs().max())
    assert err <= bound, (err, bound)


def _close_logits(got, want, x, wt, bias, nw, nb, tol=1e-6):
    """class logits = b + sum_p q[p] (w . z[p]): a dot product with cancellation, so its error is measured against the sum of
    the absolute values of its terms, |b| + sum_p q[p] sum_c |w[c] z[p, c]|."""
    n, c = x.shape[:2]
    x, wt, bias, nw, nb = (v.double() for v in (x, wt, bias, nw, nb))
    z = F.layer_norm(x.permute(0, 2, 3, 1), (c,), nw, nb, 1e-6).reshape(n, -1, c)                 # [n, hw, c]
    q = torch.sigmoid(torch.einsum("kc,npc->nkp", wt, z) + bias[None, :, None])
    q = q / (q.sum(dim=2, keepdim=True) + 1e-8)
    scale = bias.abs()[None] + torch.einsum("nkp,kc,npc->nk", q, wt.abs(), z.abs())
    assert bool(((got.double() - want).abs() <= tol * scale).all()), float(((got.double() - want).abs() / scale).max())


# ---- the kernels on the reference's own fixture ----------------------------------------------------------------------------
def test_kernels_on_reference_fixture():
    gold = dict(np.load(GOLD))
    nw, nb = torch.from_numpy(gold["norm_w"]), torch.from_numpy(gold["norm_b"])
    for hw in ("12x12", "5x7"):
        x = torch.from_numpy(gold[f"x_{hw}"])
        for lam in (0.1, 1.0):
            tag = f"l{round(10 * lam)}"
            for k in (1, 8):
                y = _sra_kernel(x, torch.from_numpy(gold[f"sra_w_k{k}"]), nw, nb, lam, normalize=False)
                _close(y, torch.from_numpy(gold[f"sra_{hw}_k{k}_{tag}"]), normalized=False)
            for k in (3, 14):
                w, b = torch.from_numpy(gold[f"pcam_w_k{k}"]), torch.from_numpy(gold[f"pcam_b_k{k}"])
                p = f"pcam_{hw}_k{k}_{tag}_fc"
                emb, lg = _pcam_kernel(x, w, b, nw, nb, lam, normalize=True)
                _close(emb, torch.from_numpy(gold[p + "0_embedding"]), normalized=True)
                _close_logits(lg, torch.from_numpy(gold[p + "0_class_logits"]), x.double(), w.double().reshape(k, -1), b.double(),
                              nw.double(), nb.double())
                feat, _ = _pcam_kernel(x, w, b, nw, nb, lam, normalize=False, logits=False)     # an fc follows: feat unnormalised
                emb_fc = F.normalize(F.linear(feat.double(), torch.from_numpy(gold["fc_w"]).double(),
                                              torch.from_numpy(gold["fc_b"]).double()), dim=1)
                _close(emb_fc, torch.from_numpy(gold[p + "1_embedding"]), normalized=True)


# ---- the kernels against float64 over shapes --------------------------------------------------------------------------------
SIDES = {1: (1, 1), 35: (5, 7), 144: (12, 12), 576: (24, 24)}


def _inputs(n, hw, c, k, seed):
    g = torch.Generator().manual_seed(seed)
    h, w = SIDES[hw]
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) + 0.5 * torch.randn(n, c, 1, 1, generator=g, dtype=torch.float64)
    x = x.float().double()                                                  # exactly what the kernel reads
    wt = (2.5 / c ** 0.5 * torch.randn(k, c, generator=g, dtype=torch.float64)).float().double()
    bias = (0.5 * torch.randn(k, generator=g, dtype=torch.float64)).float().double()
    nw = (0.5 + torch.rand(c, generator=g, dtype=torch.float64)).float().double()
    nb = (0.1 * torch.randn(c, generator=g, dtype=torch.float64)).float().double()
    return x, wt, bias, nw, nb


@pytest.mark.parametrize("k", [1, 8, 16])
@pytest.mark.parametrize("c", [64, 1024])
@pytest.mark.parametrize("hw", [1, 35, 144, 576])
def test_sra_kernel_matches_float64(hw, c, k):
    for n in (1, 5):
        x, wt, _, nw, nb = _inputs(n, hw, c, k, seed=hw * 7 + c + k + n)
        want = sra_head(x, wt, nw, nb, 0.3)
        _close(_sra_kernel(x, wt, nw, nb, 0.3, normalize=False), want, normalized=False)
        _close(_sra_kernel(x, wt, nw, nb, 0.3, normalize=True), F.normalize(want, dim=1), normalized=True)
        # sensitivity: a kernel that dropped the attention branch would give lam = 1 == lam = 0
        d = _sra_kernel(x, wt, nw, nb, 1.0, normalize=False) - _sra_kernel(x, wt, nw, nb, 0.0, normalize=False)
        assert float(d.abs().max()) >= 1e-2


@pytest.mark.parametrize("k", [1, 3, 14])
@pytest.mark.parametrize("c", [64, 1024])
@pytest.mark.parametrize("hw", [1, 35, 144, 576])
def test_pcam_kernel_matches_float64(hw, c, k):
    for n in (1, 5):
        x, wt, bias, nw, nb = _inputs(n, hw, c, k, seed=hw * 5 + c + k + n)
        emb, logits, _, feat = pcam_head(x, wt, bias, nw, nb, 0.3)
        y, lg = _pcam_kernel(x, wt, bias, nw, nb, 0.3, normalize=False)
        _close(y, feat, normalized=False)
        _close_logits(lg, logits, x, wt, bias, nw, nb)
        y, lg = _pcam_kernel(x, wt, bias, nw, nb, 0.3, normalize=True, logits=False)
        _close(y, emb, normalized=True)
        assert torch.isnan(lg).all()                                   # NULL logits: nothing written
        d = _pcam_kernel(x, wt, bias, nw, nb, 1.0, normalize=False)[0] - _pcam_kernel(x, wt, bias, nw, nb, 0.0, normalize=False)[0]
        assert float(d.abs().max()) >= 1e-2


def test_kernels_batch_independent_and_contained():
    x, wt, bias, nw, nb = _inputs(5, 144, 1024, 8, seed=11)
    runs = {"sra": lambda v: _sra_kernel(v, wt, nw, nb, 0.1, True),
            "pcam": lambda v: torch.cat(_pcam_kernel(v, wt[:3], bias[:3], nw, nb, 0.1, True), dim=1)}
    for name, run in runs.items():
        full = run(x)
        for i in range(5):
            assert torch.equal(run(x[i:i + 1])[0], full[i]), (name, i)
        bad = x.clone()
        bad[2, 5, 3, 4] = float("nan")
        dirty = run(bad)
        assert torch.equal(dirty[[0, 1, 3, 4]], full[[0, 1, 3, 4]]), name
        assert not torch.isfinite(dirty[2]).all(), name


def test_out_of_bound_arguments_do_not_launch():
    L = _lib()
    lib = L.load()
    x = torch.randn(2 * 144, 1024, device=DEV)
    w = torch.randn(65, 1024, device=DEV)
    b = torch.zeros(65, device=DEV)
    g, be = torch.ones(8192, device=DEV), torch.zeros(8192, device=DEV)
    y = torch.full((2, 8192), 7.0, device=DEV)
    st = _st()
    cases = [  # (n, hw, c, K, x offset in floats, what the message names)
        (2, 144, 1022, 8, 0, b"multiple of 4"), (2, 144, 0, 8, 0, b"multiple of 4"), (1, 8, 8196, 8, 0, b"8192"),
        (2, 144, 1024, 0, 0, b"K"), (2, 144, 1024, 65, 0, b"K"), (2, 0, 1024, 8, 0, b"hw"), (1, 288, 1024, 54, 0, b"16384"),
        (-1, 144, 1024, 8, 0, b"batch"), (1, 144, 1020, 8, 1, b"aligned"),
    ]
    for n, hw, c, k, off, msg in cases:
        xp = _ptr_at(x, off)
        rc = lib.mirx_sra_head_nhwc(xp, n, hw, c, _ptr(w), k, _ptr(g), _ptr(be), 1e-6, 0.1, 1, _ptr(y), st)
        assert rc != 0 and msg in lib.mirx_last_error(), (n, hw, c, k, lib.mirx_last_error())
        rc = lib.mirx_pcam_head_nhwc(xp, n, hw, c, _ptr(w), _ptr(b), k, _ptr(g), _ptr(be), 1e-6, 0.1, 1, _ptr(y), None, st)
        assert rc != 0 and msg in lib.mirx_last_error(), (n, hw, c, k, lib.mirx_last_error())
    rc = lib.mirx_pcam_head_nhwc(_ptr(x), 2, 144, 1024, _ptr(w), None, 3, _ptr(g), _ptr(be), 1e-6, 0.1, 1, _ptr(y), None, st)
    assert rc != 0 and b"b_cls" in lib.mirx_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                      # nothing was launched
    # the largest admitted LDS use runs: (64 + 3) * 244 = 16348 floats
    xs = torch.randn(1, 64, 4, 61, dtype=torch.float64)
    ws = 0.3 * torch.randn(64, 64, dtype=torch.float64)
    nw, nb = torch.ones(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    _close(_sra_kernel(xs, ws, nw, nb, 0.5, normalize=False), sra_head(xs.float().double(), ws.float().double(), nw, nb, 0.5),
           normalized=False)


def _ptr_at(t, off_floats):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * off_floats)


# ---- the models end to end ----------------------------------------------------------------------------------------------------
def _images(n, seed=1, size=384):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


def _sra_model(seed=0, k=8, lam=0.5):
    from mirx.model import ConvNeXtV2_SRA
    torch.manual_seed(seed)
    return randomize(ConvNeXtV2_SRA(num_heads=k, lam=lam), seed=seed + 1).eval().to(DEV)


def _pcam_model(dim=None, seed=0, k=3, lam=0.5):
    from mirx.model import ConvNeXtV2_PCAM
    torch.manual_seed(seed)
    return randomize(ConvNeXtV2_PCAM(num_classes=k, lam=lam, embedding_dim=dim), seed=seed + 1).eval().to(DEV)


def _eager_fp32(m, x):
    """The same module's torch graph in fp32 on the GPU (grad mode routes every block to its library ops)."""
    with torch.enable_grad():
        return m(x).detach()


@pytest.mark.parametrize("which", ["sra", "pcam", "pcam256"])
def test_end_to_end_matches_float64(which):
    m = _sra_model() if which == "sra" else _pcam_model(256 if which == "pcam256" else None)
    x = _images(2)
    with torch.no_grad():
        y = m(x.to(DEV))
    eager = _eager_fp32(m, x.to(DEV))
    ref = embed_sra(x, m.state_dict(), 0.5) if which == "sra" else embed_pcam(x, m.state_dict(), 0.5)
    err_native = float((y.cpu().double() - ref).abs().max())
    err_eager = float((eager.cpu().double() - ref).abs().max())
    print(f"{which}: native {err_native:.3e}, eager fp32 {err_eager:.3e}")
    assert y.shape == (2, 256 if which == "pcam256" else 1024)
    assert torch.allclose(y.norm(dim=1), torch.ones(2, device=DEV), atol=1e-5)
    assert err_native <= max(1e-5, 2 * err_eager)


def test_batch_independence():
    for m in (_sra_model(seed=3), _pcam_model(seed=3)):
        x = _images(16, seed=4).to(DEV)
        with torch.no_grad():
            full = m(x)
            parts = torch.cat([m(x[i:i + 2]) for i in range(0, 16, 2)])
        assert float((full - parts).abs().max()) <= 1e-6


def test_native_path_runs_no_library_ops():
    from torch.profiler import ProfilerActivity, profile
    x = _images(2, seed=6).to(DEV)
    for m in (_sra_model(seed=5), _pcam_model(dim=128, seed=5)):
        with torch.no_grad():
            m(x)
        with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
            m(x)
        names = {e.name for e in prof.events()}
        banned = ("mean", "softmax", "_softmax", "bmm", "layer_norm", "native_layer_norm", "linear", "matmul", "mm", "addmm", "einsum",
                  "conv")
        bad = [nm for nm in names if nm.startswith("aten::") and any(nm[6:] == b or nm[6:].startswith(b + "_") or nm[6:] == "_" + b
                                                                     for b in banned)]
        assert not bad, bad
        assert not any("convolution" in nm for nm in names)


def test_cache_follows_the_weights():
    m = _sra_model(seed=7)
    p = _pcam_model(seed=7)
    x = _images(2, seed=8, size=64)
    with torch.no_grad():
        m(x.to(DEV))
        m.sra.conv_att.weight.mul_(-3.0)
        y = m(x.to(DEV))
        _close(y.cpu(), embed_sra(x, m.state_dict(), 0.5), normalized=True, tol=1e-5)
        m.convnext.head.norm.weight.add_(0.7)
        y = m(x.to(DEV))
        _close(y.cpu(), embed_sra(x, m.state_dict(), 0.5), normalized=True, tol=1e-5)
        other = randomize(_sra_model(seed=9), seed=10)
        m.load_state_dict(other.state_dict())
        y = m(x.to(DEV))
        _close(y.cpu(), embed_sra(x, other.state_dict(), 0.5), normalized=True, tol=1e-5)
        p(x.to(DEV))
        p.pcam.classifier.weight.mul_(2.0)
        p.pcam.classifier.bias.add_(1.0)
        y = p(x.to(DEV))
        _close(y.cpu(), embed_pcam(x, p.state_dict(), 0.5), normalized=True, tol=1e-5)


def test_retrieval_round_trip():
    from mirx.retriever import MODEL_CONFIGS, MilvusManager
    m = _sra_model(seed=12)
    x = _images(6, seed=13).to(DEV)
    with torch.no_grad():
        e = m(x)
    assert e.shape == (6, MODEL_CONFIGS["convnextv2_sra"]["embedding_dim"])
    mgr = MilvusManager(dataset="covid")
    mgr.connect()
    col = mgr.create_collection("convnextv2_sra", drop_old=True)
    mgr.create_index("convnextv2_sra", metric_type="COSINE")
    col.insert([[f"/d/{i}.png" for i in range(6)], ["normal"] * 6, e.cpu()])
    col.load()
    hits = col.search(e.cpu(), limit=1)
    assert [h[0].id for h in hits] == list(range(6))
