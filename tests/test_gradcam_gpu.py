"""MedSigLIP Grad-CAM on the GPU: k_gradcam.hip against the float64 restatement (_gradcam_ref) on the same fp32 tokens at the
MedSigLIP geometry and at odd sizes, bits across batches and chunks, NaN containment, argument checks, the tower left
bit-identical, the reduced model end to end against the reference's fixture, the 448 x 448 tower against float64 autograd,
no library GEMM / softmax / LayerNorm / upsample / autograd in a native call, and the torch path where the gate says so."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _gradcam_ref as R
from mirx import _lib, xai
from mirx import siglip_gradcam as G
from mirx.model import MedSigLIP, _layernorm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gradcam_ref.npz")
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _tiny(gold, case=None, dtype=torch.float32):
    m = R.build_model({k[2:]: v for k, v in gold.items() if k.startswith("w/")}, dtype=dtype)
    if case == "flat":
        with torch.no_grad():
            m.projection[3].weight.zero_()
    return m.to(DEV).eval()


def _geometry(d, heads, inter, n, seed):
    """A one-layer MedSigLIP of width d (its tower is not run: the tests hand the kernels tokens) with perturbed weights."""
    side = int(round(n ** 0.5))
    torch.manual_seed(seed)
    m = MedSigLIP(vision_config=dict(hidden_size=d, intermediate_size=inter, num_hidden_layers=1, num_attention_heads=heads,
                                     image_size=side * 2, patch_size=2), embed_dim=64)
    m.backbone.embeddings.num_positions = n
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g))
    return m.to(DEV).eval()


def _tokens(b, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((b, n, d), generator=g) * (1.0 + torch.rand((b, n, 1), generator=g))).to(DEV)


def _qemb(m, bq, seed):
    e = m.projection[3].out_features
    return torch.nn.functional.normalize(torch.randn((bq, e), generator=torch.Generator().manual_seed(seed)), dim=1).to(DEV)


def _expected(m, x, q, size):
    W = {k: v.detach().double().cpu().numpy() for k, v in m.state_dict().items()}
    return R.expected(W, x.double().cpu().numpy(), q.double().cpu().numpy(), m.backbone.head.attention.num_heads, size)


GEOMETRIES = [(1152, 16, 4304, 1024, 448), (64, 4, 64, 25, 35), (128, 4, 96, 257, 40), (256, 4, 128, 257, 33)]


@pytest.mark.parametrize("d,heads,inter,n,size", GEOMETRIES)
def test_pool_kernel_matches_float64(d, heads, inter, n, size):
    """ybar = sum_n P y_n: each entry within gamma_k (2 A + 1) max|y| (k = d + n + 16, A = max_n sum_d |y_n u_h|: the score
    error moves P by at most 2 gamma_k A relative), DESIGN 21."""
    x = _tokens(2, n, d, 3)
    gamma = (1.0 + 0.2 * torch.randn(d, generator=torch.Generator().manual_seed(4))).to(DEV)
    beta = (0.2 * torch.randn(d, generator=torch.Generator().manual_seed(5))).to(DEV)
    u = (torch.randn((heads, d), generator=torch.Generator().manual_seed(6)) / d ** 0.5).to(DEV)
    c = torch.randn(heads, generator=torch.Generator().manual_seed(7)).to(DEV)
    ws = torch.empty((G.workspace_floats(2, n, d, heads),), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        ybar = G.gradcam_pool(x, gamma, beta, 1e-6, u, c, ws).double().cpu().numpy()
    xd, gd, bd, ud, cd = (t.double().cpu().numpy() for t in (x, gamma, beta, u, c))
    for i in range(2):
        y, _, _ = R._ln(xd[i], gd, bd, 1e-6)
        S = y @ ud.T + cd
        P = np.exp(S - S.max(0))
        P /= P.sum(0)
        ref = P.T @ y
        A = (np.abs(y) @ np.abs(ud).T).max()
        bound = (d + n + 16) * EPS32 * (2 * A + 1) * np.abs(y).max()
        assert float(np.abs(ybar[i] - ref).max()) <= bound


@pytest.mark.parametrize("d,heads,inter,n,size", [g for g in GEOMETRIES if int(g[3] ** 0.5) ** 2 == g[3]])
def test_kernels_match_float64_maps(d, heads, inter, n, size):
    m = _geometry(d, heads, inter, n, 10)
    x = _tokens(2, n, d, 11)
    q = _qemb(m, 2, 12)
    with torch.no_grad():
        got = G.gradcam_from_tokens(m, q, x, (size, size)).cpu().numpy()
    ref = _expected(m, x, q, (size, size))
    assert float(np.abs(got - ref).max()) <= 1e-3


def test_bits_across_batches_and_chunks():
    m = _geometry(1152, 16, 4304, 1024, 20)
    x = _tokens(5, 1024, 1152, 21)
    q = _qemb(m, 1, 22)
    with torch.no_grad():
        all5 = G.gradcam_from_tokens(m, q, x, (448, 448))
        one = G.gradcam_from_tokens(m, q, x[2:3].contiguous(), (448, 448))
        parts = torch.cat([G.gradcam_from_tokens(m, q, x[:2].contiguous(), (448, 448)),
                           G.gradcam_from_tokens(m, q, x[2:].contiguous(), (448, 448))])
    assert torch.equal(all5[2], one[0]) and torch.equal(all5, parts)
    assert float(all5.max()) == 1.0


def test_nan_containment(gold):
    m = _tiny(gold)
    x = _tokens(3, R.N, 64, 30)
    q = _qemb(m, 1, 31)
    with torch.no_grad():
        clean = G.gradcam_from_tokens(m, q, x, R.SIZE)
        x[1, 7, 5] = float("nan")
        dirty = G.gradcam_from_tokens(m, q, x, R.SIZE)
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[2], clean[2])
    assert torch.count_nonzero(dirty[1]) == 0


def test_bad_arguments_fail_before_launch():
    x = torch.zeros((1, 24, 64), device=DEV)
    ws = torch.zeros((G.workspace_floats(1, 24, 64, 4),), device=DEV)
    with pytest.raises(_lib.MirxError):
        G.gradcam_finish(x, 4, ws, (35, 35))                          # 24 tokens: not a square grid
    with pytest.raises(_lib.MirxError):
        G.gradcam_finish(torch.zeros((1, 25, 64), device=DEV), 4, ws, (35, 35))     # workspace of 24 tokens
    with pytest.raises(_lib.MirxError):
        G.gradcam_pool(torch.zeros((1, 25, 64), device=DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV), 1e-6,
                       torch.zeros((17, 64), device=DEV), torch.zeros(17, device=DEV), ws)       # 17 heads
    torch.cuda.synchronize()


def test_tower_stays_bit_identical(gold):
    m = _tiny(gold)
    bb = m.backbone
    img = torch.from_numpy(gold["k3_retrieved"]).to(DEV)
    with torch.no_grad():
        before = bb(pixel_values=img)
        emb = m(img)
        last = bb._last_layer_tokens(img)
        xai.compute_gradcam_saliency(m, img[:1], img, DEV)
        after = bb(pixel_values=img)
        emb_after = m(img)
        assert torch.equal(_layernorm(bb.post_layernorm, last), before.last_hidden_state)
    assert xai.compute_gradcam_saliency.last_native
    assert torch.equal(before.last_hidden_state, after.last_hidden_state)
    assert torch.equal(before.pooler_output, after.pooler_output) and torch.equal(emb, emb_after)


@pytest.mark.parametrize("case", R.CASES)
def test_reduced_model_matches_the_fixture(gold, case):
    m = _tiny(gold, case)
    q = torch.from_numpy(gold[f"{case}_query"]).to(DEV)
    r = torch.from_numpy(gold[f"{case}_retrieved"]).to(DEV)
    if case == "bq2":
        with torch.no_grad():
            qemb = m(q)
        got = np.stack([xai._compute_single_gradcam(m, qemb, r[i:i + 1], DEV) for i in range(r.shape[0])])
        assert xai._compute_single_gradcam.last_native
    else:
        got = xai.compute_gradcam_saliency(m, q, r, DEV)
        assert xai.compute_gradcam_saliency.last_native
    ref = gold[f"{case}_out"]
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert float(np.abs(got - ref).max()) <= 1e-3
    if case == "flat":
        assert np.all(got == 0)
    if case == "nan":
        assert np.all(got[R.NAN_IMAGE] == 0)
    assert all(p.grad is None for p in m.parameters())


@pytest.fixture(scope="module")
def medsiglip():
    torch.manual_seed(40)
    m = MedSigLIP()
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
    return m.to(DEV).eval()


def test_full_geometry_matches_float64_autograd(medsiglip):
    img = torch.randn((3, 3, 448, 448), generator=torch.Generator().manual_seed(42)).to(DEV)
    got = xai.compute_gradcam_saliency(medsiglip, img[:1], img[1:], DEV)
    assert xai.compute_gradcam_saliency.last_native
    m64 = MedSigLIP()
    m64.load_state_dict(medsiglip.state_dict())
    m64 = m64.to(DEV).double().eval()
    with torch.no_grad():
        q64 = m64(img[:1].double())
    ref = np.stack([G._single_torch(m64, q64, img[i:i + 1].double()) for i in (1, 2)])
    del m64
    assert float(np.abs(got - ref).max()) <= 1e-3


def test_native_call_runs_no_library_ops(medsiglip):
    img = torch.randn((2, 3, 448, 448), generator=torch.Generator().manual_seed(43)).to(DEV)
    xai.compute_gradcam_saliency(medsiglip, img[:1], img[1:], DEV)                   # caches built outside the profile
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        xai.compute_gradcam_saliency(medsiglip, img[:1], img[1:], DEV)
    assert xai.compute_gradcam_saliency.last_native
    names = {e.key for e in prof.key_averages()}
    banned = {"aten::mm", "aten::bmm", "aten::matmul", "aten::addmm", "aten::linear", "aten::softmax", "aten::_softmax",
              "aten::layer_norm", "aten::native_layer_norm", "aten::upsample_bilinear2d"}
    assert not (names & banned), names & banned
    assert not [n for n in names if "Backward" in n or "autograd::engine" in n]


def test_torch_path_where_the_gate_says_so(gold):
    m = _tiny(gold)
    q = torch.from_numpy(gold["k3_query"]).to(DEV)
    r = torch.from_numpy(gold["k3_retrieved"]).to(DEV)
    native = xai.compute_gradcam_saliency(m, q, r, DEV)
    assert xai.compute_gradcam_saliency.last_native

    class Wrap(nn.Module):                       # not a mirx MedSigLIP: same modules, the torch path
        def __init__(self, inner):
            super().__init__()
            self.backbone, self.projection, self.inner = inner.backbone, inner.projection, inner

        def forward(self, x):
            return self.inner(x)

    other = xai.compute_gradcam_saliency(Wrap(m), q, r, DEV)
    assert not xai.compute_gradcam_saliency.last_native
    assert float(np.abs(other - native).max()) <= 1e-3
    m64 = _tiny(gold, dtype=torch.float64)
    d64 = xai.compute_gradcam_saliency(m64, q.double(), r.double(), DEV)
    assert not xai.compute_gradcam_saliency.last_native
    assert float(np.abs(d64 - gold["k3_out"]).max()) <= 1e-6          # float64 on the GPU: other libm rounding
    cpu = xai.compute_gradcam_saliency(_tiny(gold).cpu(), q.cpu(), r.cpu(), torch.device("cpu"))
    assert not xai.compute_gradcam_saliency.last_native
    assert float(np.abs(cpu - native).max()) <= 1e-3
