"""SwinV2 on the MI355X: the shifted-window cosine attention kernel (mirx_window_attention_split2h) on every configuration the
model uses, its mask semantics, the res-post-norm and patch-merge glue, and the model end to end against float64."""
import math

import pytest
import torch
import torch.nn.functional as F

from _swinv2_ref import embed, randomize, region_ids, window_attention

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _lib():
    from mirx import _lib as L
    return L


def _ptr(t):
    from mirx.model import _ptr as p
    return p(t)


def _st():
    from mirx.model import _stream
    return _stream(torch.device(DEV))


def _decode_terms(t, scale):
    """terms rows [m, 2 c] fp16 -> float64 [m, c] (high + low) / scale"""
    m = t.shape[0]
    v = t.cpu().view(m, -1, 2, 32).double()
    return ((v[:, :, 0] + v[:, :, 1]) / scale).reshape(m, -1)


def _run_attention(qkv, side, ws, shift, heads, table, ls, out_scale=2.0 ** 10):
    n = qkv.shape[0]
    c = qkv.shape[-1] // 3
    q = qkv.reshape(-1, 3 * c).float().contiguous().to(DEV)
    out = torch.empty((q.shape[0], c), dtype=torch.float32, device=DEV)
    terms = torch.empty((q.shape[0], 2 * c), dtype=torch.float16, device=DEV)
    tg, lg = table.float().contiguous().to(DEV), ls.float().contiguous().to(DEV)      # held until the kernel has run
    L = _lib()
    L.check(L.load().mirx_window_attention_split2h(_ptr(q), n, side, ws, shift, heads, 32, _ptr(tg), _ptr(lg), _ptr(out), _ptr(terms),
                                                   out_scale, _st()))
    torch.cuda.synchronize()
    return out.cpu().double().view(n, side, side, c), _decode_terms(terms, out_scale).view(n, side, side, c)


# (side, heads, window, shift): every attention the model runs at 384 x 384
CONFIGS = [(96, 4, 24, 0), (96, 4, 24, 12), (48, 8, 24, 0), (48, 8, 24, 12), (24, 16, 24, 0), (12, 32, 12, 0)]


@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("side,heads,ws,shift", CONFIGS)
def test_window_attention_matches_float64(side, heads, ws, shift, n, clamped):
    g = torch.Generator().manual_seed(side * 100 + heads + shift + n + 7 * clamped)
    c = 32 * heads
    qkv = torch.randn(n, side, side, 3 * c, generator=g)
    qkv[..., 2 * c:] *= 3.0
    table = 16 * torch.rand(heads, (2 * ws - 1) ** 2, generator=g)
    # ls = exp(min(logit_scale, ln 100)): random in [1, 100), or exactly at the clamp
    ls = torch.full((heads,), 100.0) if clamped else torch.exp(math.log(100.0) * torch.rand(heads, generator=g))
    ref = window_attention(qkv.double(), heads, side, ws, shift, table.double(), ls.double())
    out, terms = _run_attention(qkv, side, ws, shift, heads, table, ls)
    # the logits carry ~2^-22 relative error of q^ . k^ times ls <= 100: weights good to ~3e-5 relative
    tol = 1e-4 * float(qkv[..., 2 * c:].abs().max())
    assert float((out - ref).abs().max()) <= tol
    assert float((terms - ref).abs().max()) <= tol
    assert float((terms - out).abs().max()) <= 1e-6 * float(out.abs().max())


def test_window_attention_mask_is_minus_100():
    """Shifted 48 x 48 map, window 24, shift 12, zero bias table, scale 100.  Query vectors point at the OTHER region of their
    window, keys at their own: same-region pairs have cosine 0, cross-region pairs +1, so 0 + 0 and 100 - 100 weigh alike and
    the output is a mixture of the two V values (an unmasked kernel gives the cross-region V, a -inf kernel the same-region V)."""
    side, ws, s, heads = 48, 24, 12, 8
    c = 32 * heads
    reg = torch.roll(region_ids(side, ws, s).view(side, side), shifts=(s, s), dims=(0, 1))   # region of every (unshifted) pixel
    partner = {0: 0, 1: 2, 2: 1, 3: 6, 6: 3, 4: 5, 5: 4, 7: 8, 8: 7}
    first = {0: 0, 1: 1, 2: 1, 3: 3, 6: 3, 4: 4, 5: 4, 7: 7, 8: 7}      # V = -1 on the window's first region pair member
    qkv = torch.zeros(1, side, side, 3 * c)
    for y in range(side):
        for x in range(side):
            r = int(reg[y, x])
            for h in range(heads):
                qkv[0, y, x, h * 32 + partner[r]] = 1.0
                qkv[0, y, x, c + h * 32 + r] = 1.0
                qkv[0, y, x, 2 * c + h * 32: 2 * c + h * 32 + 32] = -1.0 if first[r] == r else 1.0
    table = torch.zeros(heads, (2 * ws - 1) ** 2)
    ls = torch.full((heads,), 100.0)
    ref = window_attention(qkv.double(), heads, side, ws, s, table.double(), ls.double())
    out, terms = _run_attention(qkv, side, ws, s, heads, table, ls)
    assert float((out - ref).abs().max()) <= 1e-5
    assert float((terms - ref).abs().max()) <= 1e-5
    # window (0, 1) of the shifted map: regions 1 (12 columns, V = -1) and 2 (12 columns, V = +1), equal weights -> 0
    px = (0 + s) % side, (24 + s) % side                               # its token (0, 0) at the unshifted pixel
    assert abs(float(ref[0, px[0], px[1], 0])) <= 1e-9
    assert abs(float(out[0, px[0], px[1], 0])) <= 1e-5


@pytest.mark.parametrize("c", [128, 256, 512, 1024])
@pytest.mark.parametrize("with_x", [False, True])
def test_postnorm_matches_float64(c, with_x):
    g = torch.Generator().manual_seed(c + with_x)
    m = 1000
    y = 3 * torch.randn(m, c, generator=g) + 1.0
    x = torch.randn(m, c, generator=g)
    gamma, beta = 0.5 + torch.rand(c, generator=g), 0.1 * torch.randn(c, generator=g)
    ref = F.layer_norm(y.double(), (c,), gamma.double(), beta.double(), 1e-5) + (x.double() if with_x else 0)
    xg, yg = x.to(DEV), y.to(DEV)
    out = xg if with_x else torch.empty_like(yg)
    t = torch.empty((m, 2 * c), dtype=torch.float16, device=DEV)
    gg, bg = gamma.to(DEV), beta.to(DEV)
    L = _lib()
    L.check(L.load().mirx_swin_postnorm(_ptr(xg) if with_x else None, _ptr(yg), m, c, _ptr(gg), _ptr(bg), 1e-5, _ptr(out), _ptr(t),
                                        1024.0, _st()))
    torch.cuda.synchronize()
    assert float((out.cpu().double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    assert float((_decode_terms(t, 1024.0) - out.cpu().double()).abs().max()) <= 1e-6 * float(ref.abs().max())


@pytest.mark.parametrize("n,side,c", [(2, 96, 128), (3, 48, 256), (1, 24, 512)])
def test_patch_merge_matches_float64(n, side, c):
    x = torch.randn(n, side, side, c, generator=torch.Generator().manual_seed(side))
    ref = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).double().reshape(-1, 4 * c)
    xg = x.to(DEV).contiguous()
    t = torch.empty((ref.shape[0], 8 * c), dtype=torch.float16, device=DEV)
    L = _lib()
    L.check(L.load().mirx_patch_merge_terms(_ptr(xg), n, side, side, c, 4096.0, _ptr(t), _st()))
    torch.cuda.synchronize()
    assert float((_decode_terms(t, 4096.0) - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def _model(emb=None, seed=0):
    from mirx.model import SwinV2
    torch.manual_seed(seed)
    return randomize(SwinV2(embedding_dim=emb), seed=seed + 1).eval().to(DEV)


def _images(n, seed=1, size=384):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


def _eager_fp32(m, x):
    with torch.no_grad():
        f = m.forward_eager(x)
        if m.fc is not None:
            f = m.fc(f)
        return F.normalize(f, dim=1)


@pytest.mark.parametrize("emb", [None, 512])
def test_end_to_end_matches_float64(emb):
    m = _model(emb)
    x = _images(2)
    with torch.no_grad():
        y = m(x.to(DEV))
    eager = _eager_fp32(m, x.to(DEV))
    ref = embed(x, m.state_dict())
    err_native = float((y.cpu().double() - ref).abs().max())
    err_eager = float((eager.cpu().double() - ref).abs().max())
    print(f"swinv2 emb={emb}: native {err_native:.3e}, eager fp32 {err_eager:.3e}")
    assert y.shape == (2, emb or 1024)
    assert err_native <= max(1e-5, 2 * err_eager)


def test_batch_independence():
    m = _model(None, seed=3)
    x = _images(16, seed=4).to(DEV)
    with torch.no_grad():
        full = m(x)
        pairs = torch.cat([m(x[i:i + 2]) for i in range(0, 16, 2)])
    assert float((full - pairs).abs().max()) <= 1e-6


def test_native_path_runs_no_library_ops():
    m = _model(512, seed=5)
    x = _images(2, seed=6).to(DEV)
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad():
        m(x)                          # the weight cache (bias tables from cpb_mlp, bounds) is built once per weight version
    with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
        m(x)
    names = {e.name for e in prof.events()}
    banned = ("matmul", "bmm", "mm", "addmm", "linear", "softmax", "_softmax", "roll", "layer_norm", "native_layer_norm", "conv")
    bad = [nm for nm in names if nm.startswith("aten::") and any(nm[6:] == b or nm[6:].startswith(b + "_") or nm[6:] == "_" + b
                                                                 for b in banned)]
    assert not bad, bad
    assert not any("convolution" in nm for nm in names)
    with pytest.raises(ValueError):
        with torch.no_grad():
            m(_images(1, size=352).to(DEV))


def test_containment_of_non_finite_images():
    m = _model(None, seed=7)
    x = _images(3, seed=8)
    bad = x.clone()
    bad[1] = float("nan")
    with torch.no_grad():
        clean = m(x.to(DEV))
        dirty = m(bad.to(DEV))
    assert torch.equal(clean[[0, 2]], dirty[[0, 2]])
    assert not torch.isfinite(dirty[1]).all()


def test_cache_follows_new_weights():
    m = _model(None, seed=9)
    x = _images(2, seed=10)
    with torch.no_grad():
        first = m(x.to(DEV))
        m.load_state_dict(_model(None, seed=11).state_dict())
        second = m(x.to(DEV))
        assert not torch.equal(first, second)
        assert float((second.cpu().double() - embed(x, m.state_dict())).abs().max()) <= 1e-4
        m.swinv2.layers[2].blocks[3].attn.logit_scale.add_(1.0)        # in-place edits
        m.swinv2.layers[1].blocks[0].norm2.weight.mul_(3.0)
        third = m(x.to(DEV))
        assert not torch.equal(second, third)
        assert float((third.cpu().double() - embed(x, m.state_dict())).abs().max()) <= 1e-4


def test_retrieval_round_trip():
    from mirx.index import FlatIndex
    from mirx.retriever import get_model_and_transform
    model, _ = get_model_and_transform("swinv2", None, 128, "cuda")
    randomize(model, seed=12)
    x = _images(6, seed=13).to(DEV)
    with torch.no_grad():
        e = model(x)
    assert e.shape == (6, 128)
    ix = FlatIndex(128, "COSINE", 0)
    ix.add(e, torch.arange(6))
    _, ids = ix.search(e, 1)
    assert ids[:, 0].cpu().tolist() == list(range(6))
