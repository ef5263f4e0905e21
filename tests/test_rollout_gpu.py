"""Attention rollout on the MI355X: the k_rollout.hip kernels against the float64 restatement in _rollout_ref (the layer
kernel with a near-tie audit of its kept sets, the row stage's kept sets exactly, the chain and finish), bit-identical batches
and chunks, NaN containment, argument checks, and AttentionRolloutMedSigLIP end to end on mirx MedSigLIP models (native path,
maps against the reference's formulas on the tower's torch attentions in float64, no library GEMM / kthvalue / softmax /
upsample inside the call)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rollout_ref as R
from _rollout_ref import _audited_expected, _fused64, _score_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
FORBIDDEN = ("aten::mm", "aten::bmm", "aten::matmul", "aten::addmm", "aten::linear", "aten::kthvalue", "aten::softmax",
             "aten::_softmax", "aten::upsample_bilinear2d")
V_SMALL = dict(hidden_size=144, intermediate_size=208, num_hidden_layers=2, num_attention_heads=2, image_size=448, patch_size=14)


def _qkv(gen, b, n, heads, dh):
    return torch.randn(b, n, 3 * heads * dh, generator=gen)


LAYER_GEOMS = [(16, 72, 2, 3), (49, 64, 16, 1), (257, 72, 16, 3), (257, 64, 2, 1), (1024, 72, 16, 1), (1024, 64, 2, 3)]


@pytest.mark.parametrize("n,dh,heads,b", LAYER_GEOMS, ids=[f"n{n}_d{d}_h{h}_b{b}" for n, d, h, b in LAYER_GEOMS])
@pytest.mark.parametrize("fusion", ["mean", "max", "min"])
@pytest.mark.parametrize("ratio", [0.0, 0.9])
def test_layer_kernel_matches_the_restatement(n, dh, heads, b, fusion, ratio):
    from mirx.rollout import rollout_layer, workspace_floats
    gen = torch.Generator().manual_seed(n * 7 + dh + heads)
    qkv = _qkv(gen, b, n, heads, dh)
    scale = dh ** -0.5
    k = max(1, int(n * ratio)) if ratio > 0 else 0
    ws = torch.full((workspace_floats(2, b, n),), float("nan"), device=DEV)
    rollout_layer(qkv.to(DEV), heads, scale, fusion, k, 1, 2, ws)
    got = ws[b * n * n:2 * b * n * n].view(b, n, n)
    assert not torch.isnan(got).any()
    eb = _score_bound(qkv, heads, dh, scale)
    tol = 2 * eb * (1 + 2 * eb) + (n + heads + 4) * U             # the fused value's relative error bound
    exp, _ = _audited_expected(_fused64(qkv, heads, dh, scale, fusion), got, k, tol)
    err = ((got.double() - exp).abs() / (exp + 1e-30)).max().item()
    assert err <= tol + 2 * (n + 4) * U, (err, tol)


ROW_CASES = [(16, 1), (16, 16), (100, 50), (100, 1), (1000, 900), (1024, 921), (1024, 1024), (63, 31), (1024, 1)]


@pytest.mark.parametrize("n,k", ROW_CASES, ids=[f"n{n}_k{k}" for n, k in ROW_CASES])
def test_row_stage_kept_set_is_exact(n, k):
    from mirx.rollout import rollout_rows_
    rng = np.random.default_rng(n + k)
    rows = 12
    a = (rng.integers(1, 40, size=(rows, n)) / 64.0).astype(np.float32)          # many ties everywhere
    a[1] = 0.25                                                                    # all equal: only the identity is left
    a[2, ::3] = 0.0                                                                # exact zeros
    a[3] = rng.random(n).astype(np.float32) + 0.5                                  # no ties
    thr_val = np.partition(a[4], k - 1)[k - 1]
    a[4, rng.permutation(n)[:3]] = thr_val                                         # ties planted at the threshold
    got = rollout_rows_(torch.from_numpy(a).to(DEV), k).cpu().numpy()
    thr = np.partition(a, k - 1, axis=1)[:, k - 1:k]
    keep = a > thr
    idx = np.arange(rows)
    off = np.ones_like(keep)
    off[idx, idx % n] = False
    assert np.array_equal((got != 0) & off, keep & (a != 0) & off)
    exp = R.row_stage(a, k)
    assert np.abs(got - exp).max() <= (n + 8) * U * np.abs(exp).max()
    assert np.allclose(got[1][idx[1] % n], 1.0 / (1.0 + 1e-8)) and np.count_nonzero(got[1]) == 1
    rollout_rows_(torch.from_numpy(a).to(DEV), 0)                                  # k = 0 is accepted (no discard)


@pytest.mark.parametrize("n,h,w,b,e", [(1024, 32, 32, 2, 512), (49, 7, 7, 3, 64), (16, 4, 4, 1, 6)])
@pytest.mark.parametrize("guided", [True, False])
def test_chain_and_finish_match_float64(n, h, w, b, e, guided):
    from mirx.rollout import rollout_finish, workspace_floats
    gen = torch.Generator().manual_seed(n + b)
    L = 5
    mats = torch.rand(L, b, n, n, generator=gen) * (torch.rand(L, b, n, n, generator=gen) > 0.8)
    mats = mats + torch.eye(n)
    mats = mats / mats.sum(-1, keepdim=True)
    ws = torch.zeros((workspace_floats(L, b, n),), device=DEV)
    ws[:L * b * n * n] = mats.reshape(-1).to(DEV)
    patches = F.normalize(torch.randn(b, n, e, generator=gen), dim=-1)
    query = F.normalize(torch.randn(e, generator=gen), dim=0)
    size = (3 * h + 2, 2 * w + 5)
    if guided:
        out = rollout_finish(ws, L, b, h, w, size, patches.to(DEV), query.to(DEV))
    else:
        out = rollout_finish(ws, L, b, h, w, size)
    v = R.importance(list(mats.double().numpy()))
    bound = (L * (n + 4) + 16) * U                                  # f32 sums of non-negative terms: the chain's bound
    if guided:
        sim = np.maximum((patches.double().numpy() * query.double().numpy()).sum(-1), 0)
        v = v * sim
        bound += (e + 2) * U / sim.max()                            # the dot of unit vectors: |error| <= e u
    exp = R.resize_bilinear(v.reshape(b, h, w), *size)
    err = np.abs(out.cpu().numpy() - exp).max() / np.abs(exp).max()
    assert err <= bound, (err, bound)


def _rollout_inputs(b, n=257, heads=4, dh=72, L=3, e=32, seed=0):
    gen = torch.Generator().manual_seed(seed)
    qkvs = [_qkv(gen, b, n, heads, dh).to(DEV) for _ in range(L)]
    patches = F.normalize(torch.randn(b, n, e, generator=gen), dim=-1).to(DEV)
    query = F.normalize(torch.randn(e, generator=gen), dim=0).to(DEV)
    return qkvs, patches, query


def test_one_image_equals_the_same_image_among_five_and_chunks():
    from mirx.rollout import rollout_maps, workspace_floats
    qkvs, patches, query = _rollout_inputs(5, n=256)
    args = (4, 72 ** -0.5, "mean", 230, 16, 16, (40, 56))
    five = rollout_maps(qkvs, *args, patches=patches, query=query)
    for i in (0, 3):
        one = rollout_maps([q[i:i + 1].contiguous() for q in qkvs], *args, patches=patches[i:i + 1].contiguous(), query=query)
        assert torch.equal(one[0], five[i])
    per = workspace_floats(3, 1, 256)
    for budget in (per, 2 * per + 5):                               # chunks of 1 and 2 images
        assert torch.equal(rollout_maps(qkvs, *args, patches=patches, query=query, budget=budget), five)
    for fusion in ("max", "min"):
        a = rollout_maps(qkvs, 4, 72 ** -0.5, fusion, 0, 16, 16, (40, 56))
        c = rollout_maps(qkvs, 4, 72 ** -0.5, fusion, 0, 16, 16, (40, 56), budget=per)
        assert torch.equal(a, c)


def test_nan_stays_in_its_image():
    from mirx.rollout import rollout_maps
    qkvs, patches, query = _rollout_inputs(3, n=256, seed=1)
    args = (4, 72 ** -0.5, "max", 128, 16, 16, (32, 32))
    clean = rollout_maps(qkvs, *args, patches=patches, query=query)
    bad = [q.clone() for q in qkvs]
    bad[1][1, 17, 5] = float("nan")
    out = rollout_maps(bad, *args, patches=patches, query=query)
    assert torch.isnan(out[1]).all()
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])


def test_bad_arguments_fail_before_any_launch():
    from mirx import _lib
    from mirx.rollout import rollout_finish, rollout_layer, rollout_rows_, workspace_floats
    ws = torch.zeros((workspace_floats(2, 1, 64),), device=DEV)
    sentinel = ws.clone()
    q = torch.zeros(1, 64, 3 * 2 * 72, device=DEV)
    for kw in (dict(k=65), dict(layer=2), dict(fusion="sum")):
        a = dict(k=1, layer=0, fusion="mean")
        a.update(kw)
        with pytest.raises((_lib.MirxError, KeyError)):
            rollout_layer(q, 2, 0.1, a["fusion"], a["k"], a["layer"], 2, ws)
    with pytest.raises(_lib.MirxError):
        rollout_layer(torch.zeros(1, 64, 3 * 2 * 74, device=DEV), 2, 0.1, "mean", 1, 0, 2, ws)       # head_dim 74
    with pytest.raises(_lib.MirxError):
        rollout_layer(torch.zeros(1, 1025, 3 * 2 * 72, device=DEV), 2, 0.1, "mean", 1, 0, 2, ws)     # n > 1024
    with pytest.raises(_lib.MirxError):
        rollout_layer(q, 2, 0.1, "mean", 1, 0, 2, ws[:-1])                                          # workspace too small
    with pytest.raises(ValueError):
        rollout_layer(q.cpu(), 2, 0.1, "mean", 1, 0, 2, ws)
    with pytest.raises(ValueError):
        rollout_layer(q, 2, 0.1, "mean", 1, 0, 2, ws.cpu())                                        # a host workspace
    with pytest.raises(ValueError):
        rollout_layer(q, 2, 0.1, "mean", 1, 0, 2, ws.double())
    with pytest.raises(ValueError):
        rollout_layer(q, 2, 0.1, "mean", 1, 0, 2, ws.view(2, -1)[:, :ws.numel() // 4])            # not contiguous
    with pytest.raises(ValueError):
        rollout_layer(torch.zeros(1, 64, 3 * 2 * 72 + 3, device=DEV), 2, 0.1, "mean", 1, 0, 2, ws)  # 3c not 3 * heads * dh
    with pytest.raises(ValueError):
        rollout_finish(ws.cpu(), 2, 1, 8, 8, (8, 8))
    with pytest.raises(ValueError):
        rollout_finish(ws, 2, 1, 8, 8, (8, 8), out=torch.zeros(1, 8, 8))                         # out on the host
    with pytest.raises(_lib.MirxError):
        rollout_rows_(torch.zeros(4, 8, device=DEV), 9)
    with pytest.raises(_lib.MirxError):
        rollout_finish(ws, 2, 1, 8, 8, (0, 8))
    with pytest.raises(ValueError):
        rollout_finish(ws, 2, 1, 8, 8, (8, 8), torch.zeros(1, 64, 4, device=DEV), torch.zeros(5, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(ws, sentinel)


# ---- end to end -------------------------------------------------------------------------------------------------------
def _no_library_ops(fn):
    """fn() under torch.profiler, after one unprofiled call (which builds the models' derived weights once)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    bad = sorted(n for n in names if n in FORBIDDEN or "conv" in n.split("::")[-1] and n.startswith("aten::"))
    assert not bad, bad
    return out


def _images(n, size, seed):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


def _reference_on_torch_attentions(model, native_mats, xq, x, fusion, ratio, guided, tie_tol):
    """The reference's formulas in float64 on the tower's torch attentions (backbone(output_attentions=True)), the kept-set
    decisions of near-ties taken from the native per-layer matrices -> ([B, H, W] float64, flips)."""
    bb = model.backbone
    B, _, H, W = x.shape
    with torch.no_grad():
        outs = bb(pixel_values=x, output_attentions=True)
        n = outs.attentions[0].shape[-1]
        k = max(1, int(n * ratio)) if ratio > 0 else 0
        v = torch.full((B, n), 1.0 / n, dtype=torch.float64, device=DEV)
        mats, flips = [], 0
        for layer, att in enumerate(outs.attentions):
            F64 = AttentionFuse[fusion](att.double())
            a, f = _audited_expected(F64, native_mats[layer], k, tie_tol)
            mats.append(a)
            flips += f
        for a in reversed(mats):
            v = torch.einsum("bi,bij->bj", v, a)
        if guided:
            p = F.normalize(outs.last_hidden_state.double(), dim=-1)
            q = model(xq).double()[0]
            if p.shape[-1] != q.shape[0]:
                p = F.normalize(copy.deepcopy(model.projection).double()(p), dim=-1)
            v = v * (p * q).sum(-1).clamp(min=0)
        side = int(n ** 0.5)
        return F.interpolate(v.view(B, 1, side, side), size=(H, W), mode="bilinear", align_corners=False)[:, 0], flips


AttentionFuse = {"mean": lambda a: a.mean(1), "max": lambda a: a.amax(1), "min": lambda a: a.amin(1)}


def _small_model(seed=3):
    from mirx.model import MedSigLIP
    torch.manual_seed(seed)
    m = MedSigLIP(vision_config=V_SMALL).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("bias"):
                p.add_(0.02 * torch.randn_like(p))
    return m.to(DEV)


def _rel(got, exp):
    return float((got.double() - exp).abs().max() / exp.abs().max())


CFGS = [("mean", 0.9, True), ("max", 0.5, False), ("min", 0.0, True), ("mean", 0.0, False)]


@pytest.mark.parametrize("fusion,ratio,guided", CFGS, ids=[f"{f}_r{int(r * 10)}_{'qg' if g else 'plain'}" for f, r, g in CFGS])
@pytest.mark.parametrize("nr", [1, 3])
def test_medsiglip_reduced_end_to_end(fusion, ratio, guided, nr):
    from mirx.xai import AttentionRolloutMedSigLIP
    model = _small_model()
    ex = AttentionRolloutMedSigLIP(model, head_fusion=fusion, discard_ratio=ratio, query_guided=guided)
    ex._keep_layers = True
    xq, x = _images(1, 448, 7).to(DEV), _images(nr, 448, 8).to(DEV)
    out = _no_library_ops(lambda: ex(xq, x))
    assert ex.last_native and out.shape == (nr, 448, 448) and ex.last_layers.shape == (2, nr, 1024, 1024)
    exp, flips = _reference_on_torch_attentions(model, ex.last_layers, xq, x, fusion, ratio, guided, 1e-3)
    err = _rel(out, exp)
    print(f"reduced {fusion} r{ratio} qg={guided} nr={nr}: rel err {err:.2e}, audited flips {flips}")
    assert err <= 1e-4, err


@pytest.mark.parametrize("fusion,ratio,guided", [("mean", 0.9, True), ("max", 0.9, False)])
def test_medsiglip_full_geometry_end_to_end(fusion, ratio, guided):
    from mirx.model import MedSigLIP
    from mirx.xai import AttentionRolloutMedSigLIP
    torch.manual_seed(4)
    model = MedSigLIP().eval().to(DEV)
    ex = AttentionRolloutMedSigLIP(model, head_fusion=fusion, discard_ratio=ratio, query_guided=guided)
    ex._keep_layers = True
    xq, x = _images(1, 448, 9).to(DEV), _images(2, 448, 10).to(DEV)
    out = _no_library_ops(lambda: ex(xq, x))
    assert ex.last_native and out.shape == (2, 448, 448)
    mats = ex.last_layers
    exp, flips = _reference_on_torch_attentions(model, mats, xq, x, fusion, ratio, guided, 1e-3)
    err = _rel(out, exp)
    print(f"full {fusion} r{ratio} qg={guided}: rel err {err:.2e}, audited flips {flips}")
    assert err <= 1e-3, err


def test_tap_leaves_the_tower_bit_identical():
    from mirx.rollout import rollout_layer, workspace_floats
    model = _small_model(5)
    bb = model.backbone
    x = _images(3, 448, 11).to(DEV)
    with torch.no_grad():
        tok0, emb0, pooled0 = bb.last_hidden_state(x), model(x), bb(pixel_values=x).pooler_output
        ws = torch.empty((workspace_floats(2, 3, 1024),), device=DEV)
        at = bb.encoder.layers[0].self_attn
        tok1 = bb._hidden_tapped(x, lambda i, qkv: rollout_layer(qkv, at.num_heads, at.scale, "mean", 921, i, 2, ws))
        tok2, emb2, pooled2 = bb.last_hidden_state(x), model(x), bb(pixel_values=x).pooler_output
    assert torch.equal(tok0, tok1) and torch.equal(tok0, tok2)
    assert torch.equal(emb0, emb2) and torch.equal(pooled0, pooled2)


def test_other_inputs_take_the_torch_path():
    from mirx.xai import AttentionRolloutMedSigLIP
    model = _small_model(6)
    xq, x = _images(1, 448, 12).to(DEV), _images(1, 448, 13).to(DEV)
    ex = AttentionRolloutMedSigLIP(model)
    native = ex(xq, x)
    assert ex.last_native
    model.train()
    torch_out = ex(xq, x)
    assert not ex.last_native and ex.last_layers is None
    model.eval()
    assert torch_out.shape == native.shape and torch.isfinite(torch_out).all()
    cpu = copy.deepcopy(model).cpu()
    ex_cpu = AttentionRolloutMedSigLIP(cpu)
    ex_cpu(xq.cpu(), x.cpu())
    assert not ex_cpu.last_native
    ex_bad = AttentionRolloutMedSigLIP(model, discard_ratio=1.5)
    with pytest.raises(RuntimeError):
        ex_bad(xq, x)
    assert not ex_bad.last_native
