"""SimCAM on the MI355X: mirx_simcam (k_simcam.hip) against the float64 restatement in _simcam_ref over the geometries the
reference's backbones produce, bit-identical batches, NaN containment, argument checks, and the four saliency configurations of
the reference's drivers end to end on mirx models (native path, maps against the reference's formulas on the eager feature map,
no library GEMM / convolution / upsample / amax inside the call)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _simcam_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORBIDDEN = ("aten::mm", "aten::bmm", "aten::matmul", "aten::addmm", "aten::upsample_bilinear2d", "aten::amax")


def _rows(gen, n, hw, c, sign=None):
    x = torch.randn(n, hw, c, generator=gen)
    if sign == "pos":
        x = x.abs()
    elif sign == "neg":
        x = -x.abs()
    return x


def _close(got, exp, tol):
    """Per map (the last two axes): NaN where expected, else within tol of the map's max |value|."""
    got = np.asarray(got, np.float64)
    exp = np.asarray(exp, np.float64)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    g2, e2 = got.reshape(-1, *got.shape[-2:]), exp.reshape(-1, *exp.shape[-2:])
    for g, e in zip(g2, e2):
        assert np.array_equal(np.isnan(g), np.isnan(e))
        if np.isnan(e).all():
            continue
        scale = float(np.abs(e).max())
        err = float(np.abs(g - e).max())
        assert err <= tol * max(scale, 1e-30), (err, scale)


def _kernel(q, r, h, w, size, eps, maps, point=None):
    from mirx.simcam import simcam_maps
    return simcam_maps(q.to(DEV), r.to(DEV), h, w, size, eps=eps, maps=maps, point=point)


# (h, w, C, P): every hw and C of the issue, P in {1, 5, 64}, kept to what a float64 restatement checks in seconds
GEOMS = [(1, 1, 1, 1), (1, 1, 64, 5), (5, 7, 3, 5), (5, 7, 1152, 64), (7, 7, 2048, 5), (7, 7, 1024, 64), (7, 7, 1, 1),
         (12, 12, 1024, 5), (12, 12, 64, 64), (32, 32, 1152, 1), (32, 32, 3, 5), (32, 32, 2048, 1)]
MODES = [("both", 1e-8, None), ("both", 0.0, None), ("retrieved", 1e-8, None), ("both", 1e-8, "c"), ("both", 0.0, "br")]


@pytest.mark.parametrize("h,w,c,p", GEOMS, ids=[f"{h}x{w}_c{c}_p{p}" for h, w, c, p in GEOMS])
@pytest.mark.parametrize("maps,eps,pt", MODES, ids=["both", "both_eps0", "retrieved", "point_c", "point_br_eps0"])
def test_kernel_matches_the_restatement(h, w, c, p, maps, eps, pt):
    gen = torch.Generator().manual_seed(h * 1000 + c * 7 + p)
    size = (3 * h + 1, 2 * w + 3)
    point = None if pt is None else R._pt(pt, *size)
    q, r = _rows(gen, 1, h * w, c)[0], _rows(gen, p, h * w, c)
    got = _kernel(q, r, h, w, size, eps, maps, point).cpu().numpy()
    exp = R.simcam(q.double().numpy(), r.double().numpy(), h, w, size[0], size[1], eps, point)
    _close(got, exp if maps == "both" else exp[:, 1], 1e-5)


@pytest.mark.parametrize("h,w,c", [(7, 7, 2048), (5, 7, 3), (32, 32, 1152)])
@pytest.mark.parametrize("pt", [None, "tl"])
def test_kernel_every_d_negative(h, w, c, pt):
    """q >= 0, r <= 0: s = max(D) + eps < 0, relu(D / s) keeps the negative part."""
    gen = torch.Generator().manual_seed(5)
    size = (2 * h, 2 * w)
    point = None if pt is None else R._pt(pt, *size)
    q, r = _rows(gen, 1, h * w, c, "pos")[0], _rows(gen, 3, h * w, c, "neg")
    got = _kernel(q, r, h, w, size, 1e-8, "both", point).cpu().numpy()
    exp = R.simcam(q.double().numpy(), r.double().numpy(), h, w, size[0], size[1], 1e-8, point)
    assert np.nanmax(exp) > 0
    _close(got, exp, 1e-5)


def test_zero_maps_give_nan_without_eps():
    q = torch.zeros(49, 1024)
    r = torch.zeros(2, 49, 1024)
    out = _kernel(q, r, 7, 7, (224, 224), 0.0, "both").cpu()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("maps,pt", [("both", None), ("retrieved", None), ("both", (100, 37))])
def test_pair_bits_do_not_depend_on_the_batch(maps, pt):
    gen = torch.Generator().manual_seed(11)
    q, r = _rows(gen, 1, 144, 1024)[0], _rows(gen, 64, 144, 1024)
    full = _kernel(q, r, 12, 12, (384, 384), 1e-8, maps, pt).cpu()
    for p in (0, 17, 63):
        alone = _kernel(q, r[p:p + 1], 12, 12, (384, 384), 1e-8, maps, pt).cpu()
        assert torch.equal(alone[0], full[p])
    part = _kernel(q, r[20:45], 12, 12, (384, 384), 1e-8, maps, pt).cpu()
    assert torch.equal(part, full[20:45])


def test_nan_stays_in_its_pair():
    gen = torch.Generator().manual_seed(12)
    q, r = _rows(gen, 1, 49, 2048)[0], _rows(gen, 8, 49, 2048)
    r[3, 20, 100] = float("nan")
    for maps, pt in (("both", None), ("retrieved", None), ("both", (3, 200))):
        out = _kernel(q, r, 7, 7, (224, 224), 1e-8, maps, pt).cpu()
        assert torch.isnan(out[3]).all()
        assert torch.isfinite(torch.cat([out[:3], out[4:]])).all()


def test_argument_checks_fire_before_any_launch():
    import ctypes
    from mirx import _lib
    from mirx.model import _ptr, _stream
    from mirx.simcam import simcam_maps
    lib = _lib.load()
    q = torch.randn(49, 64, device=DEV)
    r = torch.randn(2, 49, 64, device=DEV)
    out = torch.full((2, 2, 8, 8), 7.0, device=DEV)
    ws = torch.empty(lib.mirx_simcam_workspace_floats(2, 49), device=DEV)
    st = _stream(DEV)
    bad = [dict(h=33, w=33), dict(h=0), dict(c=0), dict(c=20000), dict(H=0), dict(W=9000), dict(maps=2), dict(eps=-1.0),
           dict(eps=float("nan")), dict(stride=49 * 63), dict(point=(8.0, 0.0)), dict(point=(0.0, -1.0)), dict(ws=10),
           dict(pairs=70000)]
    for b in bad:
        pt = b.get("point")
        args = dict(h=7, w=7, c=64, H=8, W=8, maps=0, eps=1e-8, stride=49 * 64, ws=ws.numel(), pairs=2)
        args.update({k: v for k, v in b.items() if k != "point"})
        cpt = None if pt is None else (ctypes.c_double * 2)(*pt)
        rc = lib.mirx_simcam(_ptr(q), _ptr(r), args["pairs"], args["stride"], args["h"], args["w"], args["c"], args["eps"],
                             args["maps"], cpt, args["H"], args["W"], _ptr(ws), args["ws"], _ptr(out), st)
        assert rc != 0, b
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert lib.mirx_simcam_workspace_floats(1, 1025) < 0 and lib.mirx_simcam_workspace_floats(-1, 49) < 0
    with pytest.raises(_lib.MirxError):
        simcam_maps(torch.randn(1089, 8, device=DEV), torch.randn(1, 1089, 8, device=DEV), 33, 33, (64, 64))
    with pytest.raises(ValueError):
        simcam_maps(q, r[:, :48], 7, 7, (8, 8))
    with pytest.raises(ValueError):
        simcam_maps(q.double(), r.double(), 7, 7, (8, 8))
    from mirx.simcam import SimCAM
    from mirx.model import ResNet50
    m = ResNet50().to(DEV).eval()
    with pytest.raises(ValueError):
        SimCAM(m, m.resnet50[7][2])(torch.randn(1, 3, 224, 224, device=DEV), torch.randn(1, 3, 224, 224, device=DEV),
                                    point=(224, 0))


# ---- the four configurations end to end -------------------------------------------------------------------------------
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


def _expected_from_fmap(fmap, size, eps, cls, fc=None):
    """The reference's formulas in float64 on an eager feature map [B, C, h, w] (a CPU tensor)."""
    rows = R.rows_of(fmap.double().numpy())
    h, w = fmap.shape[-2:]
    if fc is not None:
        rows = R.token_fc(rows, fc.weight.detach().cpu().double().numpy(), fc.bias.detach().cpu().double().numpy(), h * w)
    if cls == "dense":
        return R.simcam(rows[0], rows[1:2], h, w, size, size, 0.0)[0]
    return R.simcam(rows[0], rows[1:], h, w, size, size, eps)


@pytest.mark.parametrize("emb", [None, 64])
@pytest.mark.parametrize("nr", [1, 5])
def test_densenet121_end_to_end(emb, nr):
    from oracle import densenet as OD
    from mirx.model import DenseNet121
    from mirx.simcam import SimCAM_Densenet121
    torch.manual_seed(0)
    model = DenseNet121(embedding_dim=emb).eval()
    model.load_state_dict(OD.randomize_bn_stats(model.state_dict(), seed=3), strict=True)
    cpu = DenseNet121(embedding_dim=emb).eval()
    cpu.load_state_dict(model.state_dict())
    model = model.to(DEV)
    seq = nn.Sequential(*list(model.children())[0], *list(model.children())[1:])      # the reference driver's Sequential
    ex = SimCAM_Densenet121(seq, seq[0], target_layers=["relu"], fc=seq[2] if emb else None).to(DEV).eval()
    xq, x = _images(1, 224, 1), _images(nr, 224, 2)
    out = _no_library_ops(lambda: ex(xq.to(DEV), x.to(DEV)))
    assert ex.last_native and out.shape == (2, 224, 224)
    with torch.no_grad():
        fmap = cpu.densenet121[0](torch.cat([xq, x])[:2])
    _close(out.cpu().numpy(), _expected_from_fmap(fmap, 224, 0.0, "dense", cpu.fc), 1e-4)


@pytest.mark.parametrize("nr", [1, 5])
def test_resnet50_end_to_end(nr):
    from mirx.model import ResNet50
    from mirx.simcam import SimCAM
    torch.manual_seed(1)
    cpu = ResNet50().eval()
    model = ResNet50().eval()
    model.load_state_dict(cpu.state_dict())
    model = model.to(DEV)
    ex = SimCAM(model=model, target_layer=model.resnet50[7][2], fc=None)
    xq, x = _images(1, 224, 3), _images(nr, 224, 4)
    out = _no_library_ops(lambda: ex(xq.to(DEV), x.to(DEV)))
    assert ex.last_native and out.shape == (nr, 2, 224, 224)
    with torch.no_grad():
        fmap = cpu.resnet50[:8](torch.cat([xq, x]))
    _close(out.cpu().numpy(), _expected_from_fmap(fmap, 224, 1e-8, "cam"), 1e-4)
    outp = ex(xq.to(DEV), x.to(DEV), point=(0, 223))
    assert ex.last_native
    rows = R.rows_of(fmap.numpy())
    _close(outp.cpu().numpy(), R.simcam(rows[0], rows[1:], 7, 7, 224, 224, 1e-8, (0, 223)), 1e-4)


@pytest.mark.parametrize("nr", [1, 5])
def test_convnextv2_end_to_end(nr):
    from mirx.model import ConvNeXtV2
    from mirx.simcam import SimCAM
    torch.manual_seed(2)
    cpu = ConvNeXtV2().eval()
    model = ConvNeXtV2().eval()
    model.load_state_dict(cpu.state_dict())
    model = model.to(DEV)
    backbone = model.convnext
    ex = SimCAM(model=backbone, target_layer=backbone.stages[3].blocks[2], fc=None)
    xq, x = _images(1, 384, 5), _images(nr, 384, 6)
    out = _no_library_ops(lambda: ex(xq.to(DEV), x.to(DEV)))
    assert ex.last_native and out.shape == (nr, 2, 384, 384)
    with torch.no_grad():
        fmap = cpu.convnext.stages(cpu.convnext.stem(torch.cat([xq, x])))
    assert fmap.shape[-2:] == (12, 12)
    _close(out.cpu().numpy(), _expected_from_fmap(fmap, 384, 1e-8, "cam"), 1e-4)


V_SMALL = dict(hidden_size=144, intermediate_size=208, num_hidden_layers=2, num_attention_heads=2, image_size=448, patch_size=14)


@pytest.mark.parametrize("nr", [1, 5])
def test_medsiglip_reduced_end_to_end(nr):
    from mirx.model import MedSigLIP
    from mirx.simcam import SimCAM_MedSigLIP
    torch.manual_seed(3)
    cpu = MedSigLIP(vision_config=V_SMALL).eval()
    with torch.no_grad():
        for name, p in cpu.named_parameters():
            if name.endswith("bias"):
                p.add_(0.02 * torch.randn_like(p))
    model = MedSigLIP(vision_config=V_SMALL).eval()
    model.load_state_dict(cpu.state_dict())
    model = model.to(DEV)
    ex = SimCAM_MedSigLIP(model, model.backbone.post_layernorm)
    xq, x = _images(1, 448, 7), _images(nr, 448, 8)
    out = _no_library_ops(lambda: ex(xq.to(DEV), x.to(DEV)))
    assert ex.last_native and out.shape == (nr, 448, 448)
    with torch.no_grad():
        tok = cpu.backbone(pixel_values=torch.cat([xq, x])).last_hidden_state.double().numpy()
    assert tok.shape[1] == 1024
    _close(out.cpu().numpy(), R.simcam(tok[0], tok[1:], 32, 32, 448, 448, 1e-8)[:, 1], 1e-4)


def test_medsiglip_full_geometry_against_the_torch_formulas():
    from mirx.model import MedSigLIP
    from mirx.simcam import SimCAM_MedSigLIP
    torch.manual_seed(4)
    model = MedSigLIP().eval().to(DEV)
    ex = SimCAM_MedSigLIP(model, model.backbone.post_layernorm)
    xq, x = _images(1, 448, 9).to(DEV), _images(5, 448, 10).to(DEV)
    out = _no_library_ops(lambda: ex(xq, x))
    assert ex.last_native and out.shape == (5, 448, 448)
    with torch.no_grad():
        tok = model.backbone.last_hidden_state(torch.cat([xq, x])).double()
        sim = torch.matmul(tok[0:1].expand(5, -1, -1), tok[1:].transpose(1, 2))
        sim = (sim / (sim.amax(dim=(1, 2), keepdim=True) + 1e-8)).clamp(min=0).view(5, 32, 32, 32, 32).sum(dim=(1, 2))
        exp = torch.nn.functional.interpolate(sim.unsqueeze(1), size=(448, 448), mode="bilinear", align_corners=False)[:, 0]
    _close(out.cpu().numpy(), exp.cpu().numpy(), 1e-5)


def test_reference_sizes_take_the_native_path():
    """ConvNeXtV2_SRA's backbone (compute_saliency_convnextv2.py) and a DenseNet at 256 x 256 (the legacy feature path)."""
    from mirx.model import ConvNeXtV2_SRA, DenseNet121
    from mirx.simcam import SimCAM, SimCAM_Densenet121
    torch.manual_seed(5)
    sra = ConvNeXtV2_SRA().eval()
    cpu_sra = ConvNeXtV2_SRA().eval()
    cpu_sra.load_state_dict(sra.state_dict())
    sra = sra.to(DEV)
    ex = SimCAM(model=sra.convnext, target_layer=sra.convnext.stages[3].blocks[2])
    xq, x = _images(1, 384, 11), _images(1, 384, 12)
    out = _no_library_ops(lambda: ex(xq.to(DEV), x.to(DEV)))
    assert ex.last_native
    with torch.no_grad():
        fmap = cpu_sra.convnext.stages(cpu_sra.convnext.stem(torch.cat([xq, x])))
    _close(out.cpu().numpy(), _expected_from_fmap(fmap, 384, 1e-8, "cam"), 1e-4)

    dn = DenseNet121().eval()
    cpu = DenseNet121().eval()
    cpu.load_state_dict(dn.state_dict())
    dn = dn.to(DEV)
    seq = nn.Sequential(*list(dn.children())[0], *list(dn.children())[1:])
    exd = SimCAM_Densenet121(seq, seq[0], target_layers=["relu"]).to(DEV).eval()
    xq, x = _images(1, 256, 13), _images(1, 256, 14)
    out = exd(xq.to(DEV), x.to(DEV), point=(128, 40))
    assert exd.last_native and out.shape == (2, 256, 256)
    with torch.no_grad():
        fmap = cpu.densenet121[0](torch.cat([xq, x]))
    rows = R.rows_of(fmap.numpy())
    _close(out.cpu().numpy(), R.simcam(rows[0], rows[1:2], 8, 8, 256, 256, 0.0, (128, 40))[0], 1e-4)


def test_training_mode_takes_the_torch_path():
    from mirx.model import ResNet50
    from mirx.simcam import SimCAM
    model = ResNet50().to(DEV).train()
    ex = SimCAM(model, model.resnet50[7][2])
    ex(_images(1, 64, 1).to(DEV), _images(1, 64, 2).to(DEV))
    assert not ex.last_native


def test_resnet50_token_fc_and_copies_stay_native():
    """A per-position fc over the map's channels runs natively; a deep-copied DenseNet121's stack resolves to the copy."""
    import copy
    from mirx.model import DenseNet121, ResNet50
    from mirx.simcam import SimCAM, SimCAM_Densenet121
    torch.manual_seed(6)
    cpu = ResNet50().eval()
    model = ResNet50().eval()
    model.load_state_dict(cpu.state_dict())
    model = model.to(DEV)
    fc = nn.Linear(2048, 64).to(DEV)
    ex = SimCAM(model, model.resnet50[7][2], fc=fc)
    xq, x = _images(1, 224, 15), _images(2, 224, 16)
    out = ex(xq.to(DEV), x.to(DEV))
    assert ex.last_native
    with torch.no_grad():
        fmap = cpu.resnet50[:8](torch.cat([xq, x]))
    _close(out.cpu().numpy(), _expected_from_fmap(fmap, 224, 1e-8, "cam", fc), 1e-4)
    bad = nn.Linear(1000, 64).to(DEV)                       # another width: the hook path, which the native model never feeds
    with pytest.raises(RuntimeError, match="hook failed"):
        SimCAM(model, model.resnet50[7][2], fc=bad)(xq.to(DEV), x.to(DEV))

    dn = copy.deepcopy(DenseNet121().eval()).to(DEV)
    seq = nn.Sequential(*list(dn.children())[0], *list(dn.children())[1:])
    exd = SimCAM_Densenet121(seq, seq[0], target_layers=["relu"]).to(DEV).eval()
    exd(_images(1, 224, 17).to(DEV), _images(1, 224, 18).to(DEV))
    assert exd.last_native


def test_pairs_chunked_by_workspace_give_the_same_bits(monkeypatch):
    import mirx.simcam as S
    from mirx import _lib
    gen = torch.Generator().manual_seed(13)
    q, r = _rows(gen, 1, 1024, 64)[0], _rows(gen, 20, 1024, 64)
    whole = _kernel(q, r, 32, 32, (64, 64), 1e-8, "both", (10, 50)).cpu()
    monkeypatch.setattr(S, "WORKSPACE_FLOATS", 7 * _lib.load().mirx_simcam_workspace_floats(1, 1024))   # 3 calls: 7, 7, 6
    chunked = _kernel(q, r, 32, 32, (64, 64), 1e-8, "both", (10, 50)).cpu()
    assert torch.equal(whole, chunked)
