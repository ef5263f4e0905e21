"""SimAtt on the MI355X: mirx_simatt (k_simatt.hip) on given rows against the float64 restatement of the closed form
(_simatt_ref), bit-identical maps whatever the batch, NaN containment, the limits, and compute_saliency.py's recipe end to end on
a mirx DenseNet121 against the same explainer on its torch path (both within 1e-4 of each map's maximum, the bound the SimCAM
end-to-end tests set for maps from the native feature path against the eager one, whatever the conditioning of wt).

Tolerance of the kernel comparisons (every error is max|got - f64| / max|f64| per map): per case e_ref is the largest such error
of the reference's own formulas in torch float32 on the same rows (_simatt_ref.ref32, autograd included); the kernel is allowed
4 * e_ref plus one float32 ulp of the map's maximum.  Each case prints `SIMATT_ACC <case> e_ref=.. native=.. bound=..` before it
asserts (profiles/r13_simatt_accuracy.txt is that output).  Cases with an fc keep every embedding component at least 1e-3 of the
largest away from zero (_simatt_ref.make_rows), where float32 and float64 cannot disagree on a sign.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _simatt_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _kernel(rows, fw, fb, size, mode, h, w, positive):
    from mirx.simatt import simatt_maps
    t = lambda a: None if a is None else torch.as_tensor(a).to(DEV)   # noqa: E731
    return simatt_maps(t(rows), t(fw), t(fb), size, mode, h, w, positive=positive).cpu().numpy()


def _check(tag, rows, fw, fb, h, w, mode, positive, size=None):
    size = size or ((3 * h + 2, 2 * w + 5) if h * w < 100 else (32 * h, 32 * w))
    got = _kernel(rows, fw, fb, size, mode, h, w, positive)
    exp = R.simatt(rows, h, w, size[0], size[1], fw, fb, mode, positive)
    e_ref = max(R.map_errors(R.ref32(rows, h, w, size[0], size[1], fw, fb, mode, positive), exp))
    errs = R.map_errors(got, exp)
    bound = 4 * e_ref + R.ULP32
    print(f"SIMATT_ACC {tag} mode={mode} positive={int(positive)} maps={len(errs)} max|f64|={np.abs(exp).max():.3e} "
          f"e_ref={e_ref:.3e} native={max(errs):.3e} bound={bound:.3e}")
    assert np.abs(exp).max() > 0, "a fixture whose every map is zero shows nothing"
    assert max(errs) <= bound, (max(errs), e_ref)


# (h, w, C, D): DenseNet's 7 x 7 x 1024 with every fc width of the issue, the 12 x 12 map of a 384 input, odd shapes
GEOMS = [(7, 7, 1024, None), (7, 7, 1024, 64), (7, 7, 1024, 256), (7, 7, 1024, 1024), (12, 12, 1024, None), (12, 12, 1024, 64),
         (1, 1, 64, None), (3, 5, 100, 7), (5, 7, 1000, None), (2, 3, 70, 33)]
GIDS = [f"{h}x{w}_c{c}_d{d}" for h, w, c, d in GEOMS]


@pytest.mark.parametrize("h,w,c,d", GEOMS, ids=GIDS)
@pytest.mark.parametrize("b", [2, 3, 9])
@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
def test_group_mode_matches_the_restatement(h, w, c, d, b, positive):
    rows, fw, fb = R.make_rows(1000 * h + 10 * b + (d or 0), b, h * w, c, d)
    _check(f"group_{h}x{w}_c{c}_d{d}_b{b}", rows, fw, fb, h, w, "group", positive)


@pytest.mark.parametrize("h,w,c,d", GEOMS, ids=GIDS)
@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
def test_pairs_mode_matches_the_restatement(h, w, c, d, k, positive):
    size = (96, 120) if k == 64 and h * w > 49 else None    # 128 maps of 12 x 12: a smaller output keeps the float64 side short
    rows, fw, fb = R.make_rows(2000 * h + 10 * k + (d or 0), 1 + k, h * w, c, d)
    _check(f"pairs_{h}x{w}_c{c}_d{d}_k{k}", rows, fw, fb, h, w, "pairs", positive, size)


@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
def test_one_component_embedding(positive):
    """D = 1: xn = +-1.  Two images on opposite sides of zero (|xn_0 - xn_1| = 2), so that no factor is an exact zero."""
    rows, _, _ = R.make_rows(5, 2, 15, 70, None)
    fw = np.linspace(-1.0, 1.0, 70, dtype=np.float32)[None]
    fb = np.array([-float(R.embedding(rows, fw, None).mean())], np.float32)
    x = R.embedding(rows, fw, fb)
    assert x[0, 0] * x[1, 0] < 0 and R.sign_margin_ok(rows, fw, fb)
    _check("group_3x5_c70_d1_b2", rows, fw, fb, 3, 5, "group", positive)
    _check("pairs_3x5_c70_d1_k1", rows, fw, fb, 3, 5, "pairs", positive)


@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
def test_group_of_257_images(positive):
    """256 factors: the rows are chosen (make_rows spread) so that each factor is about 1 and the product stays in float32's
    range; image 1 is on the query's side, so the flipped first factor 1 - |.| does not cancel."""
    rows, fw, fb = R.make_rows(31, 257, 15, 4, None, spread=True)
    _check("group_3x5_c4_b257", rows, fw, fb, 3, 5, "group", positive)


def test_pairs_of_256_retrievals():
    rows, fw, fb = R.make_rows(32, 257, 49, 64, 16)
    _check("pairs_7x7_c64_d16_k256", rows, fw, fb, 7, 7, "pairs", True)


def test_dead_channel_has_sign_zero():
    rows, _, _ = R.make_rows(33, 3, 49, 1024, None)
    rows[:, :, 5] = 0.0
    _check("group_7x7_c1024_dead_channel", rows, None, None, 7, 7, "group", True)
    _check("pairs_7x7_c1024_dead_channel", rows, None, None, 7, 7, "pairs", False)


@pytest.mark.parametrize("d", [None, 256])
@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
def test_pair_bits_do_not_depend_on_the_batch(d, positive):
    rows, fw, fb = R.make_rows(41, 257, 49, 1024, d)
    full = _kernel(rows, fw, fb, (224, 224), "pairs", 7, 7, positive)            # K = 256, B = 257
    k64 = _kernel(rows[:65], fw, fb, (224, 224), "pairs", 7, 7, positive)
    assert np.array_equal(k64, full[:64])
    for k in (0, 17, 63, 255):
        alone = _kernel(rows[[0, k + 1]], fw, fb, (224, 224), "pairs", 7, 7, positive)   # K = 1, B = 2
        assert np.array_equal(alone[0], full[k])
        group = _kernel(rows[[0, k + 1]], fw, fb, (224, 224), "group", 7, 7, positive)   # the same two images as a group
        assert np.array_equal(group, full[k])
    part = _kernel(rows[[0] + list(range(21, 46))], fw, fb, (224, 224), "pairs", 7, 7, positive)
    assert np.array_equal(part, full[20:45])


def test_group_call_is_deterministic_and_writes_into_out():
    from mirx.simatt import simatt_maps
    rows, fw, fb = R.make_rows(42, 9, 49, 1024, 64)
    r, a, b = (torch.as_tensor(t).to(DEV) for t in (rows, fw, fb))
    out = torch.empty(9, 224, 224, device=DEV)
    assert simatt_maps(r, a, b, (224, 224), "group", 7, 7, positive=True, out=out) is out
    again = simatt_maps(r, a, b, (224, 224), "group", 7, 7, positive=True)
    assert torch.equal(out, again) and bool(torch.isfinite(out).all()) and float(out.max()) > 0


@pytest.mark.parametrize("d", [None, 64])
def test_nan_containment(d):
    rows, fw, fb = R.make_rows(43, 9, 49, 1024, d)
    rows[4, 20, 100] = np.nan                                                     # retrieval k = 3
    for positive in (True, False):
        out = _kernel(rows, fw, fb, (64, 64), "pairs", 7, 7, positive)
        assert np.isnan(out[3]).all() and np.isfinite(np.delete(out, 3, axis=0)).all()
        exp = R.simatt(rows, 7, 7, 64, 64, fw, fb, "pairs", positive)
        assert np.array_equal(np.isnan(out), np.isnan(exp))
        grp = _kernel(rows, fw, fb, (64, 64), "group", 7, 7, positive)
        assert np.isnan(grp).all()                                                # as torch: every wt has image 4 as a factor
        ref = R.ref32(rows, 7, 7, 64, 64, fw, fb, "group", positive)
        assert np.isnan(ref).all()
    rows, fw, fb = R.make_rows(44, 4, 49, 1024, d)
    rows[0, 0, 0] = np.nan                                                        # the query: every pair
    assert np.isnan(_kernel(rows, fw, fb, (64, 64), "pairs", 7, 7, True)).all()


def test_limits_fail_before_any_launch():
    from mirx import _lib
    from mirx.model import _ptr, _stream
    from mirx.simatt import simatt_maps
    lib = _lib.load()
    rows = torch.randn(3, 49, 64, device=DEV)
    fw = torch.randn(8, 64, device=DEV)
    out = torch.full((3, 8, 8), 7.0, device=DEV)
    ws = torch.empty(lib.mirx_simatt_workspace_floats(3, 64, 8, 1), device=DEV)
    st = _stream(DEV)
    base = dict(b=3, h=7, w=7, c=64, d=8, mode=0, positive=0, H=8, W=8, ws=ws.numel(), fc=True)
    bad = [dict(h=33, w=32), dict(h=0), dict(c=0), dict(c=16385), dict(d=16385), dict(d=0), dict(fc=False), dict(b=1),
           dict(b=65536), dict(H=0), dict(W=8193), dict(mode=2), dict(positive=2), dict(ws=10)]
    for kw in bad:
        a = dict(base, **kw)
        rc = lib.mirx_simatt(_ptr(rows), a["b"], a["h"], a["w"], a["c"], _ptr(fw) if a["fc"] else None, None, a["d"], a["mode"],
                             a["positive"], a["H"], a["W"], _ptr(ws), a["ws"], _ptr(out), st)
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for args in ((torch.randn(2, 1089, 8, device=DEV), None, None, (64, 64), "group", 33, 33),
                 (torch.randn(1, 49, 8, device=DEV), None, None, (64, 64), "group", 7, 7),
                 (rows, None, None, (8193, 8), "group", 7, 7),
                 (rows, fw[:, :32], None, (8, 8), "group", 7, 7),
                 (rows, fw.double(), None, (8, 8), "group", 7, 7),
                 (rows, None, torch.zeros(8, device=DEV), (8, 8), "group", 7, 7),
                 (rows.double(), None, None, (8, 8), "group", 7, 7)):
        with pytest.raises(ValueError):
            simatt_maps(*args)
    with pytest.raises(ValueError):
        simatt_maps(rows, None, None, (8, 8), "group", 7, 7, out=torch.empty(3, 8, 9, device=DEV))


# ---- compute_saliency.py's recipe end to end -----------------------------------------------------------------------------
FEATURE_TOL = 1e-4             # maps from the native feature path against the eager one: the bound of the SimCAM end-to-end tests


def _images(n, size, seed):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


def _flat(emb):
    from oracle import densenet as OD
    from mirx.model import DenseNet121
    torch.manual_seed(0)
    model = DenseNet121(embedding_dim=emb).eval()
    model.load_state_dict(OD.randomize_bn_stats(model.state_dict(), seed=3), strict=True)
    model = model.to(DEV)
    seq = nn.Sequential(*list(model.children())[0], *list(model.children())[1:]).to(DEV).eval()   # compute_saliency.py:190
    seq.__dict__["_keep"] = model       # the feature stack knows its DenseNet121 through a weak reference: keep the model alive
    return seq


def _condition(seq, x, positive_first):
    """From the EAGER embedding of x: whether the sign margin holds, and (printed only) the worst-case amplification of an error
    of xn in wt, 1 / mean|factor| over the factors |xn_0 - xn_j| (or 1 - that)."""
    with torch.no_grad():
        e = torch.flatten(seq[1](seq[0](x)), 1)
        e = (seq[2](e) if len(seq) == 3 else e).double().cpu().numpy()
    ok = bool((np.abs(e).min(axis=1) >= R.SIGN_MARGIN * np.abs(e).max(axis=1)).all()) if len(seq) == 3 else True
    xn = e / np.linalg.norm(e, axis=1, keepdims=True)
    f = np.abs(xn[0] - xn[1:])
    if positive_first:
        f[0] = 1 - f[0]
    return ok, float((1.0 / f.mean(axis=1)).max())


@pytest.mark.parametrize("emb", [None, 64])
@pytest.mark.parametrize("size", [224, 256])
@pytest.mark.parametrize("form", ["ap", "an", "triplet"])
def test_densenet121_end_to_end(monkeypatch, emb, size, form):
    import mirx.simatt as S
    seq = _flat(emb)
    ex = S.SimAtt(seq, seq[0], target_layers=["relu"]).to(DEV).eval()
    for seed in range(100, 164):                            # with an fc: a seed whose eager embedding keeps the sign margin
        xq, xo = _images(1, size, seed).to(DEV), _images(2, size, seed + 1000).to(DEV)
        xp = xo[:1] if form in ("ap", "triplet") else None
        xn = xo[1:] if form in ("an", "triplet") else None
        ok, cond = _condition(seq, torch.cat([t for t in (xq, xp, xn) if t is not None]), xp is not None)
        if ok:
            break
    else:
        raise AssertionError("no seed keeps the sign margin")
    out = ex(xq, xp, xn)
    assert ex.last_native is True and out.shape == ((3 if form == "triplet" else 2), size, size) and not out.requires_grad
    with torch.no_grad():
        again = ex(xq, xp, xn)                              # no graph is needed
    assert ex.last_native is True and again.shape == out.shape
    with monkeypatch.context() as mp:
        mp.setattr(S, "_native_plan", lambda *a, **k: None)
        ref = ex(xq, xp, xn)                                # the reference's formulas: eager modules, autograd
        assert ex.last_native is False
    errs = R.map_errors(out.cpu().numpy(), ref.double().cpu().numpy())
    errs += R.map_errors(again.cpu().numpy(), ref.double().cpu().numpy())   # (the 256 x 256 feature path is not bit-stable per call)
    print(f"SIMATT_E2E emb={emb} size={size} form={form} seed={seed} cond={cond:.3e} max|ref|={float(ref.abs().max()):.3e} "
          f"err={max(errs):.3e} bound={FEATURE_TOL:.3e}")
    assert float(ref.abs().max()) > 0
    assert max(errs) <= FEATURE_TOL, (errs, cond)


@pytest.mark.parametrize("emb", [None, 64])
@pytest.mark.parametrize("positive", [True, False], ids=["pos", "neg"])
def test_simatt_pairs_equals_the_per_pair_calls(emb, positive):
    import mirx.simatt as S
    seq = _flat(emb)
    ex = S.SimAtt(seq, seq[0], target_layers=["relu"]).to(DEV).eval()
    xq, xr = _images(1, 224, 7).to(DEV), _images(5, 224, 8).to(DEV)
    out = S.simatt_pairs(ex, xq, xr, positive=positive)
    assert ex.last_native is True and out.shape == (5, 2, 224, 224)
    for k in range(5):
        one = ex(xq, xr[k:k + 1]) if positive else ex(xq, None, xr[k:k + 1])
        assert ex.last_native is True and torch.equal(one, out[k])
    assert torch.equal(S.simatt_pairs(seq, xq, xr, positive=positive), out)


@pytest.mark.parametrize("emb", [None, 64])
def test_driver_lines_as_written_go_native(emb):
    """compute_saliency.py:189-192 verbatim: `model` is rebound to the Sequential, which drops the DenseNet121 itself."""
    import gc
    from mirx.model import DenseNet121
    from mirx.xai import SimAtt
    torch.manual_seed(0)
    model = DenseNet121(embedding_dim=emb).to(DEV)
    model.eval()
    model = nn.Sequential(*list(model.children())
                          [0], *list(model.children())[1:])
    explainer = SimAtt(model, model[0], target_layers=["relu"])
    explainer = explainer.to(DEV)
    explainer.eval()
    gc.collect()
    assert model[0].__dict__["_mirx_owner"]() is None       # the wrapper is gone
    xq, xp, xn = _images(1, 224, 1).to(DEV), _images(1, 224, 2).to(DEV), _images(1, 224, 3).to(DEV)
    out = explainer(xq, xp, xn)
    assert explainer.last_native is True and out.shape == (3, 224, 224)
    owner = model[0].__dict__["_mirx_owner"]()
    assert owner is not None and owner.densenet121[0] is model[0]
    out2 = explainer(xq, xp, xn)
    assert explainer.last_native is True and model[0].__dict__["_mirx_owner"]() is owner and torch.equal(out, out2)
    kept = DenseNet121(embedding_dim=emb).to(DEV).eval()    # the same weights on a model that stays alive: the same bits
    kept.load_state_dict({**{"densenet121.0." + k: v for k, v in model[0].state_dict().items()},
                          **({"fc." + k: v for k, v in model[2].state_dict().items()} if emb else {})})
    seq = nn.Sequential(*list(kept.children())[0], *list(kept.children())[1:]).eval()
    assert torch.equal(SimAtt(seq, seq[0], ["relu"])(xq, xp, xn), out)


@pytest.mark.parametrize("emb", [None, 64])
def test_simatt_pairs_over_several_embed_chunks(emb):
    """K = 70: 71 images, two _relu_rows chunks.  At 224 x 224 an image's rows do not depend on its batch, so a pair among 70
    equals the pair alone bit for bit."""
    import mirx.simatt as S
    seq = _flat(emb)
    ex = S.SimAtt(seq, seq[0], target_layers=["relu"]).to(DEV).eval()
    xq, xr = _images(1, 224, 21).to(DEV), _images(70, 224, 22).to(DEV)
    assert 1 + xr.shape[0] > S.EMBED_CHUNK
    out = S.simatt_pairs(ex, xq, xr)
    assert ex.last_native is True and out.shape == (70, 2, 224, 224)
    for k in (0, 62, 63, 64, 69):
        assert torch.equal(ex(xq, xr[k:k + 1]), out[k]), k


def test_other_forms_take_the_torch_path():
    import mirx.simatt as S
    from mirx.model import DenseNet121
    model = DenseNet121(embedding_dim=16, num_labels=3).to(DEV).eval()
    seq = nn.Sequential(*list(model.children())[0], *list(model.children())[1:]).eval()      # ..., fc, classification head
    ex = S.SimAtt(seq, seq[0], ["relu"])
    xq, xp = _images(1, 64, 1).to(DEV), _images(1, 64, 2).to(DEV)
    assert ex(xq, xp).shape == (2, 64, 64) and ex.last_native is False
    seq2 = _flat(None)
    ex2 = S.SimAtt(seq2, seq2[0], ["relu"])
    assert ex2(xq).shape == (1, 64, 64) and ex2.last_native is False                          # a single image: no factor
    assert ex2(xq[:, :1].expand(-1, 3, -1, -1).contiguous(), xp).shape == (2, 64, 64) and ex2.last_native is True
    with pytest.raises(RuntimeError):
        ex2(xq[:, :2], xp[:, :2])                           # two channels: the torch path, conv0's error as in the reference
    assert ex2.last_native is False
    seq2.train()
    ex2(xq, xp)
    assert ex2.last_native is False
    drv = nn.Sequential(*list(model.children()))                                              # the other drivers' form
    with pytest.raises(RuntimeError):
        S.SimAtt(drv, drv[0], ["relu"])(xq, xp)
