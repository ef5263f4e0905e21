"""ResNet50 on the MI355X: the channels-last terms convolution (mirx_conv_terms) on every convolution shape of ResNet-50,
its glue kernels, and the model end to end against a float64 restatement."""
import pytest
import torch
import torch.nn.functional as F

from oracle.densenet import randomize_bn_stats
from _convterms_ref import _decode, _pow2_scale
from _convterms_ref import _run_and_check as _check_hw
from _resnet_ref import embed

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (cin, cout, k, stride, side in): every distinct convolution of ResNet-50 v1.5 at 224 x 224
SHAPES = [
    (64, 64, 1, 1, 56), (256, 64, 1, 1, 56), (64, 64, 3, 1, 56), (64, 256, 1, 1, 56),
    (256, 128, 1, 1, 56), (512, 128, 1, 1, 28), (128, 128, 3, 2, 56), (128, 128, 3, 1, 28), (128, 512, 1, 1, 28),
    (256, 512, 1, 2, 56),
    (512, 256, 1, 1, 28), (1024, 256, 1, 1, 14), (256, 256, 3, 2, 28), (256, 256, 3, 1, 14), (256, 1024, 1, 1, 14),
    (512, 1024, 1, 2, 28),
    (1024, 512, 1, 1, 14), (2048, 512, 1, 1, 7), (512, 512, 3, 2, 14), (512, 512, 3, 1, 7), (512, 2048, 1, 1, 7),
    (1024, 2048, 1, 2, 14),
]


def _run_and_check(shape, n, seed, mags, res, relu, report=None):
    """shape = (cin, cout, k, stride, side): the square map of _convterms_ref._run_and_check"""
    cin, cout, k, s, side = shape
    _check_hw((cin, cout, k, s, side, side), n, seed, mags, res, relu, report)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d-%d_k%ds%d_%d" % s)
def test_conv_terms_every_resnet_shape(shape):
    """plain and +residual +ReLU, three images of magnitudes 1e-3 / 1 / 1e3 per launch (pixel tiles straddle them), both
    outputs (terms rows and fp32 rows) of one launch against float64."""
    loose = []
    _run_and_check(shape, 3, 11, (1e-3, 1.0, 1e3), res=False, relu=False, report=loose)
    _run_and_check(shape, 3, 12, (1e3, 1e-3, 1.0), res=True, relu=True, report=loose)
    print("bound / max|y| for", shape, ["%.1f" % v for v in loose])


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[6], SHAPES[13], SHAPES[19], SHAPES[21]],
                         ids=lambda s: "c%d-%d_k%ds%d_%d" % s)
@pytest.mark.parametrize("n", [1, 64])
def test_conv_terms_batch_sizes(shape, n):
    """n = 1 (the last tile partial) and n = 64 (many straddling tiles); relu without residual."""
    _run_and_check(shape, n, 21, (1.0, 1e2, 1e-2), res=False, relu=True)


def test_conv_terms_rejects_bad_arguments():
    from mirx import _lib
    lib = _lib.load()
    rc = lib.mirx_conv_terms(None, None, None, 1, 8, 8, 48, 3, 1, None, None, None, 64, 1.0, 0.0, None, None, None, 0,
                             None, None, None, None, None)
    assert rc == -1
    rc = lib.mirx_conv_terms(None, None, None, 1, 8, 8, 64, 5, 1, None, None, None, 64, 1.0, 0.0, None, None, None, 0,
                             None, None, None, None, None)
    assert rc == -1 and b"kernel size" in lib.mirx_last_error()


def test_nchw_to_terms():
    from mirx import _lib
    from mirx.model import _ptr, _stream
    n, c, hw = 5, 64, 56 * 56
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, c, hw, generator=g) * torch.tensor([1e-3, 1.0, 1e3, 7.0, 0.0]).view(n, 1, 1)
    xg = x.to(DEV)
    rng = xg.abs().reshape(n, -1).amax(dim=1).contiguous()
    xt = torch.empty((n * hw, 2 * c), dtype=torch.float16, device=DEV)
    sc = torch.empty((n,), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mirx_nchw_to_terms(_ptr(xg), c * hw, n, c, hw, _ptr(rng), _ptr(sc), _ptr(xt), _stream(xg.device)))
    torch.cuda.synchronize()
    want = _pow2_scale(rng.cpu().double())
    assert torch.equal(sc.cpu().double(), want)
    dec = _decode(xt, sc, n)
    ref = x.double().permute(0, 2, 1)
    for b in range(n):
        assert float((dec[b] - ref[b]).abs().max()) <= 2.0 ** -21 * float(rng[b]), b


@pytest.mark.parametrize("normalize", [0, 1])
def test_gap_nhwc_head(normalize):
    from mirx import _lib
    from mirx.model import _ptr, _stream
    n, hw, c = 6, 49, 2048
    x = torch.randn(n, hw, c, generator=torch.Generator().manual_seed(5)).abs()
    xg = x.to(DEV)
    y = torch.empty((n, c), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mirx_gap_nhwc_l2norm(_ptr(xg), n, hw, c, normalize, _ptr(y), _stream(xg.device)))
    ref = x.double().mean(dim=1)
    if normalize:
        ref = F.normalize(ref, dim=1)
    assert float((y.cpu().double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def _model(emb=None, seed=0):
    from mirx.model import ResNet50
    torch.manual_seed(seed)
    m = ResNet50(embedding_dim=emb)
    m.load_state_dict(randomize_bn_stats(m.state_dict(), seed=seed + 3))
    return m.eval().to(DEV)


def _images(n, h=224, w=224, seed=1):
    return torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("emb", [None, 512])
def test_end_to_end_matches_float64(emb):
    m = _model(emb)
    x = _images(3)
    with torch.no_grad():
        y = m(x.to(DEV))
    ref = embed(x, m.state_dict())
    assert float((y.cpu().double() - ref).abs().max()) <= 1e-5
    r = m.__dict__["_mirx_last_ranges"]
    assert torch.isfinite(r).all()


def test_end_to_end_non_square():
    m = _model(None, seed=4)
    x = _images(2, 160, 192, seed=6)
    with torch.no_grad():
        y = m(x.to(DEV))
    assert float((y.cpu().double() - embed(x, m.state_dict())).abs().max()) <= 1e-5


def test_native_path_runs_no_library_convolution():
    m = _model(None)
    x = _images(2).to(DEV)
    from torch.profiler import ProfilerActivity, profile
    with torch.no_grad(), profile(activities=[ProfilerActivity.CPU]) as prof:
        m(x)
    names = {e.name for e in prof.events()}
    assert not any("conv" in nm.lower() and nm.startswith("aten::") for nm in names), sorted(names)
    with pytest.raises(ValueError):
        with torch.no_grad():
            m(_images(1, 226, 224).to(DEV))


def test_batch_independence_bit_identical():
    m = _model(None, seed=7)
    x = _images(64, seed=8).to(DEV)
    with torch.no_grad():
        full = m(x)
        for i in (0, 17, 63):
            assert torch.equal(m(x[i:i + 1])[0], full[i]), i
        assert torch.equal(m(x[30:32]), full[30:32])


def test_containment_of_non_finite_images():
    m = _model(None, seed=9)
    x = _images(8, seed=10)
    bad = x.clone()
    bad[3] = float("nan")
    bad[5] = 1e30
    with torch.no_grad():
        clean = m(x.to(DEV))
        dirty = m(bad.to(DEV))
    keep = [i for i in range(8) if i not in (3, 5)]
    assert torch.equal(clean[keep], dirty[keep])
    assert not torch.isfinite(dirty[3]).all()


def test_uint8_input_bit_identical_to_normalised_fp32():
    """ToTensor + Normalize inside the stem against the reference's CPU transform (u / 255, - mean, / std in fp32)."""
    m = _model(None, seed=11)
    u = torch.randint(0, 256, (4, 3, 224, 224), dtype=torch.uint8, generator=torch.Generator().manual_seed(12))
    u[2] = 0
    xf = m.normalize_uint8(u)                                  # CPU tensor in, CPU ops
    with torch.no_grad():
        a = m(u.to(DEV))
        b = m(xf.to(DEV))
    assert torch.equal(a, b)


def test_cache_follows_new_weights():
    m = _model(None, seed=13)
    x = _images(2, seed=14)
    with torch.no_grad():
        first = m(x.to(DEV))
        sd = randomize_bn_stats(_model(None, seed=15).state_dict(), seed=16)
        m.load_state_dict(sd)
        second = m(x.to(DEV))
        assert not torch.equal(first, second)
        assert float((second.cpu().double() - embed(x, m.state_dict())).abs().max()) <= 1e-5
        m.resnet50[4][0].conv1.weight.mul_(1.5)                       # in-place edit
        third = m(x.to(DEV))
        assert float((third.cpu().double() - embed(x, m.state_dict())).abs().max()) <= 1e-5


def test_retrieval_round_trip():
    from mirx.retriever import Collection, get_model_and_transform
    model, tf = get_model_and_transform("resnet50", None, 512, "cuda")
    x = _images(16, seed=17).to(DEV)
    with torch.no_grad():
        e = model(x)
    assert e.shape == (16, 512)
    col = Collection("resnet50", 512)
    col.insert([[f"img{i}.png" for i in range(16)], list(range(16)), e])
    hits = col.search(e, limit=3)
    assert [h[0].id for h in hits] == list(range(16))


# ---- the model at the sizes whose maps are odd, non-square or down to 1 x 1 (test_conv_terms_edges_gpu.py has the kernel) ------
_SMALL = {}


def _small_model():
    if "m" not in _SMALL:
        _SMALL["m"] = _model(None, seed=21)
    return _SMALL["m"]


@pytest.mark.parametrize("h,w", [(8, 8), (12, 20), (36, 52), (100, 100)])
def test_end_to_end_small_and_odd(h, w):
    """8 x 8: every map from layer2 on is 1 x 1; 12 x 20: 3 x 5 -> 2 x 3 -> 1 x 2 -> 1 x 1; 36 x 52: 9 x 13 -> 5 x 7 -> 3 x 4 ->
    2 x 2; 100 x 100: 25 -> 13 -> 7 -> 4 (every stride-2 input odd)."""
    m = _small_model()
    x = _images(3, h, w, seed=22)
    with torch.no_grad():
        y = m(x.to(DEV))
    err = float((y.cpu().double() - embed(x, m.state_dict())).abs().max())
    print(f"resnet50 {h} x {w}: native {err:.3e}")
    assert y.shape == (3, 2048)
    assert err <= 1e-5


def test_batch_independence_8x8_bit_identical():
    """200 images of 8 x 8: from layer2 on 128 images share a pixel tile; images either side of that boundary alone"""
    m = _small_model()
    x = _images(200, 8, 8, seed=23).to(DEV)
    with torch.no_grad():
        full = m(x)
        for i in (0, 127, 128, 199):
            assert torch.equal(m(x[i:i + 1])[0], full[i]), i
    assert torch.isfinite(full).all()


def test_containment_8x8_of_a_nan_image():
    m = _small_model()
    x = _images(200, 8, 8, seed=24)
    bad = x.clone()
    bad[127] = float("nan")
    with torch.no_grad():
        clean = m(x.to(DEV))
        dirty = m(bad.to(DEV))
    keep = [i for i in range(200) if i != 127]
    assert torch.equal(clean[keep], dirty[keep])
    assert torch.isfinite(clean).all() and not torch.isfinite(dirty[127]).all()
