"""MedSigLIP Grad-CAM on the CPU: the float64 restatement (_gradcam_ref) and mirx.xai's torch path against the fixture made by
the reference's own functions (tests/golden/make_golden_gradcam.py), the surface, the model's side effects, the failures kept
from the reference, and the ctypes signatures and argument checks of the new entry points."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _gradcam_ref as R
from mirx import _lib, xai
from mirx import siglip_gradcam as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gradcam_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _model(gold, case=None):
    m = R.build_model({k[2:]: v for k, v in gold.items() if k.startswith("w/")})
    if case == "flat":
        with torch.no_grad():
            m.projection[3].weight.zero_()
    return m


def _case(gold, case):
    return (torch.from_numpy(gold[f"{case}_query"]).double(), torch.from_numpy(gold[f"{case}_retrieved"]).double(),
            torch.from_numpy(gold[f"{case}_qemb"]))


def test_fixture_covers_the_issue_cases(gold):
    assert gold["k1_out"].shape == (1,) + R.SIZE and gold["k3_out"].shape == (R.BATCH,) + R.SIZE
    assert gold["bq2_qemb"].shape[0] == 2 and gold["k1_qemb"].shape[0] == 1
    assert np.all(gold["flat_out"] == 0)
    nan = gold["nan_out"]
    assert np.isnan(gold["nan_retrieved"][R.NAN_IMAGE]).any() and np.all(nan[R.NAN_IMAGE] == 0)
    keep = [i for i in range(R.BATCH) if i != R.NAN_IMAGE]
    assert np.array_equal(nan[keep], gold["k3_out"][keep])
    for c in R.CASES:
        if c != "flat":
            assert gold[f"{c}_out"].max() == 1.0
    assert R.N % 16 != 0 and os.path.getsize(GOLD) < 1 << 20


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_matches_the_fixture(gold, case):
    m = _model(gold, case)
    _, r, qemb = _case(gold, case)
    W = {k: v.double().numpy() for k, v in m.state_dict().items()}
    exp = R.expected(W, R.last_tokens(m, r), qemb.numpy(), R.VISION["num_attention_heads"], R.SIZE)
    assert float(np.abs(exp - gold[f"{case}_out"]).max()) <= 1e-10


@pytest.mark.parametrize("case", R.CASES)
def test_torch_path_matches_the_fixture(gold, case):
    m = _model(gold, case)
    q, r, qemb = _case(gold, case)
    if case == "bq2":
        got = np.stack([xai._compute_single_gradcam(m, qemb, r[i:i + 1], torch.device("cpu")) for i in range(r.shape[0])])
        assert xai._compute_single_gradcam.last_native is False
    else:
        got = xai.compute_gradcam_saliency(m, q, r, torch.device("cpu"))
        assert xai.compute_gradcam_saliency.last_native is False
    assert got.dtype == np.float64 and got.shape == gold[f"{case}_out"].shape
    assert float(np.abs(got - gold[f"{case}_out"]).max()) <= 1e-12


def test_surface_and_signatures():
    assert xai.compute_gradcam_saliency is G.compute_gradcam_saliency
    assert xai._compute_single_gradcam is G._compute_single_gradcam
    assert list(inspect.signature(G.compute_gradcam_saliency).parameters) == ["model", "query_tensor", "retrieved_tensor", "device"]
    assert list(inspect.signature(G._compute_single_gradcam).parameters) == ["model", "query_emb", "img_tensor", "device"]


def test_side_effects_eval_and_device(gold):
    m = _model(gold).float().train()
    q, r, _ = _case(gold, "k1")
    out = xai.compute_gradcam_saliency(m, q.float(), r.float(), torch.device("cpu"))
    assert not m.training and not m.backbone.training and out.dtype == np.float32
    assert all(p.device.type == "cpu" for p in m.parameters())


def test_non_square_and_query_batch_raise(gold):
    m = _model(gold)
    emb = m.backbone.embeddings                                 # 28 x 42 images: a 4 x 6 grid of 24 tokens
    emb.num_positions = 24
    emb.position_embedding = torch.nn.Embedding(24, R.VISION["hidden_size"]).double()
    img = torch.randn(2, 3, 28, 42, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        xai.compute_gradcam_saliency(m, img[:1], img[1:], torch.device("cpu"))
    with pytest.raises(RuntimeError):
        xai._compute_single_gradcam(m, m(img[:1]).detach(), img[1:], torch.device("cpu"))
    m = _model(gold)
    q, r, _ = _case(gold, "k1")
    with pytest.raises(RuntimeError):
        xai.compute_gradcam_saliency(m, torch.cat([q, q]), r, torch.device("cpu"))


def test_ctypes_signatures():
    lib = _lib.load()
    for name, (res, args) in _lib.SYMBOLS.items():
        if name.startswith("mirx_gradcam_"):
            f = getattr(lib, name)
            assert f.restype is res and f.argtypes == args, name
    assert len([n for n in _lib.SYMBOLS if n.startswith("mirx_gradcam_")]) == 9


def test_slot_layout_mirrors_the_library():
    """R.slot_layout (the layout written in include/mirx.h and DESIGN 21) against mirx_gradcam_workspace_floats."""
    lib = _lib.load()
    seen = 0
    for n in (1, 2, 3, 4, 5, 25, 257, 1024):
        for d in (1, 7, 40, 64, 1152, 8192):
            for heads in [h for h in range(1, 17) if d % h == 0]:
                s = R.slot_layout(n, d, heads)
                assert s["per"] % 4 == 0 and 0 <= s["per"] - (s["minmax"] + 1024) < 4
                assert (s["P"], s["dP"] - s["P"], s["dsum"] - s["dP"], s["partials"] - s["dsum"]) == (2 * n, n * heads, n * heads, 16)
                assert (s["wbar"] - s["partials"], s["cam"] - s["wbar"], s["minmax"] - s["cam"]) == (-(-n // 4) * d, d, n)
                for b in (0, 1, 3):
                    assert lib.mirx_gradcam_workspace_floats(b, n, d, heads) == b * s["per"], (b, n, d, heads)
                    seen += 1
    assert seen >= 8 * 6 * 3


def test_trace_names_every_intermediate(gold):
    m = _model(gold)
    _, r, qemb = _case(gold, "k1")
    W = {k: v.double().numpy() for k, v in m.state_dict().items()}
    x = R.last_tokens(m, r)[0]
    heads = R.VISION["num_attention_heads"]
    t = R.trace(W, x, qemb.numpy(), heads)
    assert set(R.TRACE_KEYS) <= set(t) and all(t[k].dtype == np.float64 for k in R.TRACE_KEYS)
    assert np.array_equal(t["g_x"], R.grad_x(W, x, qemb.numpy(), heads))
    n, d = x.shape
    assert t["mu"].shape == t["r"].shape == (n,) and t["P"].shape == t["dP"].shape == (n, heads)
    assert t["ybar"].shape == t["w"].shape == (heads, d) and t["e"].shape == t["dsum"].shape == (heads,)
    assert np.abs(t["P"].sum(0) - 1).max() <= 1e-14 and np.abs(t["dsum"] - (t["P"] * t["dP"]).sum(0)).max() == 0
    assert np.abs(t["y"] - ((x - t["mu"][:, None]) * t["r"][:, None] * W["backbone.post_layernorm.weight"]
                            + W["backbone.post_layernorm.bias"])).max() <= 1e-13


def test_normalise_rule_at_the_threshold():
    """numpy's `max - min > 1e-8` on float32 maps, the oracle of the planted cases of tests/test_gradcam_kernels_gpu.py: a
    float32 spread above 1e-8 normalises to {0, 1}; 2^-27, float32(1e-8) itself, a constant and all zeros give zeros."""
    tiny = np.float32(1e-8)

    def two(hi):
        return np.array([[0, hi], [hi, 0]], dtype=np.float32)

    for hi in (np.float32(2.0 ** -26), np.nextafter(tiny, np.float32(1))):
        out = G._normalise01(two(hi))
        assert out.dtype == np.float32 and np.array_equal(out, two(1.0))
    for m in (two(np.float32(2.0 ** -27)), two(tiny), np.full((2, 2), 0.75, np.float32), np.zeros((2, 2), np.float32)):
        out = G._normalise01(m)
        assert out.dtype == np.float32 and not out.any()
    assert float(tiny) < 1e-8 < float(np.nextafter(tiny, np.float32(1)))        # either comparison width gives the same answers


def test_argument_checks_without_a_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    assert lib.mirx_gradcam_workspace_floats(1, 1025, 64, 4) == -1          # n > 1024
    assert lib.mirx_gradcam_workspace_floats(1, 25, 64, 17) == -1           # heads > 16
    assert lib.mirx_gradcam_workspace_floats(1, 25, 66, 4) == -1            # d % heads
    assert lib.mirx_gradcam_workspace_floats(1, 1024, 1152, 16) > 0
    ws = lib.mirx_gradcam_workspace_floats(1, 25, 64, 4)
    assert lib.mirx_gradcam_pool(p, 1, 25, 64, 4, p, p, 1e-6, p, p, p, ws - 1, p, None) == -1       # workspace too small
    assert lib.mirx_gradcam_pool(p, 1, 25, 64, 4, p, p, float("nan"), p, p, p, ws, p, None) == -1  # eps
    assert lib.mirx_gradcam_pool(p, 1, 25, 64, 4, None, p, 1e-6, p, p, p, ws, p, None) == -1       # null
    assert lib.mirx_gradcam_pool(ctypes.c_void_p(66), 1, 25, 64, 4, p, p, 1e-6, p, p, p, ws, p, None) == -1   # alignment
    assert lib.mirx_gradcam_tokens(p, 70000, 25, 64, 4, p, p, p, p, p, p, ws, None) == -1          # b > 65535
    ws24 = lib.mirx_gradcam_workspace_floats(1, 24, 64, 4)
    assert lib.mirx_gradcam_finish(p, 1, 24, 64, 4, p, ws24, 35, 35, p, None) == -1                # n not a square
    assert lib.mirx_gradcam_finish(p, 1, 25, 64, 4, p, ws, 8193, 35, p, None) == -1               # H > 8192
    assert lib.mirx_gradcam_finish(p, 1, 25, 64, 4, p, ws, 0, 35, p, None) == -1
    assert lib.mirx_gradcam_gemv(p, 4, p, 4, None, None, 0, p, 4, 1, 0, 4, 1, 1, 0, 0, None) == -1  # m = 0
    assert lib.mirx_gradcam_layernorm(p, 1, 8193, p, p, 1e-5, 0, p, p, None) == -1
    assert lib.mirx_gradcam_layernorm_bwd(p, None, p, p, None, 1, 16, None, p, None) == -1
    assert lib.mirx_gradcam_gelu(p, None, 4, 1, p, None) == -1                                     # mode 1 needs g
    assert lib.mirx_gradcam_cosine_bwd(p, 1, 16, p, 0, p, None) == -1                              # bq = 0
    assert b"gradcam" in lib.mirx_last_error()


def test_each_bad_argument_is_einval_and_names_its_entry_point():
    """Every limit of include/mirx.h's Grad-CAM comment, one call each: MIRX_EINVAL (-1) before anything is launched (the
    pointers are not dereferenced), and mirx_last_error() starts with the entry point's name."""
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    ws = lib.mirx_gradcam_workspace_floats(1, 25, 64, 4)
    assert ws == R.slot_layout(25, 64, 4)["per"]

    def pool(n=25, d=64, heads=4, eps=1e-6, wsf=ws):
        return lib.mirx_gradcam_pool(p, 1, n, d, heads, p, p, eps, p, p, p, wsf, p, None)

    def tokens(n=25, d=64, heads=4, wsf=ws):
        return lib.mirx_gradcam_tokens(p, 1, n, d, heads, p, p, p, p, p, p, wsf, None)

    def finish(n=25, d=64, heads=4, wsf=ws, H=35, W=35):
        return lib.mirx_gradcam_finish(p, 1, n, d, heads, p, wsf, H, W, p, None)

    def gemv(lda=4, xs=4, rs=0, os_=4, acol=0, xg=0):
        return lib.mirx_gradcam_gemv(p, lda, p, xs, None, None, rs, p, os_, 1, 4, 4, 4, 4, acol, xg, None)

    big = 1 << 40                                   # a workspace size that passes: the dims must be what fails
    calls = []
    for name, f in (("gradcam_pool", pool), ("gradcam_tokens", tokens), ("gradcam_finish", finish)):
        calls += [(name, lambda f=f: f(wsf=ws - 1)), (name, lambda f=f: f(d=66, wsf=big)), (name, lambda f=f: f(n=1025, wsf=big)),
                  (name, lambda f=f: f(heads=17, d=68, wsf=big))]
    calls += [("gradcam_finish", lambda: finish(H=0)), ("gradcam_finish", lambda: finish(W=8193)),
              ("gradcam_finish", lambda: finish(H=8193)), ("gradcam_finish", lambda: finish(W=0)),
              ("gradcam_pool", lambda: pool(eps=-1e-6)), ("gradcam_pool", lambda: pool(eps=float("nan"))),
              ("gradcam_pool", lambda: pool(eps=float("inf"))),
              ("gradcam_layernorm", lambda: lib.mirx_gradcam_layernorm(p, 1, 16, p, p, -1e-6, 0, p, p, None)),
              ("gradcam_layernorm", lambda: lib.mirx_gradcam_layernorm(p, 1, 16, p, p, float("nan"), 0, p, p, None)),
              ("gradcam_layernorm", lambda: lib.mirx_gradcam_layernorm(p, 1, 8193, p, p, 1e-5, 0, p, p, None)),
              ("gradcam_layernorm", lambda: lib.mirx_gradcam_layernorm(p, 1, 0, p, p, 1e-5, 0, p, p, None)),
              ("gradcam_layernorm_bwd", lambda: lib.mirx_gradcam_layernorm_bwd(p, None, p, p, p, 1, 8193, None, p, None)),
              ("gradcam_gelu", lambda: lib.mirx_gradcam_gelu(p, p, 4, 2, p, None)),
              ("gradcam_gelu", lambda: lib.mirx_gradcam_gelu(p, p, 4, -1, p, None)),
              ("gradcam_cosine_bwd", lambda: lib.mirx_gradcam_cosine_bwd(p, 1, 16, p, 0, p, None)),
              ("gradcam_cosine_bwd", lambda: lib.mirx_gradcam_cosine_bwd(p, 1, 8193, p, 1, p, None))]
    for kw in ("lda", "xs", "rs", "os_", "acol", "xg"):
        calls.append(("gradcam_gemv", lambda kw=kw: gemv(**{kw: -1})))
    assert len(calls) == 34
    for name, call in calls:
        assert call() == -1, name
        msg = lib.mirx_last_error()
        assert msg.startswith(name.encode() + b":"), (name, msg)
    # the same calls with the limits met pass the checks up to the null test only when b = 0 asks for no launch
    assert lib.mirx_gradcam_pool(p, 0, 25, 64, 4, p, p, 1e-6, p, p, p, 0, p, None) == 0
    assert lib.mirx_gradcam_gemv(p, 4, p, 4, None, None, 0, p, 4, 0, 4, 4, 4, 4, 0, 0, None) == 0
