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
