"""SimCAM on the CPU: the float64 restatement (_simcam_ref) against the fixture made by the reference's own explainer classes
(tests/golden/make_golden_simcam.py), mirx.xai's SimCAM / SimCAM_Densenet121 / SimCAM_MedSigLIP (the torch path off the GPU)
against the same fixture, and the classes' signatures and argument checks."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import _simcam_ref as R
from mirx import xai
from mirx.simcam import SimCAM, SimCAM_Densenet121, SimCAM_MedSigLIP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simcam_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture
def f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)          # as the fixture ran (SimCAM_Densenet121 fills a default-dtype tensor)
    yield
    torch.set_default_dtype(old)


def _fc(gold, case):
    if not case.get("fc"):
        return None
    fc = nn.Linear(case["c"], case["fc"]).double()
    with torch.no_grad():
        fc.weight.copy_(torch.from_numpy(gold[case["name"] + "_fc_w"]))
        fc.bias.copy_(torch.from_numpy(gold[case["name"] + "_fc_b"]))
    return fc


def _same(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    scale = max(1.0, float(np.abs(b[ok]).max())) if ok.any() else 1.0
    err = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    assert err <= tol * scale, err


def test_fixture_covers_the_issue_cases(gold):
    names = {c["name"] for c in R.CASES}
    assert all(f"{n}_out" in gold for n in names)
    assert np.isnan(gold["dn_zero_out"]).all()                                   # max(D) = 0 without eps: NaN, as there
    assert gold["cam_signed_out"].shape == (3, 2, 10, 14) and gold["cam_q2_out"].shape == (3, 2, 10, 14)
    assert gold["dn_plain_out"].shape == (2, 10, 14) and gold["sig_k3_out"].shape == (3, 12, 12)
    assert os.path.getsize(GOLD) < 1 << 20


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_restatement_matches_the_fixture(gold, case):
    n = case["name"]
    exp = R.case_expected(case, gold[n + "_xq"], gold[n + "_x"], gold.get(n + "_fc_w"), gold.get(n + "_fc_b"))
    _same(exp, gold[n + "_out"], 1e-12)


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_torch_path_matches_the_fixture(gold, case, f64_default):
    n = case["name"]
    explainer = R.case_model(case, xai, _fc(gold, case))
    xq, x = torch.from_numpy(gold[n + "_xq"]), torch.from_numpy(gold[n + "_x"])
    out = explainer(xq, x) if case["cls"] == "SimCAM_MedSigLIP" else explainer(xq, x, point=case.get("point"))
    assert explainer.last_native is False
    _same(out.numpy(), gold[n + "_out"], 1e-12)


def test_signatures_are_the_references():
    assert xai.SimCAM is SimCAM and xai.SimCAM_Densenet121 is SimCAM_Densenet121 and xai.SimCAM_MedSigLIP is SimCAM_MedSigLIP
    assert list(inspect.signature(SimCAM.__init__).parameters) == ["self", "model", "target_layer", "fc"]
    assert list(inspect.signature(SimCAM.forward).parameters) == ["self", "x_q", "x", "point"]
    assert list(inspect.signature(SimCAM_Densenet121.__init__).parameters) == ["self", "model", "feature_module", "target_layers", "fc"]
    assert list(inspect.signature(SimCAM_Densenet121.forward).parameters) == ["self", "x_q", "x", "point"]
    assert list(inspect.signature(SimCAM_MedSigLIP.__init__).parameters) == ["self", "model", "target_layer"]
    assert list(inspect.signature(SimCAM_MedSigLIP.forward).parameters) == ["self", "x_q", "x"]
    for cls in (SimCAM, SimCAM_Densenet121, SimCAM_MedSigLIP):
        assert issubclass(cls, nn.Module)


def test_medsiglip_needs_a_single_query():
    model = R.TokenNet(2).eval()
    ex = SimCAM_MedSigLIP(model, model.backbone.post_layernorm)
    with pytest.raises(AssertionError):
        ex(torch.randn(2, 3, 12, 12), torch.randn(1, 3, 12, 12))


def test_medsiglip_needs_a_square_grid():
    model = R.TokenNet(2).eval()
    ex = SimCAM_MedSigLIP(model, model.backbone.post_layernorm)
    with pytest.raises(AssertionError):
        ex(torch.randn(1, 3, 10, 14), torch.randn(1, 3, 10, 14))


@pytest.mark.parametrize("point", [(-1, 0), (0, -0.5), (10, 3), (3, 14), (1e9, 0)])
def test_points_outside_the_image_raise(point):
    model = R.PoolNet(2).eval()
    feats = R.pool_features(2)
    seq = nn.Sequential(feats, nn.AdaptiveAvgPool2d((1, 1))).eval()
    xq, x = torch.randn(1, 3, 10, 14), torch.randn(2, 3, 10, 14)
    with pytest.raises(ValueError):
        SimCAM(model, model.tap)(xq, x, point=point)
    with pytest.raises(ValueError):
        SimCAM_Densenet121(seq, seq[0], ["relu"])(xq, x, point=point)


def test_reference_failures_are_kept():
    model = R.PoolNet(2).eval()
    with pytest.raises(RuntimeError, match="hook failed"):
        SimCAM(model, nn.ReLU())(torch.randn(1, 3, 10, 14), torch.randn(1, 3, 10, 14))        # a layer the model never runs
    tower = R.TokenNet(2).eval()
    with pytest.raises(RuntimeError, match="did not capture"):
        SimCAM_MedSigLIP(tower, nn.Identity())(torch.randn(1, 3, 12, 12), torch.randn(1, 3, 12, 12))


def test_densenet_feature_stack_knows_its_model_outside_the_state_dict():
    from mirx.model import DenseNet121
    m = DenseNet121(embedding_dim=8)
    f = m.densenet121[0]
    assert f.__dict__["_mirx_owner"]() is m
    assert "_mirx_owner" not in dict(f.named_modules()) and not any("owner" in k for k in m.state_dict())
    m2 = DenseNet121(embedding_dim=8)
    m2.load_state_dict(m.state_dict(), strict=True)
    # the reference driver's Sequential of the wrapper's children: features, avgpool, fc
    seq = nn.Sequential(*list(m.children())[0], *list(m.children())[1:])
    assert seq[0] is f and seq[2] is m.fc


def test_densenet_pickles_and_copies_with_its_owner_reference():
    import copy
    import io
    import pickle

    from mirx.model import DenseNet121
    from mirx.simcam import _densenet_owner
    torch.manual_seed(0)
    m = DenseNet121(embedding_dim=8).eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        ref = m(x)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    copies = [torch.load(buf, weights_only=False), pickle.loads(pickle.dumps(m)), copy.deepcopy(m)]
    for c in copies:
        f = c.densenet121[0]
        assert f is not m.densenet121[0]
        assert f.__dict__["_mirx_owner"]() is c                                  # the copy's stack resolves to the copy
        seq = nn.Sequential(*list(c.children())[0], *list(c.children())[1:])
        assert _densenet_owner(seq, seq[0], ["relu"]) is c
        with torch.no_grad():
            assert torch.equal(c(x), ref)
    assert m.densenet121[0].__dict__["_mirx_owner"]() is m                       # the original is untouched
    feats = copy.deepcopy(m.densenet121[0])                                      # a stack copied on its own has no owner
    assert feats.__dict__["_mirx_owner"]() is None
