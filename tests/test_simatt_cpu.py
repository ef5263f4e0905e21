"""SimAtt on the CPU: the float64 restatement of the closed form (_simatt_ref) against the fixture made by the reference's own
class (tests/golden/make_golden_simatt.py), mirx.xai.SimAtt's torch path against the same fixture and its exception types, the
closed form against autograd, simatt_pairs' fallback against the per-pair calls, argument validation and the ABI symbols."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import _simatt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "simatt_ref.npz")
IDS = [c["name"] for c in R.CASES]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _inputs(gold, name):
    return tuple(torch.from_numpy(gold[f"{name}_{k}"]) if f"{name}_{k}" in gold else None for k in ("xq", "xp", "xn"))


def _fc(gold, case):
    return R.make_fc(gold[case["name"] + "_fc_w"], gold[case["name"] + "_fc_b"]) if case["fc"] else None


def test_fixture_covers_the_issue_cases(gold):
    assert all(f"{n}_out" in gold for n in IDS)
    for base in ("ap", "an", "triplet", "p1n2"):
        assert f"{base}_out" in gold and f"{base}_fc_out" in gold
    assert gold["ap_out"].shape == (2, 10, 14) and gold["triplet_out"].shape == (3, 10, 14) and gold["p1n2_fc_out"].shape == (4, 10, 14)
    assert R.case_rows(*_inputs(gold, "ap"))[1] == (5, 7)                       # a non-square map
    rows = R.case_rows(*_inputs(gold, "ap_zero_channel"))[0]
    assert (rows[:, :, 2] == 0).all() and (rows[:, :, 0] > 0).any()             # a dead channel: sign(0) = 0
    assert {str(gold[f"fail_{n}"]) for n in R.FAILING} <= {"IndexError", "RuntimeError", "TypeError"}
    assert os.path.getsize(GOLD) < 1 << 19


@pytest.mark.parametrize("case", [c for c in R.CASES if c["fc"]], ids=[c["name"] for c in R.CASES if c["fc"]])
def test_fixture_embeddings_keep_their_sign_margin(gold, case):
    n = case["name"]
    assert R.sign_margin_ok(R.case_rows(*_inputs(gold, n))[0], gold[n + "_fc_w"], gold[n + "_fc_b"])


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_restatement_matches_the_fixture(gold, case):
    n = case["name"]
    exp = R.case_expected(*_inputs(gold, n), gold.get(n + "_fc_w"), gold.get(n + "_fc_b"))
    errs = R.map_errors(exp, gold[n + "_out"])
    assert max(errs) <= 1e-12, errs


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_torch_path_matches_the_fixture(gold, case):
    from mirx import xai
    n = case["name"]
    model = R.flat_model(_fc(gold, case)).double().eval()
    ex = xai.SimAtt(model, model[0], target_layers=["relu"])
    xq, xp, xn = _inputs(gold, n)
    out = ex(xq.clone().requires_grad_(True), xp, xn)       # (the tiny model has no parameter: the query carries the graph)
    assert ex.last_native is False and not out.requires_grad
    errs = R.map_errors(out.numpy(), gold[n + "_out"])
    assert max(errs) <= 1e-12, errs


@pytest.mark.parametrize("name", R.FAILING)
def test_failing_driver_forms_raise_what_the_reference_raises(gold, name):
    from mirx import xai
    fc = R.make_fc(np.zeros((R.FC_DIM, R.CHANNELS)), np.zeros(R.FC_DIM)) if name.endswith("_fc") else None
    model, module, targets = R.failing_form(name, fc)
    model = model.double().eval()
    g = torch.Generator().manual_seed(77)
    xq = torch.randn(1, R.CHANNELS, *R.SIZE, generator=g, dtype=torch.float64).requires_grad_(True)
    xp = torch.randn(1, R.CHANNELS, *R.SIZE, generator=g, dtype=torch.float64)
    exc = {"IndexError": IndexError, "RuntimeError": RuntimeError, "TypeError": TypeError}[str(gold[f"fail_{name}"])]
    with pytest.raises(exc):
        xai.SimAtt(model, module, target_layers=targets)(xq, xp)


def test_no_graph_raises_like_the_reference():
    from mirx.simatt import SimAtt
    model = R.flat_model().eval()
    ex = SimAtt(model, model[0], ["relu"])
    x = torch.randn(1, R.CHANNELS, *R.SIZE)
    with pytest.raises(RuntimeError):
        ex(x, x.clone())                                    # nothing requires grad
    with pytest.raises(RuntimeError), torch.no_grad():
        ex(x.clone().requires_grad_(True), x.clone())


@pytest.mark.parametrize("d", [None, 64])
@pytest.mark.parametrize("npos,nneg", [(1, 0), (0, 1), (1, 1), (1, 2)])
def test_closed_form_equals_autograd(d, npos, nneg):
    b, h, w, c = 1 + npos + nneg, 7, 7, 1024
    rows, fw, fb = R.make_rows(100 + 10 * npos + nneg, b, h * w, c, d)
    exp = R.simatt(rows, h, w, 32, 40, fw, fb, "group", positive=npos > 0)
    got = R.ref_torch(rows, h, w, 32, 40, fw, fb, "group", positive=npos > 0, dtype=torch.float64)
    assert max(R.map_errors(exp, got)) <= 1e-12
    if npos + nneg == 1:
        pairs = R.simatt(rows, h, w, 32, 40, fw, fb, "pairs", positive=npos > 0)
        assert pairs.shape == (1, 2, 32, 40) and np.array_equal(pairs[0], exp)


def test_pairs_fallback_equals_the_per_pair_calls(gold):
    from mirx.simatt import SimAtt, simatt_pairs
    case = next(c for c in R.CASES if c["name"] == "p1n2_fc")
    model = R.flat_model(_fc(gold, case)).double().eval()
    ex = SimAtt(model, model[0], ["relu"])
    xq, xp, xn = _inputs(gold, "p1n2_fc")
    xq = xq.clone().requires_grad_(True)
    xr = torch.cat((xp, xn))
    for positive in (True, False):
        out = simatt_pairs(ex, xq, xr, positive=positive)
        assert out.shape == (3, 2, 10, 14) and ex.last_native is False
        rows, (h, w) = R.case_rows(xq.detach(), xp, xn)
        exp = R.simatt(rows, h, w, 10, 14, gold["p1n2_fc_fc_w"], gold["p1n2_fc_fc_b"], "pairs", positive=positive)
        assert max(R.map_errors(out.numpy(), exp)) <= 1e-12
        for k in range(3):
            one = ex(xq, xr[k:k + 1]) if positive else ex(xq, None, xr[k:k + 1])
            assert torch.equal(one, out[k])
    built = simatt_pairs(model, xq, xr)                       # a bare flattened model: the explainer is built
    assert torch.equal(built, simatt_pairs(ex, xq, xr))
    with pytest.raises(ValueError):
        simatt_pairs(ex, xr, xr)                              # one query
    with pytest.raises(ValueError):
        simatt_pairs(ex, xq, xr[:, :, :8])


def test_signature_is_the_references():
    from mirx import xai
    from mirx.simatt import SimAtt, simatt_maps, simatt_pairs
    assert xai.SimAtt is SimAtt and xai.simatt_pairs is simatt_pairs and xai.simatt_maps is simatt_maps
    assert issubclass(SimAtt, nn.Module)
    assert list(inspect.signature(SimAtt.__init__).parameters) == ["self", "model", "feature_module", "target_layers"]
    sig = inspect.signature(SimAtt.forward)
    assert list(sig.parameters) == ["self", "x_q", "x_p", "x_n"]
    assert sig.parameters["x_p"].default is None and sig.parameters["x_n"].default is None
    assert list(inspect.signature(simatt_pairs).parameters) == ["model_or_explainer", "x_q", "x_r", "positive"]
    assert inspect.signature(simatt_pairs).parameters["positive"].default is True


def test_native_gate_is_closed_off_the_gpu_and_for_other_shapes():
    from mirx.model import DenseNet121
    from mirx.simatt import _densenet_side, _native_plan
    m = DenseNet121(embedding_dim=8).eval()
    seq = nn.Sequential(*list(m.children())[0], *list(m.children())[1:]).eval()
    x = torch.randn(2, 3, 64, 64)
    assert _native_plan(seq, seq[0], ["relu"], x) is None                       # CPU input
    assert _native_plan(seq, seq[0], None, x) is None and _native_plan(seq, seq[0], ["norm5"], x) is None
    drv = nn.Sequential(*list(m.children()))
    assert _native_plan(drv, drv[0], ["relu"], x) is None                       # the other drivers' form
    assert [_densenet_side(n) for n in (224, 256, 384, 32, 31, 1024)] == [7, 8, 12, 1, 1, 32]
    with torch.no_grad():
        assert m.densenet121[0](torch.randn(1, 3, 95, 224)).shape[-2:] == (_densenet_side(95), 7)


def test_a_stack_whose_model_was_collected_is_adopted():
    """compute_saliency.py:190 rebinds `model` to the Sequential: the DenseNet121 is gone, DenseNet121._adopt puts a headless
    one around the same stack (no parameter copied), which pickles and copies with the Sequential that keeps it."""
    import copy
    import gc
    import pickle
    from mirx.model import DenseNet121
    torch.manual_seed(0)
    model = DenseNet121(embedding_dim=8).eval()
    model = nn.Sequential(*list(model.children())[0], *list(model.children())[1:])
    gc.collect()
    stack = model[0]
    assert stack.__dict__["_mirx_owner"]() is None
    owner = DenseNet121._adopt(stack)
    assert owner.densenet121[0] is stack and stack.__dict__["_mirx_owner"]() is owner and owner.training is False
    assert {id(p) for p in owner.parameters()} == {id(p) for p in stack.parameters()} and owner.fc is None
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        assert torch.equal(owner.forward_eager(x), torch.flatten(model[1](stack(x)), 1))
    model.__dict__["_mirx_keep"] = owner
    for c in (copy.deepcopy(model), pickle.loads(pickle.dumps(model))):
        assert c[0] is not stack and c.__dict__["_mirx_keep"].densenet121[0] is c[0]
        assert c[0].__dict__["_mirx_owner"]() is c.__dict__["_mirx_keep"]
    assert "relu" in stack._modules and list(stack._modules)[-1] == "relu"     # adopted as it is: no second ReLU


def test_simatt_maps_validates_its_arguments():
    from mirx.simatt import simatt_maps
    rows = torch.zeros(2, 49, 16)
    with pytest.raises(ValueError, match="mode"):
        simatt_maps(rows, None, None, (8, 8), "both", 7, 7)
    with pytest.raises(ValueError, match="CUDA"):
        simatt_maps(rows, None, None, (8, 8), "group", 7, 7)
    with pytest.raises(ValueError, match="rows must be"):
        simatt_maps(rows, None, None, (8, 8), "group", 7, 6)
    with pytest.raises(ValueError, match="rows must be"):
        simatt_maps(rows[0], None, None, (8, 8), "group", 7, 7)


def test_abi_symbols_are_declared_and_bound():
    import ctypes
    import mirx._lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mirx.h")).read(), flags=re.S)
    for name, nargs in (("mirx_simatt", 16), ("mirx_simatt_workspace_floats", 4)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(L.SYMBOLS[name][1])
    assert L.SYMBOLS["mirx_simatt_workspace_floats"][0] is ctypes.c_int64 and L.SYMBOLS["mirx_simatt"][0] is ctypes.c_int
    assert (L.SIMATT_GROUP, L.SIMATT_PAIRS) == (0, 1)
    for macro, val in (("MIRX_SIMATT_MAX_HW", 1024), ("MIRX_SIMATT_MAX_C", 16384), ("MIRX_SIMATT_MAX_D", 16384),
                       ("MIRX_SIMATT_MAX_B", 65535), ("MIRX_SIMATT_MAX_SIZE", 8192), ("MIRX_SIMATT_GROUP", 0), ("MIRX_SIMATT_PAIRS", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), text), macro
    lib = L.load()
    # the limits answer without a GPU: nothing is launched
    assert lib.mirx_simatt_workspace_floats(2, 1024, 0, 0) == 2 * 1024 + 2 * 1024
    assert lib.mirx_simatt_workspace_floats(6, 1024, 64, 1) == 6 * 64 + 10 * (1024 + 64)
    for bad in ((1, 1024, 0, 0), (65536, 1024, 0, 0), (2, 0, 0, 0), (2, 16385, 0, 0), (2, 8, 16385, 0), (2, 8, -1, 0), (2, 8, 0, 2)):
        assert lib.mirx_simatt_workspace_floats(*bad) == -1 and b"simatt" in lib.mirx_last_error()
    assert lib.mirx_simatt(None, 2, 33, 32, 8, None, None, 0, 0, 0, 8, 8, None, 0, None, None) == -1
    assert lib.mirx_simatt(None, 2, 7, 7, 8, None, None, 0, 0, 0, 8, 9000, None, 0, None, None) == -1
    assert lib.mirx_simatt(None, 2, 7, 7, 8, None, None, 0, 0, 0, 8, 8, None, 0, None, None) == -1 and b"null" in lib.mirx_last_error()
