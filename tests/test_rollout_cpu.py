"""Attention rollout on the CPU: the float64 restatement (_rollout_ref) against the fixture made by the reference's own
AttentionRolloutMedSigLIP (tests/golden/make_golden_rollout.py), mirx.xai's AttentionRolloutMedSigLIP (the torch path off the
GPU) against the same fixture, the class's surface and the ctypes signatures of the new entry points."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import _rollout_ref as R
from mirx import xai
from mirx.rollout import AttentionRolloutMedSigLIP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _inputs(gold, setup):
    pre = setup + "_"
    return {k[len(pre):]: v for k, v in gold.items() if k.startswith(pre) and not k.endswith("_out")}


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_fixture_covers_the_issue_cases(gold):
    assert {c["fusion"] for c in R.CASES} == {"mean", "max", "min"}
    assert {c["ratio"] for c in R.CASES} == {0.0, 0.5, 0.9} and {c["qg"] for c in R.CASES} == {True, False}
    assert any(R.SETUPS[c["setup"]]["d"] == R.SETUPS[c["setup"]]["e"] and c["qg"] for c in R.CASES)   # projection skipped
    for c in R.CASES:
        assert gold[c["name"] + "_out"].shape == (R.BATCH,) + R.SIZE
    assert os.path.getsize(GOLD) < 1 << 20


@pytest.mark.parametrize("fusion", ["mean", "max", "min"])
@pytest.mark.parametrize("ratio", [0.5, 0.9])
def test_fixture_has_ties_at_the_threshold(gold, fusion, ratio):
    atts = _inputs(gold, "proj")["atts"]
    k = max(1, int(R.N * ratio))
    for layer in range(R.LAYERS):
        a = R.fuse(atts[layer], fusion)
        thr = np.partition(a, k - 1, axis=-1)[..., k - 1:k]
        assert ((a == thr).sum(-1) >= 2).mean() >= 0.25     # a tie at the k-th smallest value in at least a quarter of the rows


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_restatement_matches_the_fixture(gold, case):
    exp = R.case_expected(case, _inputs(gold, case["setup"]))
    assert _rel(exp, gold[case["name"] + "_out"]) < 1e-6          # the reference's rollout runs in float32


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_torch_path_matches_the_fixture(gold, case):
    model = R.StandIn(_inputs(gold, case["setup"]))
    ex = xai.AttentionRolloutMedSigLIP(model, head_fusion=case["fusion"], discard_ratio=case["ratio"], query_guided=case["qg"])
    out = ex(R.pixels(1), R.pixels(R.BATCH))
    assert ex.last_native is False and ex.last_layers is None
    assert np.array_equal(out.numpy(), gold[case["name"] + "_out"])            # the same torch formulas: the same bits


def test_unknown_fusion_raises(gold):
    model = R.StandIn(_inputs(gold, "proj"))
    ex = AttentionRolloutMedSigLIP(model, head_fusion="median")
    with pytest.raises(ValueError, match="Unknown head_fusion mode"):
        ex(R.pixels(1), R.pixels(1))
    with pytest.raises(ValueError, match="Unknown head_fusion mode"):
        AttentionRolloutMedSigLIP._fuse_heads(torch.zeros(1, 2, 3, 3), "sum")


def test_discard_ratio_above_one_fails_as_kthvalue(gold):
    ex = AttentionRolloutMedSigLIP(R.StandIn(_inputs(gold, "proj")), discard_ratio=1.5)
    with pytest.raises(RuntimeError):
        ex(R.pixels(1), R.pixels(1))


def test_rollout_on_given_attentions(gold):
    """_rollout on attention tuples: its mean over rows is the restatement's importance."""
    atts = _inputs(gold, "proj")["atts"]
    ex = AttentionRolloutMedSigLIP(None, head_fusion="max", discard_ratio=0.5)
    got = ex._rollout([torch.from_numpy(a) for a in atts]).mean(dim=1).numpy()
    k = max(1, int(R.N * 0.5))
    exp = R.importance([R.layer_matrix(a, "max", k) for a in atts])
    assert _rel(got, exp) < 1e-6


def test_surface_is_the_references():
    assert xai.AttentionRolloutMedSigLIP is AttentionRolloutMedSigLIP
    assert list(inspect.signature(AttentionRolloutMedSigLIP.__init__).parameters) == [
        "self", "model", "head_fusion", "discard_ratio", "query_guided"]
    sig = inspect.signature(AttentionRolloutMedSigLIP.__init__).parameters
    assert (sig["head_fusion"].default, sig["discard_ratio"].default, sig["query_guided"].default) == ("mean", 0.9, True)
    assert list(inspect.signature(AttentionRolloutMedSigLIP.forward).parameters) == ["self", "query_tensor", "retrieved_tensor"]
    assert isinstance(inspect.getattr_static(AttentionRolloutMedSigLIP, "_fuse_heads"), staticmethod)
    ex = AttentionRolloutMedSigLIP(None)
    assert ex.last_native is False and ex.to("cpu") is ex


def test_ctypes_signatures_of_the_entry_points():
    import mirx._lib as L
    vp, i64, i, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert L.SYMBOLS["mirx_rollout_workspace_floats"] == (i64, [i, i64, i64])
    assert L.SYMBOLS["mirx_rollout_layer"] == (i, [vp, i64, i, i, i, f, i, i, i, i, vp, i64, vp])
    assert L.SYMBOLS["mirx_rollout_rows"] == (i, [vp, i64, i, i, vp])
    assert L.SYMBOLS["mirx_rollout_finish"] == (i, [vp, i64, i, i64, i, i, vp, vp, i64, i, i, vp, vp])
    assert L.ROLLOUT_FUSE == {"mean": 0, "max": 1, "min": 2}


def test_argument_checks_without_gpu():
    """Bad arguments are refused on the host before anything is launched (no device needed)."""
    import mirx._lib as L
    lib = L.load()
    n = 1024
    assert lib.mirx_rollout_workspace_floats(27, 1, n) == (27 + 4) * n * n + 17 * n      # + 4 n^2: the head splits
    assert lib.mirx_rollout_workspace_floats(27, 1, 1025) == -1
    assert lib.mirx_rollout_workspace_floats(0, 1, n) == -1
    buf = ctypes.c_void_p(16)                                      # never dereferenced: every call below fails its checks
    ws = lib.mirx_rollout_workspace_floats(2, 1, 16)
    bad = [dict(n=1025), dict(head_dim=74), dict(head_dim=132), dict(heads=0), dict(fusion=3), dict(k=17), dict(k=-1),
           dict(layer=2), dict(scale=float("nan")), dict(ws=ws - 1), dict(qkv=None)]
    for kw in bad:
        a = dict(qkv=buf, b=1, n=16, heads=2, head_dim=8, scale=0.5, fusion=0, k=8, layer=0, layers=2, ws=ws)
        a.update(kw)
        rc = lib.mirx_rollout_layer(a["qkv"], a["b"], a["n"], a["heads"], a["head_dim"], a["scale"], a["fusion"], a["k"],
                                    a["layer"], a["layers"], buf, a["ws"], None)
        assert rc == -1, kw
    assert lib.mirx_rollout_rows(buf, 4, 1025, 1, None) == -1
    assert lib.mirx_rollout_rows(buf, 4, 16, 17, None) == -1
    assert lib.mirx_rollout_rows(None, 4, 16, 1, None) == -1
    assert lib.mirx_rollout_finish(buf, ws, 2, 1, 4, 4, buf, None, 8, 10, 10, buf, None) == -1      # patches without query
    assert lib.mirx_rollout_finish(buf, ws - 1, 2, 1, 4, 4, None, None, 0, 10, 10, buf, None) == -1
    assert lib.mirx_rollout_finish(buf, ws, 2, 1, 4, 4, None, None, 0, 0, 10, buf, None) == -1
    assert lib.mirx_rollout_finish(buf, ws, 2, 1, 33, 32, None, None, 0, 10, 10, buf, None) == -1
