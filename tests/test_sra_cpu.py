"""ConvNeXtV2_SRA / ConvNeXtV2_PCAM on the CPU: the reference's module tree and state-dict keys, strict checkpoint round trips,
the eager heads against the fixture made by the reference's own SRA / PCAMPool (tests/golden/make_golden_sra.py), and the eager
models against the float64 restatement in _sra_ref."""
import os

import numpy as np
import pytest
import torch

from mirx.model import PCAMPool, SRA, ConvNeXtV2, ConvNeXtV2_PCAM, ConvNeXtV2_SRA, _LayerNorm2d
from _sra_ref import embed_pcam, embed_sra, pcam_head, randomize, sra_head

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sra_pcam_heads.npz")
HWS = ("12x12", "5x7")
LAMS = (0.1, 1.0)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def _norm(gold, dtype):
    ln = _LayerNorm2d(128, eps=1e-6).to(dtype)
    with torch.no_grad():
        ln.weight.copy_(_t(gold["norm_w"], dtype))
        ln.bias.copy_(_t(gold["norm_b"], dtype))
    return ln


def _sra(gold, k, lam, dtype):
    head = SRA(128, num_heads=k, lam=lam, norm_layer=_norm(gold, dtype)).to(dtype)
    with torch.no_grad():
        head.conv_att.weight.copy_(_t(gold[f"sra_w_k{k}"], dtype))
    return head


def _pcam(gold, k, lam, fc, dtype):
    head = PCAMPool(128, num_classes=k, lam=lam, norm_layer=_norm(gold, dtype), embedding_dim=32 if fc else None).to(dtype)
    with torch.no_grad():
        head.classifier.weight.copy_(_t(gold[f"pcam_w_k{k}"], dtype))
        head.classifier.bias.copy_(_t(gold[f"pcam_b_k{k}"], dtype))
        if fc:
            head.fc.weight.copy_(_t(gold["fc_w"], dtype))
            head.fc.bias.copy_(_t(gold["fc_b"], dtype))
    return head


def _backbone_keys():
    return {"convnext." + k for k in ConvNeXtV2().convnext.state_dict()}


def _nparams(m):
    return sum(p.numel() for p in m.parameters())


@pytest.mark.parametrize("k", [1, 8])
def test_sra_module_tree_and_keys(k):
    m = ConvNeXtV2_SRA(num_heads=k)
    keys = set(m.state_dict())
    assert keys == _backbone_keys() | {"sra.conv_att.weight", "sra.norm_layer.weight", "sra.norm_layer.bias"}
    assert m.sra.norm_layer is m.convnext.head.norm
    assert m.sra.conv_att.weight.shape == (k, 1024, 1, 1) and m.sra.conv_att.bias is None
    assert _nparams(m) == _nparams(ConvNeXtV2().convnext) + 1024 * k
    assert float(m.sra.conv_att.weight.detach().std()) < 1e-3           # normal(0, 1e-4), as the reference initialises it
    assert m.sra.lam == 0.1 and ConvNeXtV2_SRA().sra.num_heads == 8


@pytest.mark.parametrize("k,dim", [(3, None), (14, None), (3, 256)])
def test_pcam_module_tree_and_keys(k, dim):
    m = ConvNeXtV2_PCAM(num_classes=k, embedding_dim=dim)
    head = {"pcam.classifier.weight", "pcam.classifier.bias", "pcam.norm_layer.weight", "pcam.norm_layer.bias"}
    if dim:
        head |= {"pcam.fc.weight", "pcam.fc.bias"}
    assert set(m.state_dict()) == _backbone_keys() | head
    assert m.pcam.norm_layer is m.convnext.head.norm
    extra = 1024 * k + k + ((1024 + 1) * dim if dim else 0)
    assert _nparams(m) == _nparams(ConvNeXtV2().convnext) + extra
    assert ConvNeXtV2_PCAM().pcam.num_classes == 3 and ConvNeXtV2_PCAM().pcam.lam == 0.1


def test_pretrained_needs_local_weights():
    for cls in (ConvNeXtV2_SRA, ConvNeXtV2_PCAM):
        with pytest.raises(RuntimeError):
            cls(pretrained=True)


def test_strict_state_dict_round_trip(tmp_path):
    torch.manual_seed(0)
    x = torch.randn(1, 3, 64, 64)
    for make in (lambda: ConvNeXtV2_SRA(num_heads=4, lam=0.5), lambda: ConvNeXtV2_PCAM(num_classes=3, embedding_dim=16)):
        a = randomize(make(), seed=1).eval()
        b = make().eval()
        b.load_state_dict(a.state_dict(), strict=True)
        with torch.no_grad():
            assert torch.equal(a(x), b(x))
        path = str(tmp_path / "ckpt.pt")
        torch.save({"state_dict": a.state_dict()}, path)
        if isinstance(a, ConvNeXtV2_SRA):
            c = ConvNeXtV2_SRA(pretrained=True, num_heads=4, lam=0.5, weights=path).eval()
        else:
            c = ConvNeXtV2_PCAM(pretrained=True, num_classes=3, embedding_dim=16, weights=path).eval()
        with torch.no_grad():
            assert torch.equal(a(x), c(x))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-12)])
def test_eager_sra_matches_reference_fixture(gold, dtype, tol):
    for hw in HWS:
        x = _t(gold[f"x_{hw}"], dtype)
        for k in (1, 8):
            for lam in LAMS:
                want = torch.from_numpy(gold[f"sra_{hw}_k{k}_l{round(10 * lam)}"])
                with torch.no_grad():
                    got = _sra(gold, k, lam, dtype)(x).double()
                assert float((got - want).abs().max()) <= tol * float(want.abs().max()), (hw, k, lam)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-12)])
def test_eager_pcam_matches_reference_fixture(gold, dtype, tol):
    for hw in HWS:
        x = _t(gold[f"x_{hw}"], dtype)
        for k in (3, 14):
            for lam in LAMS:
                for fc in (0, 1):
                    p = f"pcam_{hw}_k{k}_l{round(10 * lam)}_fc{fc}_"
                    with torch.no_grad():
                        got = _pcam(gold, k, lam, fc, dtype)(x)
                    for g, name in zip(got, ("embedding", "class_logits", "pcam_probs")):
                        want = torch.from_numpy(gold[p + name])
                        assert g.shape == want.shape
                        assert float((g.double() - want).abs().max()) <= tol * max(1.0, float(want.abs().max())), (p, name)


def test_float64_restatement_matches_reference_fixture(gold):
    """_sra_ref's heads (the GPU tests' yardstick) against the reference's own outputs."""
    nw, nb = _t(gold["norm_w"], torch.float64), _t(gold["norm_b"], torch.float64)
    for hw in HWS:
        x = _t(gold[f"x_{hw}"], torch.float64)
        for k in (1, 8):
            for lam in LAMS:
                got = sra_head(x, _t(gold[f"sra_w_k{k}"], torch.float64), nw, nb, lam)
                assert torch.allclose(got, torch.from_numpy(gold[f"sra_{hw}_k{k}_l{round(10 * lam)}"]), rtol=0, atol=1e-12)
        for k in (3, 14):
            for lam in LAMS:
                for fc in (0, 1):
                    p = f"pcam_{hw}_k{k}_l{round(10 * lam)}_fc{fc}_"
                    fw = _t(gold["fc_w"], torch.float64) if fc else None
                    fb = _t(gold["fc_b"], torch.float64) if fc else None
                    emb, logits, probs, _ = pcam_head(x, _t(gold[f"pcam_w_k{k}"], torch.float64), _t(gold[f"pcam_b_k{k}"], torch.float64),
                                                      nw, nb, lam, fw, fb)
                    for g, name in zip((emb, logits, probs), ("embedding", "class_logits", "pcam_probs")):
                        assert torch.allclose(g, torch.from_numpy(gold[p + name]), rtol=0, atol=1e-12), (p, name)


def test_pcam_training_mode_returns_the_reference_dict(gold):
    k, lam = 14, 1.0
    m = ConvNeXtV2_PCAM(num_classes=k, lam=lam, embedding_dim=32)
    m.pcam = _pcam(gold, k, lam, 1, torch.float32)
    m.convnext.forward_features = lambda x: x                   # feed the fixture's pre-pool map straight into the head
    m.train()
    out = m(_t(gold["x_12x12"], torch.float32))
    assert set(out) == {"embedding", "class_logits", "pcam_maps"}
    p = f"pcam_12x12_k{k}_l10_fc1_"
    for key, name in (("embedding", "embedding"), ("class_logits", "class_logits"), ("pcam_maps", "pcam_probs")):
        want = torch.from_numpy(gold[p + name])
        assert float((out[key].detach().double() - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max())), key
    assert out["class_logits"].requires_grad                     # the training path keeps autograd
    m.eval()
    with torch.no_grad():
        e = m(_t(gold["x_12x12"], torch.float32))
    assert torch.is_tensor(e) and e.shape == (2, 32)


@pytest.mark.parametrize("size", [(64, 64), (96, 64)])
def test_eager_models_match_float64_restatement(size):
    x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(sum(size)), dtype=torch.float64)
    sra = randomize(ConvNeXtV2_SRA(num_heads=8, lam=0.7), seed=3).double().eval()
    pcam = randomize(ConvNeXtV2_PCAM(num_classes=3, lam=0.7, embedding_dim=48), seed=4).double().eval()
    with torch.no_grad():
        a, b = sra(x), pcam(x)
    assert a.shape == (2, 1024) and b.shape == (2, 48)
    assert float((a - embed_sra(x, sra.state_dict(), 0.7)).abs().max()) <= 1e-10
    assert float((b - embed_pcam(x, pcam.state_dict(), 0.7)).abs().max()) <= 1e-10


def test_lam_zero_is_convnextv2():
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    sra = randomize(ConvNeXtV2_SRA(num_heads=8, lam=0.0), seed=6).eval()
    base = ConvNeXtV2().eval()
    base.load_state_dict({k: v for k, v in sra.state_dict().items() if k.startswith("convnext.")}, strict=True)
    with torch.no_grad():
        assert torch.allclose(sra(x), base(x), rtol=0, atol=1e-7)


def test_factory_still_points_at_the_class():
    from mirx.model import build_model
    with pytest.raises(ValueError, match="ConvNeXtV2_SRA"):
        build_model("convnextv2_sra")


def test_native_head_limits_match_the_header():
    """The model takes the eager head outside the kernel's documented limits (include/mirx.h)."""
    import re
    from mirx.model import ATTNPOOL_LDS_FLOATS, ATTNPOOL_MAX_C, ATTNPOOL_MAX_K, _attnpool_ok
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mirx.h")).read()
    for name, val in (("MAX_C", ATTNPOOL_MAX_C), ("MAX_K", ATTNPOOL_MAX_K), ("LDS_FLOATS", ATTNPOOL_LDS_FLOATS)):
        assert int(re.search(r"#define MIRX_ATTNPOOL_%s (\d+)" % name, hdr).group(1)) == val
    assert _attnpool_ok(1024, 8, 144) and _attnpool_ok(1024, 64, 244) and _attnpool_ok(8192, 1, 1)
    assert not _attnpool_ok(1024, 64, 245) and not _attnpool_ok(1024, 65, 1) and not _attnpool_ok(1024, 0, 1)
    assert not _attnpool_ok(1022, 8, 144) and not _attnpool_ok(8196, 8, 144) and not _attnpool_ok(1024, 8, 0)
