"""ResNet50 (reference model.py:9-39): module tree, checkpoints, factory and the eager forward, on the CPU."""
import pytest
import torch

from oracle.densenet import randomize_bn_stats
from _resnet_ref import LAYERS, embed


def _expected_keys():
    """resnet50.* state-dict keys from torchvision's naming rule (Sequential children 0-8, Bottleneck names)."""
    def bn(p):
        return [f"{p}.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    keys = ["resnet50.0.weight"] + bn("resnet50.1")
    for li, nb in enumerate(LAYERS):
        for j in range(nb):
            p = f"resnet50.{4 + li}.{j}"
            for c in (1, 2, 3):
                keys += [f"{p}.conv{c}.weight"] + bn(f"{p}.bn{c}")
            if j == 0:
                keys += [f"{p}.downsample.0.weight"] + bn(f"{p}.downsample.1")
    return keys


def test_module_tree_matches_torchvision_names():
    from mirx.model import ResNet50
    m = ResNet50(embedding_dim=512)
    sd = m.state_dict()
    bb = [k for k in sd if k.startswith("resnet50.")]
    assert len(bb) == 318
    assert sorted(bb) == sorted(_expected_keys())
    assert "resnet50.4.0.downsample.0.weight" in sd and "resnet50.7.2.bn3.running_var" in sd
    assert sum(p.numel() for n, p in m.named_parameters() if n.startswith("resnet50.")) == 23_508_032
    assert tuple(sd["fc.weight"].shape) == (512, 2048)
    assert len(m.resnet50) == 9
    assert isinstance(m.resnet50[7][-1].conv3, torch.nn.Conv2d)        # the reference's Grad-CAM target
    assert m.resnet50[7][-1].conv3.out_channels == 2048
    assert ResNet50().fc is None and ResNet50(num_labels=3).classification_head.out_features == 3


def test_checkpoint_wrappers_round_trip():
    from mirx.model import ResNet50
    torch.manual_seed(0)
    src = ResNet50(embedding_dim=64)
    sd = randomize_bn_stats(src.state_dict(), seed=5)
    for wrap in ("state_dict", "state-dict"):
        dst = ResNet50(embedding_dim=64, weights={wrap: sd})
        for k, v in dst.state_dict().items():
            assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        ResNet50(pretrained=True)


def test_factory():
    from mirx.model import ResNet50, build_model
    m, size = build_model("resnet50")
    assert isinstance(m, ResNet50) and size == 224 and m.fc is None
    m, _ = build_model("resnet50", embedding_dim=128)
    assert m.fc.out_features == 128
    with pytest.raises(ValueError):
        build_model("convnextv2_sra")


@pytest.mark.parametrize("emb", [None, 32])
def test_eager_forward_matches_float64_restatement(emb):
    from mirx.model import ResNet50
    torch.manual_seed(1)
    m = ResNet50(embedding_dim=emb)
    m.load_state_dict(randomize_bn_stats(m.state_dict(), seed=2))
    m.eval()
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        y = m(x)
        u = m(((x - x.min()) / (x.max() - x.min()) * 255).round().to(torch.uint8))
    ref = embed(x, m.state_dict())
    assert y.shape == (2, emb or 2048)
    assert float((y.double() - ref).abs().max()) <= 1e-5
    assert torch.allclose(u.norm(dim=1), torch.ones(2), atol=1e-5)
