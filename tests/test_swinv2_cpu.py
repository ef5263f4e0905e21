"""SwinV2 (reference model.py:418-446): module tree, checkpoints, factory and the eager forward on the CPU, against
transformers.Swinv2Model (an independent implementation of the same network) and a float64 restatement."""
import re

import pytest
import torch

from _swinv2_ref import DEPTHS, embed, features, randomize

BACKBONE_PARAMS = 86_893_816


def _expected_keys(emb):
    """timm 0.9.7 parameter names of swinv2_base_window12to24_192to384 (PatchMerging at the start of stages 1-3)."""
    keys = ["swinv2.patch_embed.proj.weight", "swinv2.patch_embed.proj.bias", "swinv2.patch_embed.norm.weight",
            "swinv2.patch_embed.norm.bias"]
    for i, depth in enumerate(DEPTHS):
        if i > 0:
            keys += [f"swinv2.layers.{i}.downsample.reduction.weight", f"swinv2.layers.{i}.downsample.norm.weight",
                     f"swinv2.layers.{i}.downsample.norm.bias"]
        for j in range(depth):
            p = f"swinv2.layers.{i}.blocks.{j}."
            keys += [p + n for n in ("attn.logit_scale", "attn.q_bias", "attn.v_bias", "attn.cpb_mlp.0.weight", "attn.cpb_mlp.0.bias",
                                     "attn.cpb_mlp.2.weight", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias",
                                     "norm1.weight", "norm1.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                                     "mlp.fc2.bias", "norm2.weight", "norm2.bias")]
    keys += ["swinv2.norm.weight", "swinv2.norm.bias"]
    if emb:
        keys += ["fc.weight", "fc.bias"]
    return keys


@pytest.mark.parametrize("emb", [None, 512])
def test_state_dict_keys_and_parameter_count(emb):
    from mirx.model import SwinV2
    m = SwinV2(embedding_dim=emb)
    sd = m.state_dict()
    assert sorted(sd) == sorted(_expected_keys(emb))               # derived buffers are not persistent
    assert sum(p.numel() for n, p in m.named_parameters() if n.startswith("swinv2.")) == BACKBONE_PARAMS
    assert tuple(sd["swinv2.layers.0.blocks.0.attn.logit_scale"].shape) == (4, 1, 1)
    assert tuple(sd["swinv2.layers.3.blocks.1.attn.cpb_mlp.2.weight"].shape) == (32, 512)
    assert tuple(sd["swinv2.layers.2.downsample.reduction.weight"].shape) == (512, 1024)
    assert m.swinv2.num_features == 1024
    if emb:
        assert tuple(sd["fc.weight"].shape) == (emb, 1024)
    else:
        assert m.fc is None
    geo = [(blk.window, blk.shift) for layer in m.swinv2.layers for blk in layer.blocks]
    assert geo[:2] == [(24, 0), (24, 12)] and geo[2:4] == [(24, 0), (24, 12)]
    assert set(geo[4:22]) == {(24, 0)} and geo[22:] == [(12, 0), (12, 0)]


def _hf_model():
    from transformers import Swinv2Config, Swinv2Model
    cfg = Swinv2Config(image_size=384, patch_size=4, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=24,
                       pretrained_window_sizes=[12, 12, 12, 6])
    hf = Swinv2Model(cfg)
    assert (hf.config.image_size, hf.config.embed_dim, list(hf.config.depths), list(hf.config.num_heads), hf.config.window_size,
            list(hf.config.pretrained_window_sizes)) == (384, 128, [2, 2, 18, 2], [4, 8, 16, 32], 24, [12, 12, 12, 6])
    assert hf.num_features == 1024
    return hf


def _to_hf(sd):
    """timm-named state dict -> transformers Swinv2Model names (qkv split into query / key / value; timm's layers.i.downsample
    is transformers' layers.i-1.downsample)."""
    out = {}
    ren = [(r"^swinv2\.patch_embed\.proj\.", "embeddings.patch_embeddings.projection."), (r"^swinv2\.patch_embed\.norm\.", "embeddings.norm."),
           (r"^swinv2\.norm\.", "layernorm.")]
    blk = {"attn.logit_scale": "attention.self.logit_scale", "attn.cpb_mlp.": "attention.self.continuous_position_bias_mlp.",
           "attn.proj.": "attention.output.dense.", "norm1.": "layernorm_before.", "norm2.": "layernorm_after.",
           "mlp.fc1.": "intermediate.dense.", "mlp.fc2.": "output.dense."}
    for k, v in sd.items():
        if k.startswith("fc."):
            continue
        m = re.match(r"^swinv2\.layers\.(\d+)\.downsample\.(.*)$", k)
        if m:
            out[f"encoder.layers.{int(m.group(1)) - 1}.downsample.{m.group(2)}"] = v
            continue
        m = re.match(r"^swinv2\.layers\.(\d+)\.blocks\.(\d+)\.(.*)$", k)
        if m:
            p, rest = f"encoder.layers.{m.group(1)}.blocks.{m.group(2)}.", m.group(3)
            if rest == "attn.qkv.weight":
                q, kk, vv = v.chunk(3, 0)
                out[p + "attention.self.query.weight"], out[p + "attention.self.key.weight"] = q, kk
                out[p + "attention.self.value.weight"] = vv
            elif rest == "attn.q_bias":
                out[p + "attention.self.query.bias"] = v
            elif rest == "attn.v_bias":
                out[p + "attention.self.value.bias"] = v
            else:
                for a, b in blk.items():
                    if rest.startswith(a):
                        out[p + b + rest[len(a):]] = v
                        break
                else:
                    raise AssertionError(k)
            continue
        for a, b in ren:
            if re.match(a, k):
                out[re.sub(a, b, k)] = v
                break
        else:
            raise AssertionError(k)
    return out


@pytest.fixture(scope="module")
def random_model():
    from mirx.model import SwinV2
    torch.manual_seed(0)
    return randomize(SwinV2(), seed=1).double().eval()


@pytest.fixture(scope="module")
def image():
    return torch.randn(1, 3, 384, 384, generator=torch.Generator().manual_seed(2), dtype=torch.float64)


def test_eager_forward_matches_transformers(random_model, image):
    hf = _hf_model().double().eval()
    params = {n for n, _ in hf.named_parameters()}
    res = hf.load_state_dict(_to_hf(random_model.state_dict()), strict=False)
    assert not res.unexpected_keys
    assert not (set(res.missing_keys) & params)                   # every parameter came from the mapped state dict
    with torch.no_grad():
        ours = random_model.forward_eager(image)
        ref = hf(pixel_values=image).pooler_output
    assert ours.shape == ref.shape == (1, 1024)
    assert float((ours - ref).abs().max()) <= 1e-10


def test_eager_forward_matches_float64_restatement(random_model, image):
    with torch.no_grad():
        ours = random_model.forward_eager(image)
    assert float((ours - features(image, random_model.state_dict())).abs().max()) <= 1e-10


def test_forward_fc_and_size_check():
    from mirx.model import SwinV2
    m = randomize(SwinV2(embedding_dim=16), seed=3).eval()
    x = torch.randn(1, 3, 384, 384, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        y = m(x)
    ref = embed(x, m.state_dict())
    assert y.shape == (1, 16)
    assert float((y.double() - ref).abs().max()) <= 1e-4
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 352, 352))


def test_factory_and_checkpoint_wrappers():
    from mirx.model import SwinV2, build_model
    from mirx.retriever import MODEL_CONFIGS
    m, size = build_model("swinv2")
    assert isinstance(m, SwinV2) and size == 384 and m.fc is None
    m, _ = build_model("swinv2", embedding_dim=64)
    assert m.fc.out_features == 64
    assert "swinv2" not in MODEL_CONFIGS
    with pytest.raises(RuntimeError):
        SwinV2(pretrained=True)
    src = randomize(SwinV2(embedding_dim=8), seed=5)
    sd = src.state_dict()
    for wrap in ("state_dict", "state-dict"):
        dst = SwinV2(embedding_dim=8, weights={wrap: sd})
        for k, v in dst.state_dict().items():
            assert torch.equal(v, sd[k]), k
    # a checkpoint that also carries the derived buffers (timm versions that kept them) loads, and they are not read
    full = dict(sd)
    for name, buf in src.named_buffers():
        full[name] = torch.full_like(buf, 7) if buf.is_floating_point() else buf + 1
    dst = SwinV2(embedding_dim=8, weights=full)
    for (name, a), (_, b) in zip(dst.named_buffers(), src.named_buffers()):
        assert torch.equal(a, b), name
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    dst.load_state_dict(full)                                      # strict loading too


def test_get_model_and_transform():
    from mirx.model import SwinV2
    from mirx.retriever import get_model_and_transform
    m, tf = get_model_and_transform("swinv2", None, 128, "cpu")
    assert isinstance(m, SwinV2) and not m.training and m.fc.out_features == 128
    assert tuple(tf(__import__("PIL.Image", fromlist=["Image"]).new("RGB", (500, 400))).shape) == (3, 384, 384)
