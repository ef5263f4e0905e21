#!/usr/bin/env python3
"""Generate the SRA / PCAM head fixture from the reference's OWN head classes.

Run in the build container only (the reference tree is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sra.py

What it does
  * imports the reference's model.py (SRA, model.py:120-164; PCAMPool, model.py:199-257) from the reference tree.  model.py
    imports torchvision and timm at module import time although neither head uses them, so inert placeholder modules are
    registered for those names first (the make_golden.py recipe).  Nothing of the reference is copied: only INPUTS and the
    reference's OUTPUTS are written.
  * uses timm's LayerNorm2d formula (a LayerNorm over the channel axis of an NCHW map, eps 1e-6) as `norm_layer`, as
    ConvNeXtV2_SRA / ConvNeXtV2_PCAM pass convnext.head.norm.
  * runs both heads in float64 on seeded float32 inputs and weights, with weights large enough that the attention maps are far
    from uniform, and stores inputs, weights and outputs as tests/golden/sra_pcam_heads.npz:
        x_12x12, x_5x7              [2, 128, h, w] float32 pre-pool maps
        norm_w, norm_b              [128] float32 LayerNorm2d affine
        sra_w_k{K}                  [K, 128, 1, 1] float32 conv_att, K in (1, 8)
        pcam_w_k{K}, pcam_b_k{K}    [K, 128, 1, 1], [K] float32 classifier, K in (3, 14)
        fc_w, fc_b                  [32, 128], [32] float32 PCAM fc (embedding_dim 32)
        sra_{hw}_k{K}_l{L}          [2, 128] float64 SRA output (before the model's F.normalize); L = 10 lam
        pcam_{hw}_k{K}_l{L}_fc{F}_{embedding,class_logits,pcam_probs}   float64 PCAMPool outputs; F = 0 / 1 (no fc / fc)
"""
import importlib
import os
import sys
import types

import numpy as np

REF = os.environ.get("MIRX_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
C = 128
HWS = {"12x12": (12, 12), "5x7": (5, 7)}
LAMS = (0.1, 1.0)


def import_reference_model():
    import torch  # noqa: F401
    import transformers  # noqa: F401  (must be imported before the placeholders exist)

    class _Anything:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return self

        def __getattr__(self, k):
            return _Anything()

    for name in ("torchvision", "torchvision.models", "torchvision.transforms", "timm"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []

            def _ga(k, _A=_Anything):
                if k.startswith("__"):
                    raise AttributeError(k)
                return _A()
            m.__getattr__ = _ga  # type: ignore[attr-defined]
            sys.modules[name] = m
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.path.insert(0, REF)
    return importlib.import_module("model")


def main():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class LayerNorm2d(nn.LayerNorm):        # timm.layers.LayerNorm2d: LayerNorm over C of an NCHW map
        def forward(self, x):
            return F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps).permute(0, 3, 1, 2)

    ref = import_reference_model()
    g = torch.Generator().manual_seed(2026)
    out = {}
    for key, (h, w) in HWS.items():
        out[f"x_{key}"] = (torch.randn(2, C, h, w, generator=g) + 0.3 * torch.randn(2, C, 1, 1, generator=g)).numpy()
    out["norm_w"] = (0.5 + torch.rand(C, generator=g)).numpy()
    out["norm_b"] = (0.1 * torch.randn(C, generator=g)).numpy()
    for k in (1, 8):
        out[f"sra_w_k{k}"] = (0.3 * torch.randn(k, C, 1, 1, generator=g)).numpy()
    for k in (3, 14):
        out[f"pcam_w_k{k}"] = (0.2 * torch.randn(k, C, 1, 1, generator=g)).numpy()
        out[f"pcam_b_k{k}"] = (0.5 * torch.randn(k, generator=g)).numpy()
    out["fc_w"] = (torch.randn(32, C, generator=g) / C ** 0.5).numpy()
    out["fc_b"] = (0.1 * torch.randn(32, generator=g)).numpy()

    def norm():
        ln = LayerNorm2d(C, eps=1e-6)
        ln.weight.data = torch.from_numpy(out["norm_w"]).double()
        ln.bias.data = torch.from_numpy(out["norm_b"]).double()
        return ln.double()

    with torch.no_grad():
        for key in HWS:
            x = torch.from_numpy(out[f"x_{key}"]).double()
            for k in (1, 8):
                for lam in LAMS:
                    head = ref.SRA(C, num_heads=k, lam=lam, norm_layer=norm()).double()
                    head.conv_att.weight.data = torch.from_numpy(out[f"sra_w_k{k}"]).double()
                    out[f"sra_{key}_k{k}_l{round(10 * lam)}"] = head(x).numpy()
            for k in (3, 14):
                for lam in LAMS:
                    for fc in (0, 1):
                        head = ref.PCAMPool(C, num_classes=k, lam=lam, norm_layer=norm(), embedding_dim=32 if fc else None).double()
                        head.classifier.weight.data = torch.from_numpy(out[f"pcam_w_k{k}"]).double()
                        head.classifier.bias.data = torch.from_numpy(out[f"pcam_b_k{k}"]).double()
                        if fc:
                            head.fc.weight.data = torch.from_numpy(out["fc_w"]).double()
                            head.fc.bias.data = torch.from_numpy(out["fc_b"]).double()
                        emb, logits, probs = head(x)
                        p = f"pcam_{key}_k{k}_l{round(10 * lam)}_fc{fc}_"
                        out[p + "embedding"], out[p + "class_logits"], out[p + "pcam_probs"] = emb.numpy(), logits.numpy(), probs.numpy()
            # the attention must be far from uniform for the fixture to pin the branch
            att = torch.softmax(F.conv2d(x, torch.from_numpy(out["sra_w_k8"]).double()).flatten(2), dim=2)
            assert float(att.max()) > 20.0 / x[0, 0].numel(), float(att.max())
    path = os.path.join(OUT, "sra_pcam_heads.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
