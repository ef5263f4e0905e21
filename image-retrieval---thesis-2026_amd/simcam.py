"""SimCAM: gradient-free similarity saliency for the retrieval backbones.

Mirrors (paths into the reference tree):
  SimCAM_Densenet121   explanations.py:664-750   (compute_saliency.py:194-199)
  SimCAM               explanations.py:753-900   (compute_saliency.py:201-217, compute_saliency_convnextv2.py:138-141)
  SimCAM_MedSigLIP     explanations.py:903-976   (compute_saliency.py:218-220)

For a query feature map Q and a retrieved one R (rows [h * w, C], one per position) the decomposition is D = Q R^T; with
s = max(D) + eps the query map is sum_j relu(D[i, j] / s), the retrieved map sum_i relu(D[i, j] / s) (or, with a point, the
bilinear blend of the rows relu(D[i*, :] / s) at the point), both upsampled bilinearly to the input size.

Native path: CUDA fp32 input, the model in eval mode, and (model, target) one of the reference drivers' configurations on a
mirx model -- DenseNet121's feature stack with target "relu", ResNet50 with resnet50[7][-1], a ConvNeXtV2 backbone (ConvNeXtV2,
_SRA, _PCAM share it) with stages[3].blocks[-1], MedSigLIP with backbone.post_layernorm.  The feature map then comes from the
embedder's own kernels (the module forwards a hook would need are bypassed there) and the decomposition, normalisation, sums,
point blend and upsample from one mirx_simcam call (k_simcam.hip), written into the returned tensor.  Everywhere else the
reference's formulas run in torch on a forward hook, as there, including its failures.  `last_native` tells which path ran.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .model import (DenseNet121, MedSigLIP, ResNet50, _cfg, _ConvNeXtV2Backbone, _linear_auto, _linear_s3_ok, _ptr,
                    _stream)

EPS = 1e-8                     # SimCAM / SimCAM_MedSigLIP: D / (max(D) + 1e-8); SimCAM_Densenet121 divides by max(D)
SIMCAM_MAX_HW = 1024           # include/mirx.h MIRX_SIMCAM_MAX_HW: positions per feature map the kernel takes
WORKSPACE_FLOATS = 1 << 26     # workspace per mirx_simcam call (256 MB): the pairs are chunked to fit


# ---- the kernel -------------------------------------------------------------------------------------------------------
def simcam_maps(q, r, h, w, size, eps=EPS, maps="both", point=None, out=None):
    """[HIP] mirx_simcam: q [h * w, C] query rows, r [P, h * w, C] retrieved rows (CUDA fp32), size = (H, W).
    maps="both" -> [P, 2, H, W] (query map, retrieved map); "retrieved" -> [P, H, W].  point: (along H, along W) or None."""
    if maps not in ("both", "retrieved"):
        raise ValueError(f"maps must be 'both' or 'retrieved', got {maps!r}")
    H, W = int(size[0]), int(size[1])
    if q.dim() != 2 or r.dim() != 3 or r.shape[1:] != q.shape or q.shape[0] != h * w:
        raise ValueError(f"simcam_maps: q must be [h * w, C] and r [P, h * w, C] (got {tuple(q.shape)}, {tuple(r.shape)}, "
                         f"h x w = {h} x {w})")
    if not (q.is_cuda and r.is_cuda and q.dtype == torch.float32 and r.dtype == torch.float32 and q.device == r.device):
        raise ValueError("simcam_maps: q and r must be float32 tensors on one CUDA device")
    lib = _lib.load()
    q = q.contiguous()
    r = r.contiguous()
    p_all = r.shape[0]
    shape = (p_all, 2, H, W) if maps == "both" else (p_all, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q.device:
        raise ValueError(f"simcam_maps: out must be a contiguous float32 {shape} tensor on {q.device}")
    pt = None if point is None else (ctypes.c_double * 2)(float(point[0]), float(point[1]))
    mode = _lib.SIMCAM_MAPS_BOTH if maps == "both" else _lib.SIMCAM_MAPS_RETRIEVED
    per_pair = lib.mirx_simcam_workspace_floats(1, h * w)
    if per_pair < 0:
        _lib.check(int(per_pair), "mirx_simcam_workspace_floats")
    # pairs per call: the grid limit, and a workspace of at most WORKSPACE_FLOATS (pair p's maps do not depend on the chunk)
    chunk = max(1, min(65535, WORKSPACE_FLOATS // per_pair))
    with torch.cuda.device(q.device):
        ws = torch.empty((per_pair * max(1, min(chunk, p_all)),), dtype=torch.float32, device=q.device)
        for p0 in range(0, max(p_all, 1), chunk):
            n = min(chunk, p_all - p0)
            rr = r[p0:p0 + n]
            _lib.check(lib.mirx_simcam(_ptr(q), _ptr(rr) if n else None, n, h * w * q.shape[1], h, w, q.shape[1], float(eps), mode,
                                       pt, H, W, _ptr(ws), ws.numel(), _ptr(out[p0:p0 + n]) if n else None, _stream(q.device)),
                       "mirx_simcam")
    return out


# ---- shared pieces of the reference's formulas ------------------------------------------------------------------------
def _check_point(point, H, W):
    if point is None:
        return
    if len(point) != 2:
        raise ValueError(f"point must be (along H, along W), got {point!r}")
    p0, p1 = float(point[0]), float(point[1])
    if not (0.0 <= p0 < H and 0.0 <= p1 < W):
        raise ValueError(f"point {tuple(point)} lies outside the {H} x {W} image")


def _point_specific(decom, point, size):
    """explanations.py Point_Specific: decom [h, w, h, w] (query position first) -> the retrieved map at the query point,
    a bilinear blend of four rows of the replicate-padded query grid, clamped at 0."""
    pad = F.pad(decom.permute(2, 3, 0, 1), (1, 1, 1, 1), mode="replicate").permute(2, 3, 0, 1)
    x = (point[0] + 0.5) / size[0] * (pad.shape[0] - 2) + 0.5
    y = (point[1] + 0.5) / size[1] * (pad.shape[1] - 2) + 0.5
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    dx, dy = x - x0, y - y0
    blend = (pad[x0, y0] * (1 - dx) * (1 - dy) + pad[x0 + 1, y0] * dx * (1 - dy) + pad[x0, y0 + 1] * (1 - dx) * dy
             + pad[x0 + 1, y0 + 1] * dx * dy)
    return blend.clamp(min=0)


class _TokenFc:
    """The reference's per-position fc, tokens @ W^T + b / (h * w), as a Linear view for _linear_auto (the project's Linear)."""

    def __init__(self, fc, hw):
        self.weight = fc.weight
        self.bias = fc.bias.detach() / hw if fc.bias is not None else None
        self.in_features, self.out_features = fc.in_features, fc.out_features
        self.__dict__["_mirx_cfg"] = _cfg(fc)

    def __call__(self, x):
        return F.linear(x, self.weight, self.bias)


def _token_fc(owner, fc, rows, hw):
    key = (id(fc), hw, fc.weight.data_ptr(), fc.weight._version, None if fc.bias is None else (fc.bias.data_ptr(), fc.bias._version))
    view = owner.__dict__.get("_mirx_token_fc")
    if view is None or view[0] != key:
        view = (key, _TokenFc(fc, hw))
        owner.__dict__["_mirx_token_fc"] = view
    return _linear_auto(view[1], rows)


def _fc_ok(fc, c, x):
    """The per-position fc can run on the project's Linear for c-channel features of the CUDA batch x (checked before the
    feature forward runs)."""
    return fc is None or (isinstance(fc, nn.Linear) and fc.in_features == c and fc.weight.device == x.device
                          and fc.weight.dtype == torch.float32 and (fc.bias is None or fc.bias.dtype == torch.float32)
                          and _linear_s3_ok(fc, x))


def _cuda_f32(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and 1 <= x.shape[0] <= 65535


# ---- the native taps: (model, target) -> (a function x -> (rows [B, h * w, C], h, w), C), or None ---------------------
def _convnext_of(model):
    if isinstance(model, _ConvNeXtV2Backbone):
        return model
    b = getattr(model, "convnext", None)
    return b if isinstance(b, _ConvNeXtV2Backbone) else None


def _simcam_tap(model, target, x):
    if not _cuda_f32(x) or model.training:
        return None
    if isinstance(model, ResNet50) and target is model.resnet50[7][-1]:
        if not ResNet50._native_size_ok(x) or model.resnet50.training:
            return None
        return (lambda t: model._layer4_rows(t, model._cache())), target.bn3.num_features
    cnx = _convnext_of(model)
    if cnx is not None and target is cnx.stages[3].blocks[-1] and not cnx.training and cnx._nhwc_ok(x):
        def tap(t):
            rows, h, w = cnx._forward_rows(t.contiguous())
            return rows.view(t.shape[0], h * w, rows.shape[-1]), h, w
        return tap, cnx.num_features
    return None


def _densenet_owner(model, feature_module, target_layers):
    ref = feature_module.__dict__.get("_mirx_owner")
    owner = ref() if ref is not None else None
    if not isinstance(owner, DenseNet121) or owner.densenet121[0] is not feature_module:
        return None
    if not any(m is feature_module for m in model._modules.values()) or "relu" not in target_layers:
        return None
    return owner


# ---- the explainers ---------------------------------------------------------------------------------------------------
class SimCAM(nn.Module):
    """explanations.py SimCAM(model, target_layer, fc=None)(x_q, x, point=None) -> [B - 1, 2, H, W]: row 0 of cat(x_q, x) is
    the query, every other row a retrieval; per retrieval the query map and the retrieved (or point-specific) map."""

    def __init__(self, model, target_layer, fc=None):
        super().__init__()
        self.model = model
        self.target_layer = target_layer
        self.fc = fc
        self.last_native = False

    def Point_Specific(self, decom, point=[0, 0], size=(224, 224)):  # noqa: B006 (the reference's signature)
        return _point_specific(decom, point, size)

    def forward(self, x_q, x, point=None):
        _, _, H, W = x_q.size()
        _check_point(point, H, W)
        x_all = torch.cat((x_q, x), dim=0)
        with torch.no_grad():                           # (the backbones' native gates read the grad mode)
            tap = _simcam_tap(self.model, self.target_layer, x_all)
            native = tap is not None and x_all.shape[0] >= 2 and _fc_ok(self.fc, tap[1], x_all)
        if native:
            with torch.no_grad(), torch.cuda.device(x_all.device):
                rows, h, w = tap[0](x_all)
                if self.fc is not None:
                    rows = _token_fc(self, self.fc, rows, h * w)
                self.last_native = True
                return simcam_maps(rows[0], rows[1:], h, w, (H, W), EPS, "both", point)
        self.last_native = False
        return self._forward_torch(x_all, H, W, point)

    def _forward_torch(self, x_all, H, W, point):
        feats = []
        handle = self.target_layer.register_forward_hook(lambda m, i, o: feats.append(o))
        with torch.no_grad():
            self.model(x_all)
            handle.remove()
            if len(feats) == 0:
                raise RuntimeError("SimCAM hook failed: no features captured.")
            fmap = feats[0]
            B, C, h, w = fmap.shape
            assert B >= 2, "Need at least 1 query + 1 retrieval image"
            tokens = fmap.permute(0, 2, 3, 1).reshape(B, h * w, C)
            q, r = tokens[0:1], tokens[1:]
            if self.fc is not None:
                wt, b = self.fc.weight.data.t(), self.fc.bias.data
                q = q @ wt + b / (h * w)
                r = r @ wt + b / (h * w)
            D = torch.matmul(q.expand(r.shape[0], -1, -1), r.transpose(1, 2))
            D = (D / (D.amax(dim=(1, 2), keepdim=True) + EPS)).clamp(min=0).view(r.shape[0], h, w, h, w)
            decom_1 = D.sum(dim=(3, 4))
            if point is not None:
                decom_2 = torch.stack([_point_specific(D[n], point, (H, W)) for n in range(D.shape[0])], dim=0)
            else:
                decom_2 = D.sum(dim=(1, 2))
            return F.interpolate(torch.stack((decom_1, decom_2), dim=1), size=(H, W), mode="bilinear", align_corners=False)


class SimCAM_Densenet121(nn.Module):
    """explanations.py SimCAM_Densenet121(model, feature_module, target_layers, fc=None)(x_q, x, point=None) -> [2, H, W]:
    images 0 and 1 of cat(x_q, x), the feature map the last of `target_layers` inside `feature_module`, normalised by max(D)
    without eps (an all-zero map gives NaN, as there).  The reference's per-call debug print is not reproduced."""

    def __init__(self, model, feature_module, target_layers, fc=None):
        super().__init__()
        self.model = model
        self.feature_module = feature_module
        self.target_layers = target_layers
        self.fc = fc
        self.last_native = False

    def Point_Specific(self, decom, point=[0, 0], size=(224, 224)):  # noqa: B006
        return _point_specific(decom, point, size)

    def forward(self, x_q, x, point=None):
        _, _, H, W = x_q.size()
        _check_point(point, H, W)
        x_all = torch.cat((x_q, x))
        owner = _densenet_owner(self.model, self.feature_module, self.target_layers)
        with torch.no_grad():
            native = (owner is not None and _cuda_f32(x_all) and x_all.shape[0] >= 2 and not self.model.training
                      and not self.feature_module.training
                      and _fc_ok(self.fc, self.feature_module.norm5.num_features, x_all))
        if native:
            with torch.no_grad(), torch.cuda.device(x_all.device):
                rows, h, w = owner._relu_rows(x_all[:2], owner._cache())    # only images 0 and 1 enter the maps
                if self.fc is not None:
                    rows = _token_fc(self, self.fc, rows, h * w)
                self.last_native = True
                return simcam_maps(rows[0], rows[1:2], h, w, (H, W), 0.0, "both", point).view(2, H, W)
        self.last_native = False
        return self._forward_torch(x_all, H, W, point)

    def _activations(self, x):
        """gradcam.py ModelOutputs without its print: the outputs of `target_layers` inside the feature module."""
        acts = []
        for module in self.model._modules.values():
            if module is self.feature_module:
                for name, sub in module._modules.items():
                    x = sub(x)
                    if name in self.target_layers:
                        acts.append(x)
            elif isinstance(module, nn.AdaptiveAvgPool2d):
                x = module(x).view(x.size(0), -1)
            else:
                x = module(x)
        return acts

    def _forward_torch(self, x_all, H, W, point):
        with torch.no_grad():
            A = self._activations(x_all)
            x = A[-1].permute(0, 2, 3, 1)
            if self.fc is not None:
                x = torch.matmul(x, self.fc.weight.data.transpose(1, 0)) + self.fc.bias.data / (x.shape[1] * x.shape[2])
            h, w = x.shape[1], x.shape[2]
            # the reference fills a zeros([h, w, h, w]) tensor (default dtype) with sum(x[0, i, j] * x[1, k, l])
            D = torch.matmul(x[0].reshape(h * w, -1), x[1].reshape(h * w, -1).t()).to(torch.get_default_dtype())
            D = (D / torch.max(D)).clamp(min=0).view(h, w, h, w)
            decom_1 = torch.sum(D, dim=(2, 3))
            decom_2 = _point_specific(D, point, (H, W)) if point is not None else torch.sum(D, dim=(0, 1))
            return F.interpolate(torch.stack((decom_1, decom_2)).unsqueeze(1), size=(H, W), mode="bilinear").squeeze(1)


class SimCAM_MedSigLIP(nn.Module):
    """explanations.py SimCAM_MedSigLIP(model, target_layer)(x_q, x) -> [K, H, W]: the retrieved maps of K retrievals against
    one query (x_q must have batch 1), on the tokens of `target_layer` (a square grid)."""

    def __init__(self, model, target_layer):
        super().__init__()
        self.model = model
        self.target_layer = target_layer
        self.last_native = False

    def _native_ok(self, x_all):
        m = self.model
        if not (isinstance(m, MedSigLIP) and self.target_layer is m.backbone.post_layernorm and _cuda_f32(x_all)
                and not m.training and not m.backbone.training):
            return False
        cfg = m.backbone.config
        side = x_all.shape[-1] // cfg.patch_size
        return (x_all.shape[-2] // cfg.patch_size) * side <= SIMCAM_MAX_HW

    def forward(self, x_q, x):
        assert x_q.shape[0] == 1, "x_q must be batch size 1"
        _, _, H, W = x_q.shape
        x_all = torch.cat([x_q, x], dim=0)
        if self._native_ok(x_all):
            with torch.no_grad(), torch.cuda.device(x_all.device):
                tokens = self.model.backbone.last_hidden_state(x_all)
                n = tokens.shape[1]
                grid = int(np.sqrt(n))
                assert grid * grid == n, f"num_patches={n} is not square"
                self.last_native = True
                return simcam_maps(tokens[0], tokens[1:], grid, grid, (H, W), EPS, "retrieved")
        self.last_native = False
        return self._forward_torch(x_all, H, W)

    def _forward_torch(self, x_all, H, W):
        feats = []
        handle = self.target_layer.register_forward_hook(lambda m, i, o: feats.append(o))
        with torch.no_grad():
            self.model.backbone(pixel_values=x_all)
            handle.remove()
            if len(feats) == 0:
                raise RuntimeError("Hook did not capture anything")
            tokens = feats[0]
            if isinstance(tokens, (tuple, list)):
                tokens = tokens[0]
            if tokens.dim() != 3:
                raise RuntimeError(f"Expected tokens [B,N,D], got {tokens.shape}")
            n = tokens.shape[1]
            grid = int(np.sqrt(n))
            assert grid * grid == n, f"num_patches={n} is not square"
            q, r = tokens[0:1], tokens[1:]
            sim = torch.matmul(q.expand(r.size(0), -1, -1), r.transpose(1, 2))
            sim = (sim / (sim.amax(dim=(1, 2), keepdim=True) + EPS)).clamp(min=0).view(r.size(0), grid, grid, grid, grid)
            maps = sim.sum(dim=(1, 2))
            return F.interpolate(maps.unsqueeze(1), size=(H, W), mode="bilinear", align_corners=False).squeeze(1)

