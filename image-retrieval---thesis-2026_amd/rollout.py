"""Attention rollout saliency for MedSigLIP.

Mirrors (paths into the reference tree):
  AttentionRolloutMedSigLIP   explanations.py:979-1147   (evaluate_test_dataset_milvus.py:413-423, evaluate_single_image.py:320-330)

Per layer the attention probabilities are fused over the heads (mean / max / min), the entries at or below each row's k-th
smallest value dropped (k = max(1, int(N * discard_ratio)), when discard_ratio > 0), the identity added and the rows
normalised by (row sum + 1e-8); the rollout is the product A_{L-1} ... A_0, and the importance of patch j its mean over rows,
optionally times clamp(cos(patch j, query embedding), 0); the grid map is upsampled bilinearly to the input size.

Native path: CUDA fp32 inputs, a mirx MedSigLIP in eval mode, head_fusion mean / max / min, 1 <= k <= N when discarding, N and
head_dim within k_rollout.hip's limits and every encoder layer on its native path.  The importance needs only the mean over
rows, (1/N) 1^T A_{L-1} ... A_0, so a vector is walked from the last layer to the first (N^2 per layer, not N^3).  Each
layer's A_l comes from mirx_rollout_layer on the packed qkv the native encoder layer computes (SiglipVisionTower
._hidden_tapped), launched on a side stream so that it overlaps the next layers of the forward; the chain, the query
weighting and the upsample come from mirx_rollout_finish; the patch projection runs on the project's Linear, LayerNorm and
row-normalise kernels.  Everywhere else the reference's formulas run in torch on backbone(output_attentions=True), as there,
including its failures.  `last_native` tells which path ran.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .model import MedSigLIP, _layernorm, _linear_auto, _linear_s3_ok, _normalize_rows, _ptr, _stream

ROLLOUT_MAX_N = 1024             # include/mirx.h MIRX_ROLLOUT_MAX_N
ROLLOUT_MAX_HEAD_DIM = 128       # MIRX_ROLLOUT_MAX_HEAD_DIM (a multiple of 4)
ROLLOUT_MAX_HEADS = 256
WORKSPACE_FLOATS = 1 << 28       # workspace per chunk of retrieved images (1 GiB; 130 MB per image at 448 x 448, 27 layers)


def _check_f32(x, what):
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor")


# ---- the kernels ------------------------------------------------------------------------------------------------------
def rollout_rows_(a, k):
    """[HIP] mirx_rollout_rows in place on a [rows, n] fp32 CUDA matrix: k > 0 -> a * (a > k-th smallest of the row); then
    + 1 at column row % n and / (row sum + 1e-8).  k = 0: no discard."""
    _check_f32(a, "rollout_rows_: a")
    if a.dim() != 2:
        raise ValueError("rollout_rows_: a must be [rows, n]")
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().mirx_rollout_rows(_ptr(a), a.shape[0], a.shape[1], int(k), _stream(a.device)), "mirx_rollout_rows")
    return a


def workspace_floats(layers, b, n):
    v = int(_lib.load().mirx_rollout_workspace_floats(int(layers), int(b), int(n)))
    if v < 0:
        _lib.check(v, "mirx_rollout_workspace_floats")
    return v


def _check_ws(ws, dev, what):
    _check_f32(ws, f"{what}: ws")
    if ws.dim() != 1 or ws.device != dev:
        raise ValueError(f"{what}: ws must be a flat float32 tensor on {dev}")


def rollout_layer(qkv, heads, scale, fusion, k, layer, layers, ws):
    """[HIP] mirx_rollout_layer: qkv [b, n, 3c] (c = heads * head_dim) -> A_layer of every image into workspace slot `layer`."""
    _check_f32(qkv, "rollout_layer: qkv")
    if qkv.dim() != 3 or int(heads) < 1 or qkv.shape[2] % (3 * int(heads)) != 0:
        raise ValueError(f"rollout_layer: qkv must be [b, n, 3 * heads * head_dim] (got {tuple(qkv.shape)}, heads = {heads})")
    _check_ws(ws, qkv.device, "rollout_layer")
    b, n, c3 = qkv.shape
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.load().mirx_rollout_layer(_ptr(qkv), b, n, int(heads), c3 // 3 // int(heads), float(scale),
                                                  _lib.ROLLOUT_FUSE[fusion], int(k), int(layer), int(layers), _ptr(ws), ws.numel(),
                                                  _stream(qkv.device)), "mirx_rollout_layer")


def rollout_finish(ws, layers, b, h, w, size, patches=None, query=None, out=None):
    """[HIP] mirx_rollout_finish: the vector chain over the workspace's `layers` slots, times clamp(patches . query, 0) when
    given (patches [b, h * w, e], query [e]), upsampled into out [b, H, W]."""
    H, W = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((b, H, W), dtype=torch.float32, device=ws.device)
    _check_ws(ws, ws.device, "rollout_finish")
    _check_f32(out, "rollout_finish: out")
    if tuple(out.shape) != (b, H, W) or out.device != ws.device:
        raise ValueError(f"rollout_finish: out must be [{b}, {H}, {W}] on {ws.device}")
    e = 0
    if (patches is None) != (query is None):
        raise ValueError("rollout_finish: patches and query go together")
    if patches is not None:
        _check_f32(patches, "rollout_finish: patches")
        _check_f32(query, "rollout_finish: query")
        e = patches.shape[-1]
        if tuple(patches.shape) != (b, h * w, e) or tuple(query.shape) != (e,):
            raise ValueError("rollout_finish: patches must be [b, h * w, e] and query [e]")
        if patches.device != ws.device or query.device != ws.device:
            raise ValueError(f"rollout_finish: patches and query must be on {ws.device}")
    with torch.cuda.device(ws.device):
        _lib.check(_lib.load().mirx_rollout_finish(_ptr(ws), ws.numel(), int(layers), b, int(h), int(w),
                                                   _ptr(patches) if patches is not None else None,
                                                   _ptr(query) if query is not None else None, e, H, W, _ptr(out),
                                                   _stream(ws.device)), "mirx_rollout_finish")
    return out


def _chunk_images(layers, n, total, budget):
    per = workspace_floats(layers, 1, n)
    return max(1, min(65535, total, int(budget) // per))


def rollout_maps(qkvs, heads, scale, fusion, k, h, w, size, patches=None, query=None, budget=None, keep_layers=False):
    """The kernels on given per-layer qkv tensors (a list of L CUDA fp32 [B, n, 3c]), images chunked by a workspace budget
    (floats) -> [B, H, W] (and the per-layer matrices [L, B, n, n] with keep_layers).  Image b's map does not depend on the
    chunking."""
    L, B, n = len(qkvs), qkvs[0].shape[0], qkvs[0].shape[1]
    dev = qkvs[0].device
    chunk = _chunk_images(L, n, B, WORKSPACE_FLOATS if budget is None else budget)
    out = torch.empty((B, int(size[0]), int(size[1])), dtype=torch.float32, device=dev)
    mats = []
    for b0 in range(0, B, chunk):
        nb = min(chunk, B - b0)
        ws = torch.empty((workspace_floats(L, nb, n),), dtype=torch.float32, device=dev)
        for layer, qkv in enumerate(qkvs):
            rollout_layer(qkv[b0:b0 + nb], heads, scale, fusion, k, layer, L, ws)
        rollout_finish(ws, L, nb, h, w, size, None if patches is None else patches[b0:b0 + nb], query, out[b0:b0 + nb])
        if keep_layers:
            mats.append(ws[:L * nb * n * n].view(L, nb, n, n).clone())
    return (out, torch.cat(mats, 1)) if keep_layers else out


_SIDE = {}


def _side_stream(dev):
    """One side stream per device for the layer kernels: at one image they fill CUs the forward leaves idle."""
    if dev.index not in _SIDE:
        _SIDE[dev.index] = torch.cuda.Stream(dev)
    return _SIDE[dev.index]


# ---- the explainer ----------------------------------------------------------------------------------------------------
def _projection_native(proj, x):
    """MedSigLIP's projection Sequential(Linear, LayerNorm, ReLU, Linear) on the project's kernels, or None when it is not
    that shape or a Linear would not take the project's kernel."""
    if not (isinstance(proj, nn.Sequential) and len(proj) == 4 and isinstance(proj[0], nn.Linear)
            and isinstance(proj[1], nn.LayerNorm) and isinstance(proj[2], nn.ReLU) and isinstance(proj[3], nn.Linear)):
        return None
    if proj.training or not (_linear_s3_ok(proj[0], x) and _linear_s3_ok(proj[3], x)):
        return None
    if not all(p.is_cuda and p.device == x.device and p.dtype == torch.float32 for p in proj.parameters()):
        return None
    return lambda t: _linear_auto(proj[3], torch.relu(_layernorm(proj[1], _linear_auto(proj[0], t))))


class AttentionRolloutMedSigLIP(nn.Module):
    """explanations.py AttentionRolloutMedSigLIP(model, head_fusion='mean', discard_ratio=0.9, query_guided=True)
    (query_tensor [1, 3, H, W], retrieved_tensor [B, 3, H, W]) -> [B, H, W]: the rollout importance of each patch of the
    retrieved images, optionally weighted by its cosine similarity to the query's embedding, upsampled to H x W."""

    def __init__(self, model, head_fusion: str = "mean", discard_ratio: float = 0.9, query_guided: bool = True):
        super().__init__()
        self.model = model
        self.head_fusion = head_fusion
        self.discard_ratio = discard_ratio
        self.query_guided = query_guided
        self.last_native = False
        self._keep_layers = False        # tests: keep the native per-layer matrices of the last call in last_layers
        self.last_layers = None

    @staticmethod
    def _fuse_heads(attn: torch.Tensor, mode: str) -> torch.Tensor:
        """[B, heads, N, N] -> [B, N, N]"""
        if mode == "mean":
            return attn.mean(dim=1)
        if mode == "max":
            return attn.max(dim=1).values
        if mode == "min":
            return attn.min(dim=1).values
        raise ValueError(f"Unknown head_fusion mode: {mode!r}")

    def _rollout(self, attentions):
        """list of [B, heads, N, N] -> the rollout [B, N, N] (row i: the influence of every token on token i)."""
        B, _, N, _ = attentions[0].shape
        eye = torch.eye(N, device=attentions[0].device, dtype=torch.float32)
        result = eye.unsqueeze(0).expand(B, -1, -1).clone()
        for att in attentions:
            a = self._fuse_heads(att.float(), self.head_fusion)
            if self.discard_ratio > 0.0:
                k = max(1, int(N * self.discard_ratio))
                thresh = a.kthvalue(k, dim=-1).values
                a = a * (a > thresh.unsqueeze(-1))
            a = a + eye.unsqueeze(0)
            a = a / (a.sum(dim=-1, keepdim=True) + 1e-8)
            result = torch.bmm(a, result)
        return result

    # -- native path --
    def _native_plan(self, query_tensor, retrieved_tensor):
        """(k, L, heads, n, grid) when the call can run natively, else None."""
        m = self.model
        if not isinstance(m, MedSigLIP) or m.training or m.backbone.training:
            return None
        x, q = retrieved_tensor, query_tensor
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] >= 1):
            return None
        if self.query_guided and not (q.is_cuda and q.dtype == torch.float32 and q.device == x.device and q.dim() == 4
                                      and q.shape[0] == 1):
            return None
        if self.head_fusion not in ("mean", "max", "min"):
            return None
        bb = m.backbone
        L = len(bb.encoder.layers)
        if L < 1 or L > 256:
            return None
        at = bb.encoder.layers[0].self_attn
        n = bb.embeddings.num_positions
        k = 0
        if self.discard_ratio > 0.0:
            k = max(1, int(n * self.discard_ratio))
            if not 1 <= k <= n:
                return None
        if not (1 <= n <= ROLLOUT_MAX_N and at.head_dim % 4 == 0 and at.head_dim <= ROLLOUT_MAX_HEAD_DIM
                and at.num_heads <= ROLLOUT_MAX_HEADS):
            return None
        with torch.no_grad():
            if not bb._native_encoder_ok(x):
                return None
            if self.query_guided and _projection_native(m.projection, x) is None:
                return None
        return k, L, at.num_heads, n, int(np.sqrt(n))

    def _forward_native(self, query_tensor, retrieved_tensor, plan):
        k, L, heads, n, grid = plan
        B, _, H, W = retrieved_tensor.shape
        m, bb = self.model, self.model.backbone
        scale = float(bb.encoder.layers[0].self_attn.scale)
        dev = retrieved_tensor.device
        x = retrieved_tensor.contiguous()
        out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        chunk = _chunk_images(L, n, B, WORKSPACE_FLOATS)
        main, side = torch.cuda.current_stream(dev), _side_stream(dev)
        mats = []
        q_feat = None
        if self.query_guided:
            q_feat = m(query_tensor.contiguous()).reshape(-1).contiguous()            # [E], unit norm
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            ws = torch.empty((workspace_floats(L, nb, n),), dtype=torch.float32, device=dev)
            ws.record_stream(side)

            def tap(layer, qkv):
                # the layer kernel on the side stream, behind the forward up to this layer's qkv; the forward goes on
                side.wait_stream(main)
                qkv.record_stream(side)
                with torch.cuda.stream(side):
                    rollout_layer(qkv, heads, scale, self.head_fusion, k, layer, L, ws)
            try:
                tokens = bb._hidden_tapped(x[b0:b0 + nb], tap)
                assert grid * grid == tokens.shape[1], f"Number of patches ({tokens.shape[1]}) is not a perfect square"
                patches = None
                if self.query_guided:
                    d = tokens.shape[-1]
                    patches = _normalize_rows(tokens.reshape(-1, d))
                    if d != q_feat.shape[0]:
                        patches = _normalize_rows(_projection_native(m.projection, patches)(patches))
                    patches = patches.view(nb, n, -1)
            finally:
                main.wait_stream(side)                   # every layer kernel of the chunk before anything reads or frees ws
            rollout_finish(ws, L, nb, grid, grid, (H, W), patches, q_feat, out[b0:b0 + nb])
            if self._keep_layers:
                mats.append(ws[:L * nb * n * n].view(L, nb, n, n).clone())
        self.last_layers = torch.cat(mats, 1) if self._keep_layers else None
        return out

    # -- the reference's formulas --
    def _forward_torch(self, query_tensor, retrieved_tensor):
        B, _, H, W = retrieved_tensor.shape
        with torch.no_grad():
            outs = self.model.backbone(pixel_values=retrieved_tensor, output_attentions=True, return_dict=True)
        if outs.attentions is None:
            raise RuntimeError("Model did not return attention weights (output_attentions=True is required).")
        importance = self._rollout(list(outs.attentions)).mean(dim=1)                   # [B, N]
        if self.query_guided:
            with torch.no_grad():
                patches = F.normalize(outs.last_hidden_state, dim=-1)
                q_feat = self.model(query_tensor).unsqueeze(1)
                if patches.shape[-1] != q_feat.shape[-1]:
                    patches = F.normalize(self.model.projection(patches), dim=-1)
                sim = (patches * q_feat.expand(B, patches.shape[1], -1)).sum(dim=-1).clamp(min=0)
                importance = importance * sim
        n = importance.shape[1]
        side = int(n ** 0.5)
        assert side * side == n, f"Number of patches ({n}) is not a perfect square"
        sal = F.interpolate(importance.reshape(B, 1, side, side), size=(H, W), mode="bilinear", align_corners=False)
        return sal.squeeze(1)

    def forward(self, query_tensor: torch.Tensor, retrieved_tensor: torch.Tensor) -> torch.Tensor:
        plan = self._native_plan(query_tensor, retrieved_tensor)
        if plan is not None:
            with torch.no_grad(), torch.cuda.device(retrieved_tensor.device):
                self.last_native = True
                return self._forward_native(query_tensor, retrieved_tensor, plan)
        self.last_native = False
        self.last_layers = None
        return self._forward_torch(query_tensor, retrieved_tensor)
