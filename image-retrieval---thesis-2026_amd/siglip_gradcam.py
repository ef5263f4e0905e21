"""Grad-CAM retrieval saliency for MedSigLIP.

Mirrors (paths into the reference tree):
  compute_gradcam_saliency   medsiglip_saliency.py:137-198
  _compute_single_gradcam    medsiglip_saliency.py:201-269

The target is the output x [1, N, D] of model.backbone.encoder.layers[-1] (before post_layernorm); grad = d sim / d x with
sim = sum over the query rows of cosine_similarity(model(img), query_emb); weights = grad.mean over the tokens,
cam = relu((x * weights).sum(-1)) on the sqrt(N)^2 grid, bilinearly upsampled to the image size, min-max normalised in numpy
(max - min > 1e-8, else zeros).

Native path: a CUDA fp32 image batch on a mirx MedSigLIP in eval mode whose encoder runs natively, within k_gradcam.hip's
limits.  Between x and the similarity only post_layernorm and the pooling head's attention touch the N tokens; everything
after them is one vector per image.  So one batched native forward gives x (SiglipVisionTower._last_layer_tokens), and the
exact gradient comes from a closed form: mirx_gradcam_pool (LayerNorm, probe scores, softmax, pooled tokens), the vector
tail forward and backward on mirx_gradcam_gemv / _layernorm / _gelu / _cosine_bwd, mirx_gradcam_tokens (the backward over
the tokens) and mirx_gradcam_finish (weights, cam, upsample, normalisation).  No autograd, no backward pass through the
tower.  Everywhere else the reference's formulas run in torch with autograd and hooks on the last encoder layer, as there,
including its failures.  `compute_gradcam_saliency.last_native` / `_compute_single_gradcam.last_native` tell which path ran.

Not reproduced: the reference's first forward + backward per image in compute_gradcam_saliency (its result is discarded);
its checks are kept (a non-square N and a query batch of more than one row raise RuntimeError, as they do there).  The native
path leaves the parameters' .grad untouched; the torch path leaves them filled by its last backward pass, as the reference.
"""

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .model import MedSigLIP, _ptr, _stream

GRADCAM_MAX_N = 1024             # include/mirx.h MIRX_GRADCAM_MAX_N
GRADCAM_MAX_HEADS = 16           # MIRX_GRADCAM_MAX_HEADS
GRADCAM_MAX_WIDTH = 8192         # MIRX_GRADCAM_MAX_WIDTH (also the vector length limit of the tail kernels)
GRADCAM_MAX_SIZE = 8192          # MIRX_GRADCAM_MAX_SIZE
WORKSPACE_FLOATS = 1 << 26       # images per chunk: this many workspace + token floats (256 MB)


def _check_f32(x, what):
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous float32 CUDA tensor")


# ---- the kernels ------------------------------------------------------------------------------------------------------
def workspace_floats(b, n, d, heads):
    v = int(_lib.load().mirx_gradcam_workspace_floats(int(b), int(n), int(d), int(heads)))
    if v < 0:
        _lib.check(v, "mirx_gradcam_workspace_floats")
    return v


def gradcam_pool(x, gamma, beta, eps, u, c, ws):
    """[HIP] mirx_gradcam_pool: x [b, n, d] -> ybar [b, heads, d]; LayerNorm stats and P stay in ws."""
    for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (u, "u"), (c, "c"), (ws, "ws")):
        _check_f32(t, f"gradcam_pool: {what}")
    b, n, d = x.shape
    heads = u.shape[0]
    ybar = torch.empty((b, heads, d), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_gradcam_pool(_ptr(x), b, n, d, heads, _ptr(gamma), _ptr(beta), float(eps), _ptr(u), _ptr(c),
                                                 _ptr(ws), ws.numel(), _ptr(ybar), _stream(x.device)), "mirx_gradcam_pool")
    return ybar


def gradcam_tokens(x, gamma, beta, u, w, e, ws):
    """[HIP] mirx_gradcam_tokens: the backward over the tokens (w [b, heads, d], e [b, heads]) into ws's column partials."""
    for t, what in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (u, "u"), (w, "w"), (e, "e"), (ws, "ws")):
        _check_f32(t, f"gradcam_tokens: {what}")
    b, n, d = x.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_gradcam_tokens(_ptr(x), b, n, d, u.shape[0], _ptr(gamma), _ptr(beta), _ptr(u), _ptr(w), _ptr(e),
                                                   _ptr(ws), ws.numel(), _stream(x.device)), "mirx_gradcam_tokens")


def gradcam_finish(x, heads, ws, size, out=None):
    """[HIP] mirx_gradcam_finish: weights, cam, upsample and normalisation -> out [b, H, W]."""
    _check_f32(x, "gradcam_finish: x")
    _check_f32(ws, "gradcam_finish: ws")
    b, n, d = x.shape
    H, W = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((b, H, W), dtype=torch.float32, device=x.device)
    _check_f32(out, "gradcam_finish: out")
    if tuple(out.shape) != (b, H, W):
        raise ValueError(f"gradcam_finish: out must be [{b}, {H}, {W}]")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().mirx_gradcam_finish(_ptr(x), b, n, d, int(heads), _ptr(ws), ws.numel(), H, W, _ptr(out),
                                                   _stream(x.device)), "mirx_gradcam_finish")
    return out


def _gemv(A, x, m, k, b, bias=None, res=None, lda=None, xs=None, mg=None, rmod=None, acol=0, xg=0):
    """[HIP] mirx_gradcam_gemv -> out [b, m] (see include/mirx.h; defaults: the plain GEMV out = x A^T)."""
    out = torch.empty((b, m), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().mirx_gradcam_gemv(_ptr(A), k if lda is None else lda, _ptr(x), k if xs is None else xs,
                                             None if bias is None else _ptr(bias), None if res is None else _ptr(res), m,
                                             _ptr(out), m, b, m, k, m if mg is None else mg, m if rmod is None else rmod, acol, xg,
                                             _stream(x.device)), "mirx_gradcam_gemv")
    return out


def _ln(v, ln, relu=False):
    b, n = v.shape
    out = torch.empty_like(v)
    st = torch.empty((b, 2), dtype=torch.float32, device=v.device)
    _lib.check(_lib.load().mirx_gradcam_layernorm(_ptr(v), b, n, _ptr(ln.weight.detach()), _ptr(ln.bias.detach()), float(ln.eps),
                                                  int(relu), _ptr(out), _ptr(st), _stream(v.device)), "mirx_gradcam_layernorm")
    return out, st


def _ln_bwd(g, v, st, ln, after=None, res=None):
    b, n = v.shape
    out = torch.empty_like(v)
    _lib.check(_lib.load().mirx_gradcam_layernorm_bwd(_ptr(g), None if after is None else _ptr(after), _ptr(v), _ptr(st),
                                                      _ptr(ln.weight.detach()), b, n, None if res is None else _ptr(res), _ptr(out),
                                                      _stream(v.device)), "mirx_gradcam_layernorm_bwd")
    return out


def _gelu(h, g=None):
    out = torch.empty_like(h)
    _lib.check(_lib.load().mirx_gradcam_gelu(_ptr(h), None if g is None else _ptr(g), h.numel(), 0 if g is None else 1, _ptr(out),
                                             _stream(h.device)), "mirx_gradcam_gelu")
    return out


def _cosine_bwd(p, q):
    out = torch.empty_like(p)
    _lib.check(_lib.load().mirx_gradcam_cosine_bwd(_ptr(p), p.shape[0], p.shape[1], _ptr(q), q.shape[0], _ptr(out), _stream(p.device)),
               "mirx_gradcam_cosine_bwd")
    return out


# ---- derived constants, once per weight version -----------------------------------------------------------------------
def _params(model):
    head, proj = model.backbone.head, model.projection
    return [head.probe, head.attention.in_proj_weight, head.attention.in_proj_bias, head.attention.out_proj.weight,
            head.attention.out_proj.bias, head.layernorm.weight, head.layernorm.bias, head.mlp.fc1.weight, head.mlp.fc1.bias,
            head.mlp.fc2.weight, head.mlp.fc2.bias, proj[0].weight, proj[0].bias, proj[1].weight, proj[1].bias, proj[3].weight,
            proj[3].bias]


def _constants(model):
    """U [heads, d], c [heads] (the probe query folded into the keys, formed in float64) and the transposed weight copies of
    the vector tail's backward; cached on the model per weight version."""
    key = tuple((p.data_ptr(), p._version, p.device) for p in _params(model))
    cached = model.__dict__.get("_mirx_gradcam")
    if cached is not None and cached[0] == key:
        return cached[1]
    head, proj = model.backbone.head, model.projection
    at, d = head.attention, head.probe.shape[-1]
    heads = at.num_heads
    dh = d // heads
    with torch.no_grad():
        q = head._probe_query().reshape(d).double()
        wk, bk = at.in_proj_weight[d:2 * d].double(), at.in_proj_bias[d:2 * d].double()
        tau = float(dh) ** -0.5
        u = (tau * (wk.view(heads, dh, d) * q.view(heads, dh, 1)).sum(1)).float().contiguous()
        c = (tau * (bk.view(heads, dh) * q.view(heads, dh)).sum(1)).float().contiguous()
        f = lambda t: t.detach().float().contiguous()            # noqa: E731
        t = lambda t: t.detach().t().float().contiguous()         # noqa: E731
        k = dict(u=u, c=c, wv=f(at.in_proj_weight[2 * d:]), bv=f(at.in_proj_bias[2 * d:]), wvT=t(at.in_proj_weight[2 * d:]),
                 wo=f(at.out_proj.weight), bo=f(at.out_proj.bias), woT=t(at.out_proj.weight),
                 w1=f(head.mlp.fc1.weight), b1=f(head.mlp.fc1.bias), w1T=t(head.mlp.fc1.weight),
                 w2=f(head.mlp.fc2.weight), b2=f(head.mlp.fc2.bias), w2T=t(head.mlp.fc2.weight),
                 p0=f(proj[0].weight), bp0=f(proj[0].bias), p0T=t(proj[0].weight),
                 p3=f(proj[3].weight), bp3=f(proj[3].bias), p3T=t(proj[3].weight))
    model.__dict__["_mirx_gradcam"] = (key, k)
    return k


def _native_ok(model, query_emb, img):
    """True when the call can run natively (checked after the reference's eval() / .to(device) side effects)."""
    if not isinstance(model, MedSigLIP) or model.training:
        return False
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and img.dim() == 4 and img.shape[0] >= 1):
        return False
    bb, proj = model.backbone, model.projection
    if not (isinstance(proj, nn.Sequential) and len(proj) == 4 and isinstance(proj[0], nn.Linear)
            and isinstance(proj[1], nn.LayerNorm) and isinstance(proj[2], nn.ReLU) and isinstance(proj[3], nn.Linear)):
        return False
    lns = (bb.post_layernorm, bb.head.layernorm, proj[1])
    if any(ln.weight is None or ln.bias is None or len(ln.normalized_shape) != 1 for ln in lns):
        return False
    if any(p is None for p in _params(model)):
        return False
    if not all(p.is_cuda and p.device == img.device and p.dtype == torch.float32 for p in model.parameters()):
        return False
    e = proj[3].out_features
    if not (isinstance(query_emb, torch.Tensor) and query_emb.is_cuda and query_emb.device == img.device
            and query_emb.dtype == torch.float32 and query_emb.dim() == 2 and query_emb.shape[1] == e
            and 1 <= query_emb.shape[0] <= 65535):
        return False
    d, heads, n = bb.config.hidden_size, bb.head.attention.num_heads, bb.embeddings.num_positions
    if not (1 <= n <= GRADCAM_MAX_N and 1 <= heads <= GRADCAM_MAX_HEADS and d % heads == 0 and d <= GRADCAM_MAX_WIDTH
            and max(e, proj[0].out_features, bb.config.intermediate_size) <= GRADCAM_MAX_WIDTH
            and 1 <= img.shape[2] <= GRADCAM_MAX_SIZE and 1 <= img.shape[3] <= GRADCAM_MAX_SIZE):
        return False
    with torch.no_grad():
        return bool(bb._native_encoder_ok(img))


def _square_or_raise(n):
    g = int(n ** 0.5)
    if g * g != n:
        raise RuntimeError(f"Grad-CAM needs a square token grid: {n} tokens do not reshape to {g} x {g}")


def gradcam_from_tokens(model, query_emb, x, size):
    """The native closed form on given last-layer tokens x [b, n, d] (CUDA fp32) -> maps [b, H, W] (one workspace)."""
    bb, k = model.backbone, _constants(model)
    head, proj = bb.head, model.projection
    b, n, d = x.shape
    heads = head.attention.num_heads
    dh = d // heads
    inter = head.mlp.fc1.out_features
    ws = torch.empty((workspace_floats(b, n, d, heads),), dtype=torch.float32, device=x.device)
    q = query_emb.contiguous()
    pl = bb.post_layernorm
    gamma, beta = pl.weight.detach(), pl.bias.detach()
    ybar = gradcam_pool(x, gamma, beta, pl.eps, k["u"], k["c"], ws)
    # the vector tail, forward
    o = _gemv(k["wv"], ybar, d, d, b, bias=k["bv"], lda=d, xs=heads * d, mg=dh, rmod=d, xg=d)
    a = _gemv(k["wo"], o, d, d, b, bias=k["bo"])
    t, st1 = _ln(a, head.layernorm)
    h = _gemv(k["w1"], t, inter, d, b, bias=k["b1"])
    z = _gemv(k["w2"], _gelu(h), d, inter, b, bias=k["b2"], res=a)
    p1 = _gemv(k["p0"], z, proj[0].out_features, d, b, bias=k["bp0"])
    r, st2 = _ln(p1, proj[1], relu=True)
    p2 = _gemv(k["p3"], r, proj[3].out_features, proj[3].in_features, b, bias=k["bp3"])
    # backward
    g_r = _gemv(k["p3T"], _cosine_bwd(p2, q), proj[3].in_features, proj[3].out_features, b)
    g_z = _gemv(k["p0T"], _ln_bwd(g_r, p1, st2, proj[1], after=r), d, proj[0].out_features, b)
    g_h = _gelu(h, _gemv(k["w2T"], g_z, inter, d, b))
    g_a = _ln_bwd(_gemv(k["w1T"], g_h, d, inter, b), a, st1, head.layernorm, res=g_z)
    g_o = _gemv(k["woT"], g_a, d, d, b)
    w = _gemv(k["wvT"], g_o, heads * d, dh, b, lda=d, xs=d, mg=d, rmod=d, acol=dh, xg=dh)
    e = _gemv(k["bv"], g_o, heads, dh, b, lda=0, xs=d, mg=1, rmod=1, acol=dh, xg=dh)
    gradcam_tokens(x, gamma, beta, k["u"], w, e, ws)
    return gradcam_finish(x, heads, ws, size)


def _native_maps(model, query_emb, imgs):
    """All images of imgs [K, 3, H, W] natively, in chunks sized by WORKSPACE_FLOATS -> [K, H, W] (CUDA fp32)."""
    bb = model.backbone
    n, d, heads = bb.embeddings.num_positions, bb.config.hidden_size, bb.head.attention.num_heads
    _square_or_raise(n)
    K, _, H, W = imgs.shape
    per = workspace_floats(1, n, d, heads) + n * d
    chunk = max(1, min(K, 65535, WORKSPACE_FLOATS // per))
    out = torch.empty((K, H, W), dtype=torch.float32, device=imgs.device)
    with torch.no_grad(), torch.cuda.device(imgs.device):
        for b0 in range(0, K, chunk):
            x = bb._last_layer_tokens(imgs[b0:b0 + chunk])
            out[b0:b0 + chunk] = gradcam_from_tokens(model, query_emb, x, (H, W))
    return out


# ---- the reference's formulas (torch, autograd) -----------------------------------------------------------------------
def _normalise01(cam):
    lo, hi = cam.min(), cam.max()
    if hi - lo > 1e-8:
        return (cam - lo) / (hi - lo)
    return np.zeros_like(cam)


def _single_torch(model, query_emb, img_tensor):
    layer = model.backbone.encoder.layers[-1]
    seen = {}

    def on_forward(module, inputs, output):
        seen["act"] = output[0] if isinstance(output, (tuple, list)) else output

    def on_backward(module, grad_inputs, grad_outputs):
        seen["grad"] = grad_outputs[0] if isinstance(grad_outputs, (tuple, list)) else grad_outputs

    handles = [layer.register_forward_hook(on_forward), layer.register_full_backward_hook(on_backward)]
    try:
        with torch.enable_grad():
            img = img_tensor.detach().requires_grad_(True)
            sim = F.cosine_similarity(model(img), query_emb.detach(), dim=1).sum()
            model.zero_grad()
            sim.backward()
    finally:
        for hd in handles:
            hd.remove()
    act, grad = seen["act"].detach(), seen["grad"].detach()
    cam = F.relu((act * grad.mean(dim=1, keepdim=True)).sum(dim=-1))
    g = int(cam.shape[1] ** 0.5)
    cam = cam.view(1, 1, g, g)
    cam = F.interpolate(cam, size=(img_tensor.shape[2], img_tensor.shape[3]), mode="bilinear", align_corners=False)
    return _normalise01(cam.squeeze().cpu().numpy())


def _single_native(model, query_emb, img_tensor):
    return _native_maps(model, query_emb, img_tensor.contiguous())[0].cpu().numpy()


def _from_device(maps):
    """The native [K, H, W] maps as the reference's list of numpy float32 maps."""
    return [m for m in maps.cpu().numpy()]


# ---- the reference's interface ----------------------------------------------------------------------------------------
def compute_gradcam_saliency(model, query_tensor, retrieved_tensor, device):
    """medsiglip_saliency.py compute_gradcam_saliency(model, query_tensor [1, 3, H, W], retrieved_tensor [K, 3, H, W], device)
    -> np.ndarray [K, H, W] in [0, 1]: per retrieved image the Grad-CAM of its cosine similarity to the query's embedding at
    the last encoder layer.  Side effects as there: model.eval(), model moved to device."""
    model.eval()
    with torch.no_grad():
        query_emb = model(query_tensor.to(device))
    model.to(device)
    model.eval()
    bb = model.backbone
    # the reference's discarded first pass fails on these: its hook reshapes the tokens to a square grid, and it calls
    # backward() on the [Bq] per-row similarity, which needs a single query row
    _square_or_raise(bb.embeddings.num_positions)
    if query_emb.shape[0] != 1:
        raise RuntimeError(f"grad can be implicitly created only for scalar outputs (query batch {query_emb.shape[0]})")
    imgs = retrieved_tensor.to(device)
    if _native_ok(model, query_emb, imgs):
        compute_gradcam_saliency.last_native = True
        maps = _from_device(_native_maps(model, query_emb, imgs.contiguous()))
    else:
        compute_gradcam_saliency.last_native = False
        maps = [_single_torch(model, query_emb, retrieved_tensor[i:i + 1].to(device)) for i in range(retrieved_tensor.shape[0])]
    return np.stack(maps, axis=0)


def _compute_single_gradcam(model, query_emb, img_tensor, device):
    """medsiglip_saliency.py _compute_single_gradcam(model, query_emb [Bq, E], img_tensor [1, 3, H, W], device) -> [H, W]:
    the Grad-CAM of sum_r cosine_similarity(model(img), query_emb[r]) at the last encoder layer, min-max normalised."""
    if (isinstance(img_tensor, torch.Tensor) and img_tensor.dim() == 4 and img_tensor.shape[0] == 1
            and _native_ok(model, query_emb, img_tensor)):
        _compute_single_gradcam.last_native = True
        return _single_native(model, query_emb, img_tensor)
    _compute_single_gradcam.last_native = False
    return _single_torch(model, query_emb, img_tensor)


compute_gradcam_saliency.last_native = False
_compute_single_gradcam.last_native = False
