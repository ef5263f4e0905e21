"""SimAtt: similarity-attention saliency for DenseNet121.

Mirrors (paths into the reference tree):
  SimAtt           explanations.py:605-661   (compute_saliency.py:189-192, the default --explainer of five more drivers)
  ModelOutputs     gradcam.py:5-57           (restated below without its per-call print)

The reference runs the model on cat(x_q, x_p, x_n) with autograd recording, x the raw embedding and `feats` the last target
activation inside the feature module:
    xn = normalize(x.detach(), dim=1);  wt = |xn[0] - xn[1:]|;  wt[0] = 1 - wt[0] if x_p is given (the first row only, whatever
    x_p's batch size);  wt = prod over rows (all ones when x_p = x_n = None);  s_b = sum_d |x[b, d]| wt[d]
    grads = autograd.grad(s, feats);  weights = mean over positions of grads;  M_b = relu(sum_c weights[b, c] feats[b, c])
and upsamples M bilinearly to the input size -> [B, H, W], the query's own map first.

Native path.  In compute_saliency.py's recipe -- SimAtt(seq, seq[0], ["relu"]) on seq = Sequential(features, avgpool[, fc]) --
everything behind the target map is average pool -> optional fc -> a score linear in |x|, so the gradient is the same at every
position and has a closed form: weights_b = W_fc^T (sign(x_b) * wt) / (h * w) (W_fc = identity without fc, sign(0) = 0).  When
`model` is that Sequential of a mirx DenseNet121 (the feature stack, an AdaptiveAvgPool2d to 1 x 1, at most one fp32 nn.Linear
over the stack's channels, nothing else) with "relu" among the target layers, everything in eval mode and the inputs CUDA fp32
with 2 or more images in all, the rows of the map come from DenseNet121._relu_rows (the embedder's own kernels, no autograd
graph, fine under torch.no_grad()) and the pooled embedding, wt, the weights, the maps and the upsample from one mirx_simatt call
(k_simatt.hip, two launches), written into the returned tensor.

Everywhere else the reference's formulas run in torch with torch.autograd.grad, including its failures, which are kept:
  * the DenseNet form of the other five drivers, SimAtt(Sequential(*model.children()), seq[0], ["relu"]): seq[0] is the
    (features, avgpool) pair, which has no child named "relu" -> IndexError at A[-1]; with an fc, a shape RuntimeError before it;
  * their ResNet50 / ConvNeXtV2 forms, SimAtt(model, <a nested layer>, target_layers=None): the layer is not a direct child of
    the model, so no activation is collected -> IndexError at A[-1] (TypeError from `name in None` when it is a direct child);
  * no parameter or input that requires grad, or a call under torch.no_grad(): RuntimeError from autograd.grad.
`last_native` tells which path ran.  simatt_pairs is the batched form of the drivers' per-hit loops.

The feature stack finds its DenseNet121 through the weak reference SimCAM_Densenet121 uses (model._OwnerRef).  The driver's
`model = nn.Sequential(*list(model.children())[0], *list(model.children())[1:])` drops the DenseNet121 itself; the first native
call then builds a headless one around the same stack (DenseNet121._adopt: no parameter is copied) and the Sequential keeps it.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .model import DenseNet121, _OwnerRef, _ptr, _stream

SIMATT_MAX_HW = 1024           # include/mirx.h MIRX_SIMATT_MAX_*
SIMATT_MAX_C = 16384
SIMATT_MAX_D = 16384
SIMATT_MAX_B = 65535
SIMATT_MAX_SIZE = 8192
EMBED_CHUNK = 64               # images per _relu_rows call


# ---- the kernel -------------------------------------------------------------------------------------------------------
def simatt_maps(rows, fc_weight, fc_bias, size, mode, h, w, positive=False, out=None):
    """[HIP] mirx_simatt on given rows [B, h * w, C] (CUDA fp32, image 0 the query); fc_weight [D, C] / fc_bias [D] or None.
    mode="group" -> [B, H, W] (one wt over the images 1 .. B - 1, its first factor flipped when `positive`);
    mode="pairs" -> [B - 1, 2, H, W] (retrieval k alone against the query: the query's map under pair k, retrieval k's)."""
    if mode not in ("group", "pairs"):
        raise ValueError(f"simatt_maps: mode must be 'group' or 'pairs', got {mode!r}")
    H, W = int(size[0]), int(size[1])
    h, w = int(h), int(w)
    if rows.dim() != 3 or h < 1 or w < 1 or rows.shape[1] != h * w:
        raise ValueError(f"simatt_maps: rows must be [B, h * w, C] (got {tuple(rows.shape)}, h x w = {h} x {w})")
    if not (rows.is_cuda and rows.dtype == torch.float32):
        raise ValueError("simatt_maps: rows must be a float32 CUDA tensor")
    b, hw, c = rows.shape
    if not (2 <= b <= SIMATT_MAX_B and hw <= SIMATT_MAX_HW and 1 <= c <= SIMATT_MAX_C):
        raise ValueError(f"simatt_maps: needs 2 <= B <= {SIMATT_MAX_B}, h * w <= {SIMATT_MAX_HW}, 1 <= C <= {SIMATT_MAX_C} "
                         f"(got B = {b}, h * w = {hw}, C = {c})")
    if not (1 <= H <= SIMATT_MAX_SIZE and 1 <= W <= SIMATT_MAX_SIZE):
        raise ValueError(f"simatt_maps: size must be within [1, {SIMATT_MAX_SIZE}] (got {H} x {W})")
    d = 0
    if fc_weight is None:
        if fc_bias is not None:
            raise ValueError("simatt_maps: fc_bias without fc_weight")
    else:
        if fc_weight.dim() != 2 or fc_weight.shape[1] != c or not 1 <= fc_weight.shape[0] <= SIMATT_MAX_D:
            raise ValueError(f"simatt_maps: fc_weight must be [D <= {SIMATT_MAX_D}, C = {c}] (got {tuple(fc_weight.shape)})")
        d = fc_weight.shape[0]
        if fc_bias is not None and tuple(fc_bias.shape) != (d,):
            raise ValueError(f"simatt_maps: fc_bias must be [{d}] (got {tuple(fc_bias.shape)})")
        for t in (fc_weight, fc_bias):
            if t is not None and not (t.dtype == torch.float32 and t.device == rows.device):
                raise ValueError("simatt_maps: the fc must be float32 on the rows' device")
        fc_weight = fc_weight.detach().contiguous()
        fc_bias = fc_bias.detach().contiguous() if fc_bias is not None else None
    lib = _lib.load()
    rows = rows.contiguous()
    kind = _lib.SIMATT_GROUP if mode == "group" else _lib.SIMATT_PAIRS
    shape = (b, H, W) if mode == "group" else (b - 1, 2, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rows.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != rows.device:
        raise ValueError(f"simatt_maps: out must be a contiguous float32 {shape} tensor on {rows.device}")
    n_ws = lib.mirx_simatt_workspace_floats(b, c, d, kind)
    if n_ws < 0:
        _lib.check(int(n_ws), "mirx_simatt_workspace_floats")
    with torch.cuda.device(rows.device):
        ws = torch.empty((n_ws,), dtype=torch.float32, device=rows.device)
        _lib.check(lib.mirx_simatt(_ptr(rows), b, h, w, c, _ptr(fc_weight) if d else None,
                                   _ptr(fc_bias) if fc_bias is not None else None, d, kind, 1 if positive else 0, H, W, _ptr(ws),
                                   ws.numel(), _ptr(out), _stream(rows.device)), "mirx_simatt")
    return out


# ---- the native gate --------------------------------------------------------------------------------------------------
def _densenet_side(n):
    """The side of DenseNet121's last map for an input side n: conv0 (7, stride 2, pad 3), pool0 (3, stride 2, pad 1), three
    2 x 2 average pools."""
    n = (n - 1) // 2 + 1
    n = (n - 1) // 2 + 1
    return n // 8


def _native_plan(model, feature_module, target_layers, x):
    """(owner, fc or None) when cat(x_q, x_p, x_n) = x can take the native path, else None."""
    if not isinstance(target_layers, (list, tuple)) or "relu" not in target_layers:
        return None
    ref = feature_module.__dict__.get("_mirx_owner") if isinstance(feature_module, nn.Module) else None
    if not isinstance(ref, _OwnerRef) or not isinstance(feature_module._modules.get("norm5"), nn.BatchNorm2d):
        return None                                         # not the feature stack of a mirx DenseNet121
    mods = list(model._modules.values()) if isinstance(model, nn.Module) else []
    if len(mods) not in (2, 3) or mods[0] is not feature_module or not isinstance(mods[1], nn.AdaptiveAvgPool2d):
        return None
    if mods[1].output_size not in (1, (1, 1)):
        return None
    fc = mods[2] if len(mods) == 3 else None
    c = feature_module.norm5.num_features
    if fc is not None:
        if not (isinstance(fc, nn.Linear) and fc.in_features == c and 1 <= fc.out_features <= SIMATT_MAX_D
                and fc.weight.dtype == torch.float32 and fc.weight.device == x.device
                and (fc.bias is None or (fc.bias.dtype == torch.float32 and fc.bias.device == x.device))):
            return None
    if model.training or feature_module.training or (fc is not None and fc.training):
        return None
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and 2 <= x.shape[0] <= SIMATT_MAX_B and x.shape[1] == 3):
        return None
    if any(t.device != x.device for t in feature_module.parameters()):
        return None                                         # the torch path raises what the reference raises
    H, W = x.shape[-2:]
    h, w = _densenet_side(H), _densenet_side(W)
    if not (h >= 1 and w >= 1 and h * w <= SIMATT_MAX_HW and H <= SIMATT_MAX_SIZE and W <= SIMATT_MAX_SIZE and c <= SIMATT_MAX_C):
        return None
    owner = ref()
    if owner is None:
        # compute_saliency.py:190 rebinds `model` to the Sequential, which drops the DenseNet121 and keeps its stack: a headless
        # model around the same stack takes its place, kept alive by the Sequential (in __dict__: outside the module tree)
        owner = DenseNet121._adopt(feature_module)
        model.__dict__["_mirx_keep"] = owner
    if not isinstance(owner, DenseNet121) or owner.densenet121[0] is not feature_module:
        return None
    return owner, fc


def _rows_of(owner, x):
    """DenseNet121._relu_rows over x in chunks -> (rows [B, h * w, C], h, w)."""
    cache = owner._cache()
    parts = []
    for i in range(0, x.shape[0], EMBED_CHUNK):
        rows, h, w = owner._relu_rows(x[i:i + EMBED_CHUNK], cache)
        parts.append(rows)
    return (parts[0] if len(parts) == 1 else torch.cat(parts)), h, w


# ---- the explainer ----------------------------------------------------------------------------------------------------
class SimAtt(nn.Module):
    """explanations.py SimAtt(model, feature_module, target_layers)(x_q, x_p=None, x_n=None) -> [B, H, W] over
    cat(x_q, x_p, x_n): anchor + positive, anchor + negative, triplet, or any number of either."""

    def __init__(self, model, feature_module, target_layers):
        super().__init__()
        self.model = model
        self.feature_module = feature_module
        self.target_layers = target_layers
        self.last_native = False
        ref = feature_module.__dict__.get("_mirx_owner") if isinstance(feature_module, nn.Module) else None
        self.__dict__["_mirx_keep"] = ref() if ref is not None else None      # outside the module tree and the state dict

    def forward(self, x_q, x_p=None, x_n=None):
        _, _, H, W = x_q.size()
        x = x_q
        if x_p is not None:
            x = torch.cat((x, x_p))
        if x_n is not None:
            x = torch.cat((x, x_n))
        plan = _native_plan(self.model, self.feature_module, self.target_layers, x)
        if plan is not None:
            owner, fc = plan
            with torch.no_grad(), torch.cuda.device(x.device):
                rows, h, w = _rows_of(owner, x)
                self.last_native = True
                return simatt_maps(rows, None if fc is None else fc.weight, None if fc is None else fc.bias, (H, W), "group",
                                   h, w, positive=x_p is not None)
        self.last_native = False
        return self._forward_torch(x, H, W, x_p is not None)

    def _extract(self, x):
        """gradcam.py ModelOutputs (return_gradients=False) without its print: the model's children in order, the outputs of
        `target_layers` inside the feature module, the pooled map flattened -> (activations, x)."""
        acts = []
        for module in self.model._modules.values():
            if module == self.feature_module:
                acts = []
                for name, sub in module._modules.items():
                    x = sub(x)
                    if name in self.target_layers:
                        acts += [x]
            elif isinstance(module, nn.AdaptiveAvgPool2d):
                x = module(x)
                x = x.view(x.size(0), -1)
            else:
                x = module(x)
        return acts, x

    def _forward_torch(self, x, H, W, positive):
        A, x = self._extract(x)
        x_norm = F.normalize(x.detach(), dim=1)
        w = torch.abs(x_norm[0] - x_norm[1:])
        if positive:
            w[0] = 1 - w[0]
        w = torch.prod(w, dim=0)
        s = torch.matmul(torch.abs(x), w)
        feats = A[-1]
        grads = torch.autograd.grad(torch.unbind(s), feats)[0]
        with torch.no_grad():
            weights = torch.mean(grads, dim=(2, 3))
            M = torch.bmm(weights.unsqueeze(1), feats.reshape(feats.shape[0], feats.shape[1], -1))
            M = M.reshape(feats.shape[0], 1, feats.shape[2], feats.shape[3]).clamp(min=0)
            return F.interpolate(M, size=(H, W), mode="bilinear").squeeze(1)


def simatt_pairs(model_or_explainer, x_q, x_r, positive=True):
    """One query x_q [1, 3, H, W] against K retrievals x_r [K, 3, H, W], each pair on its own -> [K, 2, H, W]: row k is
    SimAtt(..)(x_q, x_r[k:k+1]) (positive) or SimAtt(..)(x_q, None, x_r[k:k+1]) (negative) -- what the drivers' per-hit loops
    compute, re-embedding the query per hit.  Native: one embed of the 1 + K images and one mirx_simatt call in pairs mode.
    `model_or_explainer`: a SimAtt, or the flattened Sequential (then SimAtt(model, model[0], ["relu"]) is built)."""
    ex = model_or_explainer if isinstance(model_or_explainer, SimAtt) else SimAtt(model_or_explainer, model_or_explainer[0], ["relu"])
    if x_q.dim() != 4 or x_r.dim() != 4 or x_q.shape[0] != 1 or x_r.shape[0] < 1 or x_q.shape[1:] != x_r.shape[1:]:
        raise ValueError(f"simatt_pairs: x_q must be [1, C, H, W] and x_r [K >= 1, C, H, W] (got {tuple(x_q.shape)}, "
                         f"{tuple(x_r.shape)})")
    H, W = x_q.shape[-2:]
    x = torch.cat((x_q, x_r))
    plan = _native_plan(ex.model, ex.feature_module, ex.target_layers, x)
    if plan is not None:
        owner, fc = plan
        with torch.no_grad(), torch.cuda.device(x.device):
            rows, h, w = _rows_of(owner, x)
            ex.last_native = True
            return simatt_maps(rows, None if fc is None else fc.weight, None if fc is None else fc.bias, (H, W), "pairs", h, w,
                               positive=positive)
    maps = [ex(x_q, x_r[k:k + 1]) if positive else ex(x_q, None, x_r[k:k + 1]) for k in range(x_r.shape[0])]
    return torch.stack(maps)
