"""float64 restatement of SwinV2-B (timm swinv2_base_window12to24_192to384 at 384 x 384, res-post-norm blocks) for the SwinV2 tests,
written with F.linear / F.layer_norm / F.normalize / torch.roll from the published definition (Liu et al., "Swin Transformer V2")
-- independent of mirx.model's module tree: it reads a state dict and nothing else."""
import math

import torch
import torch.nn.functional as F

DEPTHS = (2, 2, 18, 2)
HEADS = (4, 8, 16, 32)
WINDOW = 24
PRETRAINED = (12, 12, 12, 6)


def window_shift(side, i):
    """(window, shift) of block i on a side x side map: the window is clamped to the map, no shift when it covers the map."""
    ws = min(WINDOW, side)
    return ws, (0 if side <= ws or i % 2 == 0 else WINDOW // 2)


def coords_table(ws, pretrained):
    """Log-spaced relative coordinates [(2 ws - 1)^2, 2], normalised by the pretrained window (a float32 table, as the published
    model builds it: its rounding is part of the network's definition)."""
    r = torch.arange(-(ws - 1), ws, dtype=torch.float32)
    t = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1) / (pretrained - 1) * 8
    return (torch.sign(t) * torch.log2(t.abs() + 1.0) / math.log2(8)).reshape(-1, 2).double()


def bias_table(sd, p, ws, pretrained):
    """16 sigmoid(cpb_mlp(table)) -> [heads, (2 ws - 1)^2]"""
    h = F.relu(F.linear(coords_table(ws, pretrained), sd[p + "cpb_mlp.0.weight"], sd[p + "cpb_mlp.0.bias"]))
    return (16 * torch.sigmoid(F.linear(h, sd[p + "cpb_mlp.2.weight"]))).t()


def region_ids(side, ws, s):
    """Region of every pixel of the shifted map: three slices per axis."""
    r = torch.zeros(side, dtype=torch.long)
    r[side - ws:] = 1
    r[side - s:] = 2
    return (3 * r[:, None] + r[None, :]).reshape(-1)


def window_attention(qkv, heads, side, ws, s, table, ls):
    """qkv [B, side, side, 3 C] (bias included) -> [B, side, side, C], float64.  table [heads, (2 ws - 1)^2]; ls [heads]
    (exp of the clamped logit scale)."""
    b, _, _, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    x = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2)) if s else qkv
    nw = side // ws
    win = x.reshape(b, nw, ws, nw, ws, 3, heads, d).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, b, nw * nw, heads, ws * ws, d)
    q, k, v = win[0], win[1], win[2]
    a = F.normalize(q, dim=-1, eps=1e-12) @ F.normalize(k, dim=-1, eps=1e-12).transpose(-1, -2) * ls.view(1, 1, heads, 1, 1)
    yy, xx = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    yy, xx = yy.reshape(-1), xx.reshape(-1)
    rel = (yy[:, None] - yy[None, :] + ws - 1) * (2 * ws - 1) + (xx[:, None] - xx[None, :] + ws - 1)
    a = a + table[:, rel].view(1, 1, heads, ws * ws, ws * ws)
    if s:
        reg = region_ids(side, ws, s).view(nw, ws, nw, ws).permute(0, 2, 1, 3).reshape(nw * nw, ws * ws)
        mask = torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0).double()
        a = a + mask.view(1, nw * nw, 1, ws * ws, ws * ws)
    o = a.softmax(-1) @ v                                              # [b, nW, heads, N, d]
    o = o.reshape(b, nw, nw, heads, ws, ws, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(b, side, side, c)
    return torch.roll(o, shifts=(s, s), dims=(1, 2)) if s else o


def ln(x, sd, p):
    return F.layer_norm(x, x.shape[-1:], sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def features(x, sd, prefix="swinv2."):
    """x [B, 3, 384, 384] -> [B, 1024] (mean of the final norm's tokens, before any fc / normalisation), float64."""
    sd = {k[len(prefix):]: v.detach().cpu().double() for k, v in sd.items() if k.startswith(prefix)}
    x = F.conv2d(x.double().cpu(), sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=4).permute(0, 2, 3, 1)
    x = ln(x, sd, "patch_embed.norm")
    for si, depth in enumerate(DEPTHS):
        if si > 0:
            b, h, w, c = x.shape
            q = [x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]]
            x = ln(F.linear(torch.cat(q, -1), sd[f"layers.{si}.downsample.reduction.weight"]), sd, f"layers.{si}.downsample.norm")
        side = x.shape[1]
        for i in range(depth):
            p = f"layers.{si}.blocks.{i}."
            ws, s = window_shift(side, i)
            c = x.shape[-1]
            bias = torch.cat([sd[p + "attn.q_bias"], torch.zeros(c, dtype=torch.float64), sd[p + "attn.v_bias"]])
            ls = torch.clamp(sd[p + "attn.logit_scale"].reshape(-1), max=math.log(100.0)).exp()
            a = window_attention(F.linear(x, sd[p + "attn.qkv.weight"], bias), HEADS[si], side, ws, s,
                                 bias_table(sd, p + "attn.", ws, PRETRAINED[si]), ls)
            x = x + ln(F.linear(a, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"]), sd, p + "norm1")
            h = F.gelu(F.linear(x, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
            x = x + ln(F.linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]), sd, p + "norm2")
    return ln(x, sd, "norm").mean(dim=(1, 2))


def embed(x, sd):
    """The reference forward(): features -> (fc) -> F.normalize, float64."""
    f = features(x, sd)
    if "fc.weight" in sd:
        f = F.linear(f, sd["fc.weight"].detach().cpu().double(), sd["fc.bias"].detach().cpu().double())
    return F.normalize(f, dim=1)


def randomize(model, seed):
    """Random non-trivial weights for tests: LayerNorm affines, logit scales (some above the ln 100 clamp), cpb_mlp, q / v
    biases and Linear biases drawn at random (in place, under no_grad)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("logit_scale"):
                p.copy_(math.log(10) + 2.5 * torch.rand(p.shape, generator=g))          # ls in [10, 122]: some clamped at 100
            elif "norm" in name and name.endswith("weight"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif name.endswith("bias") or name.endswith("q_bias") or name.endswith("v_bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "cpb_mlp" in name:
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if name.endswith("0.weight") else 0.05))
    return model
