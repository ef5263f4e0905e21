"""float64 restatement of ConvNeXtV2_SRA / ConvNeXtV2_PCAM for the SRA tests: the backbone up to its pre-pool map (the loop of
oracle/convnext.features without its pooling) and both pooling heads, written with F.conv2d / F.linear / F.layer_norm /
torch.softmax from the reference's formulas (model.py:120-278 there) -- independent of mirx.model's module tree: it reads a
state dict and nothing else."""
import torch
import torch.nn.functional as F

DEPTHS = (3, 3, 27, 3)
EPS = 1e-6
P = "convnext."


def _ln2d(x, w, b):
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, EPS).permute(0, 3, 1, 2)


def feature_map(x, sd):
    """[b, 3, H, W] -> the pre-pool map [b, 1024, H / 32, W / 32] (timm forward_features)."""
    x = F.conv2d(x, sd[P + "stem.0.weight"], sd[P + "stem.0.bias"], stride=4)
    x = _ln2d(x, sd[P + "stem.1.weight"], sd[P + "stem.1.bias"])
    for si, depth in enumerate(DEPTHS):
        sp = f"{P}stages.{si}."
        if si > 0:
            x = _ln2d(x, sd[sp + "downsample.0.weight"], sd[sp + "downsample.0.bias"])
            x = F.conv2d(x, sd[sp + "downsample.1.weight"], sd[sp + "downsample.1.bias"], stride=2)
        for bi in range(depth):
            bp = f"{sp}blocks.{bi}."
            c = x.shape[1]
            y = F.conv2d(x, sd[bp + "conv_dw.weight"], sd[bp + "conv_dw.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (c,), sd[bp + "norm.weight"], sd[bp + "norm.bias"], EPS)
            y = F.gelu(F.linear(y, sd[bp + "mlp.fc1.weight"], sd[bp + "mlp.fc1.bias"]))
            g = torch.linalg.vector_norm(y, ord=2, dim=(1, 2), keepdim=True)
            y = y + torch.addcmul(sd[bp + "mlp.grn.bias"], sd[bp + "mlp.grn.weight"], y * (g / (g.mean(dim=-1, keepdim=True) + 1e-6)))
            x = F.linear(y, sd[bp + "mlp.fc2.weight"], sd[bp + "mlp.fc2.bias"]).permute(0, 3, 1, 2) + x
    return x


def _gap_ln(x, nw, nb):
    return F.layer_norm(x.mean(dim=(2, 3)), (x.shape[1],), nw, nb, EPS)


def sra_head(x, w_att, nw, nb, lam):
    """SRA.forward: LN(GAP) + lam LN(mean_k sum_p softmax_p(w_att[k] . x[p]) x[p])  -> [b, c] (not normalised)."""
    b, c = x.shape[:2]
    xf = x.reshape(b, c, -1)
    a = torch.softmax(torch.einsum("kc,bcp->bkp", w_att.reshape(-1, c), xf), dim=2)
    s = torch.einsum("bkp,bcp->bkc", a, xf).mean(dim=1)
    return _gap_ln(x, nw, nb) + lam * F.layer_norm(s, (c,), nw, nb, EPS)


def pcam_head(x, w_cls, b_cls, nw, nb, lam, fc_w=None, fc_b=None):
    """PCAMPool.forward -> (embedding [b, D] unit norm, class_logits [b, K], pcam_probs [b, K, h, w], feat [b, c] before fc)."""
    b, c, h, w = x.shape
    k = w_cls.shape[0]
    z = _ln2d(x, nw, nb)
    zf = z.reshape(b, c, -1)
    probs = torch.sigmoid(torch.einsum("kc,bcp->bkp", w_cls.reshape(k, c), zf) + b_cls[None, :, None])
    q = probs / (probs.sum(dim=2, keepdim=True) + 1e-8)
    pooled = torch.einsum("bkp,bcp->bkc", q, zf)
    logits = torch.einsum("bkc,kc->bk", pooled, w_cls.reshape(k, c)) + b_cls
    feat = _gap_ln(x, nw, nb) + lam * torch.einsum("bk,bkc->bc", torch.softmax(logits, dim=1), pooled)
    out = feat if fc_w is None else F.linear(feat, fc_w, fc_b)
    return F.normalize(out, dim=1), logits, probs.reshape(b, k, h, w), feat


def _sd64(sd):
    return {k: v.detach().cpu().double() for k, v in sd.items()}


def embed_sra(x, sd, lam):
    sd = _sd64(sd)
    m = feature_map(x.cpu().double(), sd)
    return F.normalize(sra_head(m, sd["sra.conv_att.weight"], sd[P + "head.norm.weight"], sd[P + "head.norm.bias"], lam), dim=1)


def embed_pcam(x, sd, lam):
    sd = _sd64(sd)
    m = feature_map(x.cpu().double(), sd)
    return pcam_head(m, sd["pcam.classifier.weight"], sd["pcam.classifier.bias"], sd[P + "head.norm.weight"], sd[P + "head.norm.bias"],
                     lam, sd.get("pcam.fc.weight"), sd.get("pcam.fc.bias"))[0]


def randomize(model, seed):
    """Random non-trivial weights for tests (in place, under no_grad): LayerNorm affines, GRN gamma / beta, biases, and head
    weights large enough that the attention / CAM maps are far from uniform."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.copy_(0.5 + torch.rand(p.shape, generator=g))
            elif "grn" in name:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("conv_att.weight") or name.endswith("classifier.weight"):
                p.copy_(0.08 * torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return model
