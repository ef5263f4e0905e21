"""Float64 numpy restatement of the Grad-CAM closed form and the seeded tiny MedSigLIP of the fixture
(tests/golden/make_golden_gradcam.py).  The tokens x of the last encoder layer come from the model's torch forward; from there
on everything is numpy: post_layernorm, the pooling head (probe attention, out_proj, LayerNorm, tanh-GELU MLP), the
projection, the summed cosine, the exact backward of all of it down to x, then weights, cam, upsample and normalisation."""
import numpy as np
import torch

VISION = dict(hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=4, image_size=35, patch_size=7)
EMBED = 16
N = (35 // 7) ** 2            # 25 tokens: a 5 x 5 grid, not a multiple of 16
SIZE = (35, 35)
BATCH = 3
NAN_IMAGE = 1                 # the image of the "nan" case with a NaN pixel
CASES = ("k1", "k3", "bq2", "flat", "nan")


def build_model(weights=None, dtype=torch.float64):
    """The fixture's MedSigLIP: weights drawn from a fixed seed (float32 values), or the given float32 state dict."""
    from mirx.model import MedSigLIP
    torch.manual_seed(0)
    m = MedSigLIP(vision_config=VISION, embed_dim=EMBED).eval()
    if weights is None:
        g = torch.Generator().manual_seed(11)
        sd = {}
        for k, v in m.state_dict().items():
            scale = 0.2 if v.dim() < 2 else 1.0 / np.sqrt(v.shape[-1] if v.dim() == 2 else v[0].numel())
            base = torch.ones_like(v) if k.endswith("weight") and v.dim() == 1 else torch.zeros_like(v)
            sd[k] = (base + scale * torch.randn(v.shape, generator=g)).float()
        weights = sd
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in weights.items()})
    return m.to(dtype)


def weights_of(model):
    return {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}


def pixels(seed, k):
    return torch.randn((k, 3) + SIZE, generator=torch.Generator().manual_seed(seed)).double()       # float32 values


def case_inputs(case):
    """(query pixels, retrieved pixels, zero the projection's last weight?) of a fixture case."""
    q = pixels(1, 2 if case == "bq2" else 1)
    r = pixels(2, 1 if case in ("k1", "bq2") else BATCH)
    if case == "nan":
        r = r.clone()
        r[NAN_IMAGE, 1, 17, 3] = float("nan")
    return q, r, case == "flat"


def last_tokens(model, img):
    """x: the last encoder layer's output [B, N, D] (torch path, no grad)."""
    bb = model.backbone
    with torch.no_grad():
        x, _ = bb.encoder(bb.embeddings(img), None)
    return x.double().cpu().numpy()


def _ln(v, g, b, eps):
    mu = v.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(((v - mu) ** 2).mean(-1, keepdims=True) + eps)
    xh = (v - mu) * r
    return xh * g + b, xh, r


def _ln_bwd(gy, xh, r, g):
    gh = gy * g
    return r * (gh - gh.mean(-1, keepdims=True) - xh * (gh * xh).mean(-1, keepdims=True))


_KB = np.sqrt(2.0 / np.pi)


def _gelu(h):
    return 0.5 * h * (1.0 + np.tanh(_KB * (h + 0.044715 * h ** 3)))


def _gelu_d(h):
    t = np.tanh(_KB * (h + 0.044715 * h ** 3))
    return 0.5 * (1.0 + t) + 0.5 * h * (1.0 - t * t) * _KB * (1.0 + 3.0 * 0.044715 * h * h)


TRACE_KEYS = ("mu", "r", "y", "S", "P", "ybar", "o", "a", "t", "h", "z", "p1", "l1", "rr", "p2",
              "g_p2", "g_rr", "g_p1", "g_z", "g_h", "g_a", "g_o", "w", "e", "dP", "dsum", "g_y", "g_x")


def trace(W, x, q, heads):
    """Every intermediate (float64) of d/dx sum_r cos(model(x), q_r) for one image's tokens x [N, D] (W: float64 state dict,
    q [Bq, E]), under the names of DESIGN 21: the forward mu, r (1 / std), y, S, P, ybar, o, a, t, h, z, p1, l1, rr, p2; the
    backward g_p2 ... g_o, w [H, D], e [H] (the gradient at the value projection), dP, dsum = sum_n P dP, g_y, g_x; and the
    folded probe U [H, D], c [H]."""
    P = "backbone."
    D = x.shape[1]
    dh = D // heads
    y, xh, r = _ln(x, W[P + "post_layernorm.weight"], W[P + "post_layernorm.bias"], 1e-6)
    ipw, ipb = W[P + "head.attention.in_proj_weight"], W[P + "head.attention.in_proj_bias"]
    wq, wk, wv = ipw[:D], ipw[D:2 * D], ipw[2 * D:]
    bq, bk, bv = ipb[:D], ipb[D:2 * D], ipb[2 * D:]
    qp = wq @ W[P + "head.probe"].reshape(D) + bq
    tau = dh ** -0.5
    U = np.stack([tau * wk[h * dh:(h + 1) * dh].T @ qp[h * dh:(h + 1) * dh] for h in range(heads)])      # [H, D]
    c = np.array([tau * qp[h * dh:(h + 1) * dh] @ bk[h * dh:(h + 1) * dh] for h in range(heads)])
    S = y @ U.T + c                                                                                        # [N, H]
    Pm = np.exp(S - S.max(0, keepdims=True))
    Pm = Pm / Pm.sum(0, keepdims=True)
    Yb = Pm.T @ y                                                                                          # [H, D]
    o = np.concatenate([wv[h * dh:(h + 1) * dh] @ Yb[h] for h in range(heads)]) + bv
    a = W[P + "head.attention.out_proj.weight"] @ o + W[P + "head.attention.out_proj.bias"]
    t, txh, tr = _ln(a, W[P + "head.layernorm.weight"], W[P + "head.layernorm.bias"], 1e-6)
    hpre = W[P + "head.mlp.fc1.weight"] @ t + W[P + "head.mlp.fc1.bias"]
    z = a + W[P + "head.mlp.fc2.weight"] @ _gelu(hpre) + W[P + "head.mlp.fc2.bias"]
    p1 = W["projection.0.weight"] @ z + W["projection.0.bias"]
    l1, l1xh, l1r = _ln(p1, W["projection.1.weight"], W["projection.1.bias"], 1e-5)
    rr = np.maximum(l1, 0.0)
    p2 = W["projection.3.weight"] @ rr + W["projection.3.bias"]
    # backward: sum_r cos(p2 / |p2|, q_r)
    pn = max(np.linalg.norm(p2), 1e-12)
    e = p2 / pn
    Q = sum(qr / max(np.linalg.norm(qr), 1e-8) for qr in q)
    en = max(np.linalg.norm(e), 1e-8)
    g_e = Q / en - (e @ Q) * e / en ** 3
    g_p2 = (g_e - e * (e @ g_e)) / pn
    g_rr = W["projection.3.weight"].T @ g_p2
    g_p1 = _ln_bwd(g_rr * (l1 > 0), l1xh, l1r, W["projection.1.weight"])
    g_z = W["projection.0.weight"].T @ g_p1
    g_h = (W[P + "head.mlp.fc2.weight"].T @ g_z) * _gelu_d(hpre)
    g_a = g_z + _ln_bwd(W[P + "head.mlp.fc1.weight"].T @ g_h, txh, tr, W[P + "head.layernorm.weight"])
    g_o = W[P + "head.attention.out_proj.weight"].T @ g_a
    w = np.stack([wv[h * dh:(h + 1) * dh].T @ g_o[h * dh:(h + 1) * dh] for h in range(heads)])        # [H, D]
    d = np.array([g_o[h * dh:(h + 1) * dh] @ bv[h * dh:(h + 1) * dh] for h in range(heads)])
    dP = y @ w.T + d
    dsum = (Pm * dP).sum(0, keepdims=True)
    dS = Pm * (dP - dsum)
    g_y = dS @ U + Pm @ w
    g_x = _ln_bwd(g_y, xh, r, W[P + "post_layernorm.weight"])
    return dict(mu=x.mean(-1), r=r[:, 0], y=y, S=S, P=Pm, ybar=Yb, o=o, a=a, t=t, h=hpre, z=z, p1=p1, l1=l1, rr=rr, p2=p2,
                g_p2=g_p2, g_rr=g_rr, g_p1=g_p1, g_z=g_z, g_h=g_h, g_a=g_a, g_o=g_o, w=w, e=d, dP=dP, dsum=dsum[0], g_y=g_y,
                g_x=g_x, U=U, c=c)


def grad_x(W, x, q, heads):
    """d/dx sum_r cos(model(x), q_r) for one image's tokens x [N, D] (W: float64 state dict, q [Bq, E])."""
    return trace(W, x, q, heads)["g_x"]


TOKENS_PER_BLOCK = 4          # include/mirx.h MIRX_GRADCAM_TOKENS_PER_BLOCK
MINMAX_FLOATS = 1024          # 2 * ceil(MIRX_GRADCAM_MAX_SIZE / 16): a (min, max) pair per 16 output rows


def slot_layout(n, d, heads):
    """The per-image Grad-CAM workspace of libmirx (include/mirx.h), in floats: offsets of
    stats [2n] | P [n heads] | dP [n heads] | dsum [16] | partials [ceil(n / 4) d] | wbar [d] | cam [n] | minmax [1024]
    and "per", the total rounded up to a multiple of 4.  Image i's slot starts at i * per."""
    s = {"stats": 0}
    s["P"] = s["stats"] + 2 * n
    s["dP"] = s["P"] + n * heads
    s["dsum"] = s["dP"] + n * heads
    s["partials"] = s["dsum"] + 16
    s["wbar"] = s["partials"] + (n + TOKENS_PER_BLOCK - 1) // TOKENS_PER_BLOCK * d
    s["cam"] = s["wbar"] + d
    s["minmax"] = s["cam"] + n
    s["per"] = (s["minmax"] + MINMAX_FLOATS + 3) // 4 * 4
    return s


def upsample(m, size):
    """ATen upsample_bilinear2d, align_corners=False, in float64."""
    g = m.shape[0]
    H, W = size
    out = np.empty((H, W))
    for yy in range(H):
        fy = max(g / H * (yy + 0.5) - 0.5, 0.0)
        y0 = int(fy)
        y1 = y0 + (1 if y0 < g - 1 else 0)
        ly = fy - y0
        for xx in range(W):
            fx = max(g / W * (xx + 0.5) - 0.5, 0.0)
            x0 = int(fx)
            x1 = x0 + (1 if x0 < g - 1 else 0)
            lx = fx - x0
            out[yy, xx] = ((1 - ly) * ((1 - lx) * m[y0, x0] + lx * m[y0, x1])
                           + ly * ((1 - lx) * m[y1, x0] + lx * m[y1, x1]))
    return out


def cam_from_grad(x, gx, size):
    cam = np.maximum(x @ gx.mean(0), 0.0)
    cam = np.where(np.isnan(x @ gx.mean(0)), np.nan, cam)
    g = int(np.sqrt(cam.shape[0]))
    up = upsample(cam.reshape(g, g), size)
    lo, hi = up.min(), up.max()
    return (up - lo) / (hi - lo) if hi - lo > 1e-8 else np.zeros_like(up)


def expected(W, x, q, heads, size):
    """[B, H, W] maps of the closed form for tokens x [B, N, D] and query embeddings q [Bq, E]."""
    return np.stack([cam_from_grad(x[i], grad_x(W, x[i], q, heads), size) for i in range(x.shape[0])])
