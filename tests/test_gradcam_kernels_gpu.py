"""Each Grad-CAM kernel (k_gradcam.hip) against float64 *before* the map is normalised ("Bounds").

The final map has passed a ReLU and a min-max normalisation, which hide every positive factor and most small errors.  So the
stages are read back from the workspace (layout: _gradcam_ref.slot_layout, include/mirx.h) and judged one at a time:

  A  mirx_gradcam_pool      stats, P, ybar                              against the float64 forward on the same operands
  B  mirx_gradcam_tokens    dP, dsum, every block partial               on a planted workspace (float64 stats and P, rounded)
  C  mirx_gradcam_finish    wbar, cam, the min / max slots, out         each against float64 of what the stage read
  D  mirx_gradcam_finish    the upsample and numpy's rule alone         on planted partials (d = 1: wbar = 1, cam = relu(x))
  E  guard words around workspace, ybar and out
  F  the vector tail, one entry point at a time (gemv by its index formula, LayerNorm, its backward, GELU, cosine backward)
  G  the assembled wbar and cam against float64 torch autograd through the model's own modules
  H  bits across batch sizes and chunks, NaN containment, per entry point

Every bound comes from reference magnitudes and u = 2^-24 (never from the kernel's output); at every geometry whose lengths
are all <= 257 no bound may exceed 1e-4 of the largest magnitude of the reference it guards (_judge's cap).  Each check prints
achieved error / bound; the worst ratio per stage is printed once more when the module ends."""
import copy
import math
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gradcam_ref as R
from mirx import _lib
from mirx import siglip_gradcam as G
from mirx.model import MedSigLIP, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gradcam_ref.npz")
U = 2.0 ** -24
EPS = 1e-6
CAP = 1e-4
SENTINEL = 0x7FA5A5A5          # a NaN bit pattern no kernel writes
WORST = {}


def gam(k):
    return k * U / (1.0 - k * U)


def wave_depth(d):
    """Roundings on the longest path of a lane-strided sum over d terms and the 6-step butterfly (adding a lane's 0 is exact)."""
    return math.ceil(math.log2(d)) if d <= 64 else -(-d // 64) - 1 + 6


def block_depth(n):
    """The same for a 256-thread workgroup and its 8-step tree."""
    return math.ceil(math.log2(n)) if n <= 256 else -(-n // 256) - 1 + 8


def div_rounds(n):
    """Roundings of a division by n: none by a power of two."""
    return 0 if n & (n - 1) == 0 else 1


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(DEV)


def host(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for stage in sorted(WORST):
        print(f"[gradcam-worst] {stage}: error / bound {WORST[stage]:.4f}")


def _judge(stage, got, ref, bound, cap=True):
    """|got - ref| <= bound everywhere (a NaN fails); the bound itself within CAP of the reference's largest magnitude.  A
    reference that is identically zero must be met exactly."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (stage, got.shape, ref.shape)
    if not np.any(ref):
        bound = np.zeros(ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    top = float(np.abs(ref).max()) if ref.size else 0.0
    print(f"[gradcam] {stage}: error / bound {worst:.4f} (max error {float(np.nanmax(err)):.3e}, max bound "
          f"{float(bound.max()):.3e}, max |ref| {top:.3e})")
    key = stage.split()[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if cap:
        assert float(bound.max()) <= CAP * top, f"{stage}: bound {float(bound.max()):.3e} above the cap {CAP * top:.3e}"
    assert np.all(err <= bound), f"{stage}: error / bound {worst}"


# ---- inputs and the float64 side ---------------------------------------------------------------------------------------
def _tokens(b, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((b, n, d), generator=g) * (1.0 + torch.rand((b, n, 1), generator=g))


def _weights(d, heads, seed, inter=24, p1=32, emb=16):
    """A float64 state dict (float32 values) with the names _gradcam_ref.trace reads, for any n (no tower, no grid)."""
    g = np.random.default_rng(seed)
    mat = lambda o, i: f32(g.standard_normal((o, i)) / math.sqrt(i))          # noqa: E731
    vec = lambda k, base=0.0: f32(base + 0.2 * g.standard_normal(k))           # noqa: E731
    P = "backbone."
    return {P + "post_layernorm.weight": vec(d, 1.0), P + "post_layernorm.bias": vec(d),
            P + "head.probe": f32(0.5 * g.standard_normal((1, 1, d))),
            P + "head.attention.in_proj_weight": mat(3 * d, d), P + "head.attention.in_proj_bias": vec(3 * d),
            P + "head.attention.out_proj.weight": mat(d, d), P + "head.attention.out_proj.bias": vec(d),
            P + "head.layernorm.weight": vec(d, 1.0), P + "head.layernorm.bias": vec(d),
            P + "head.mlp.fc1.weight": mat(inter, d), P + "head.mlp.fc1.bias": vec(inter),
            P + "head.mlp.fc2.weight": mat(d, inter), P + "head.mlp.fc2.bias": vec(d),
            "projection.0.weight": mat(p1, d), "projection.0.bias": vec(p1),
            "projection.1.weight": vec(p1, 1.0), "projection.1.bias": vec(p1),
            "projection.3.weight": mat(emb, p1), "projection.3.bias": vec(emb)}


def _forward64(x, g, be, Um, c):
    mu = x.mean(-1)
    r = 1.0 / np.sqrt(((x - mu[:, None]) ** 2).mean(-1) + EPS)
    xh = (x - mu[:, None]) * r[:, None]
    y = xh * g + be
    S = y @ Um.T + c
    Pm = np.exp(S - S.max(0, keepdims=True))
    Pm = Pm / Pm.sum(0, keepdims=True)
    return SimpleNamespace(mu=mu, r=r, xh=xh, y=y, S=S, P=Pm, ybar=Pm.T @ y)


def _block_sum(a):
    """Rows 4k ... min(4k + 3, n - 1) of a [n, d] summed: the column partial of token block k."""
    nb = -(-a.shape[0] // R.TOKENS_PER_BLOCK)
    return np.stack([a[R.TOKENS_PER_BLOCK * k:R.TOKENS_PER_BLOCK * (k + 1)].sum(0) for k in range(nb)])


class Case:
    """One geometry: tokens, weights, the float64 trace per image and the fp32 operands the kernels are handed (U, c, w, e
    are the float64 values rounded once; the float64 side then starts from the rounded values, so it reads what the kernel
    reads)."""

    def __init__(self, n, d, heads, b):
        self.n, self.d, self.heads, self.b = n, d, heads, b
        self.capped = max(n, d) <= 257
        self.W = _weights(d, heads, 100 + n + d)
        self.x = _tokens(b, n, d, 3)
        self.x64 = self.x.double().numpy()
        q = torch.randn((2, 16), generator=torch.Generator().manual_seed(8))
        self.q64 = F.normalize(q, dim=1).double().numpy()
        self.tr = [R.trace(self.W, self.x64[i], self.q64, heads) for i in range(b)]
        self.g, self.be = self.W["backbone.post_layernorm.weight"], self.W["backbone.post_layernorm.bias"]
        self.U, self.c = f32(self.tr[0]["U"]), f32(self.tr[0]["c"])
        self.w = np.stack([f32(t["w"]) for t in self.tr])
        self.e = np.stack([f32(t["e"]) for t in self.tr])
        self.fw = [_forward64(self.x64[i], self.g, self.be, self.U, self.c) for i in range(b)]
        self.sl = R.slot_layout(n, d, heads)
        # _forward64 is trace's forward: the same numbers from the unrounded U, c
        f0 = _forward64(self.x64[0], self.g, self.be, self.tr[0]["U"], self.tr[0]["c"])
        for k in ("mu", "r", "y", "S", "P", "ybar"):
            assert np.allclose(getattr(f0, k), self.tr[0][k], rtol=1e-12, atol=1e-14), k

    def device(self):
        if not hasattr(self, "_dev"):
            self._dev = SimpleNamespace(x=self.x.to(DEV), g=dev(self.g), be=dev(self.be), U=dev(self.U), c=dev(self.c),
                                        w=dev(self.w), e=dev(self.e))
        return self._dev

    def workspace(self):
        return torch.zeros((self.b * self.sl["per"],), dtype=torch.float32, device=DEV)

    def region(self, ws, i, name, count):
        o = i * self.sl["per"] + self.sl[name]
        return ws[o:o + count]


GEOMS = [(1, 1, 1, 3), (3, 7, 7, 3), (4, 7, 1, 3), (6, 48, 3, 3), (7, 40, 5, 3), (9, 48, 3, 3), (25, 64, 4, 3), (49, 40, 5, 3),
         (121, 256, 16, 3), (257, 96, 2, 3), (1024, 1152, 16, 1)]
SQUARE = [g for g in GEOMS if int(round(g[0] ** 0.5)) ** 2 == g[0]]


@lru_cache(maxsize=None)
def case(n, d, heads, b):
    return Case(n, d, heads, b)


# ---- the raw entry points (the wrappers of siglip_gradcam allocate their outputs; the guard tests must not) ---------------
def _opt(t):
    return None if t is None else _ptr(t)


def pool(x, g, be, Um, c, ws, ybar=None, eps=EPS):
    b, n, d = x.shape
    if ybar is None:
        ybar = torch.empty((b, Um.shape[0], d), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mirx_gradcam_pool(_ptr(x), b, n, d, Um.shape[0], _ptr(g), _ptr(be), float(eps), _ptr(Um), _ptr(c), _ptr(ws),
                                             ws.numel(), _ptr(ybar), _stream(DEV)), "mirx_gradcam_pool")
    return ybar


def tokens(x, g, be, Um, w, e, ws):
    b, n, d = x.shape
    _lib.check(_lib.load().mirx_gradcam_tokens(_ptr(x), b, n, d, Um.shape[0], _ptr(g), _ptr(be), _ptr(Um), _ptr(w), _ptr(e), _ptr(ws),
                                               ws.numel(), _stream(DEV)), "mirx_gradcam_tokens")


def finish(x, heads, ws, H, W, out=None):
    b, n, d = x.shape
    if out is None:
        out = torch.empty((b, H, W), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().mirx_gradcam_finish(_ptr(x), b, n, d, heads, _ptr(ws), ws.numel(), H, W, _ptr(out), _stream(DEV)),
               "mirx_gradcam_finish")
    return out


def gemv(A, lda, x, xs, bias, res, rs, out, os_, b, m, k, mg, rmod, acol, xg):
    _lib.check(_lib.load().mirx_gradcam_gemv(_ptr(A), lda, _ptr(x), xs, _opt(bias), _opt(res), rs, _ptr(out), os_, b, m, k, mg, rmod,
                                             acol, xg, _stream(DEV)), "mirx_gradcam_gemv")
    return out


def chain(cs, ws, ybar=None):
    """pool -> tokens (w, e: the float64 reference values, rounded) on the case's tokens; the workspace is left filled."""
    dv = cs.device()
    ybar = pool(dv.x, dv.g, dv.be, dv.U, dv.c, ws, ybar)
    tokens(dv.x, dv.g, dv.be, dv.U, dv.w, dv.e, ws)
    return ybar


# ---- A: mirx_gradcam_pool ----------------------------------------------------------------------------------------------
def pool_bounds(cs, i):
    """DESIGN 21 "Bounds": stats, the scores' error, the softmax and the pooled tokens, from the float64 forward alone."""
    x, f, n, d = cs.x64[i], cs.fw[i], cs.n, cs.d
    ld = wave_depth(d)
    var = ((x - f.mu[:, None]) ** 2).mean(-1)
    e_mu = gam(ld + div_rounds(d)) * np.abs(x).mean(-1)
    rho_r = gam(ld + 8) + e_mu ** 2 / (var + EPS)
    e_y = np.abs(cs.g) * (e_mu[:, None] * f.r[:, None] + np.abs(f.xh) * (rho_r[:, None] + 3 * U)) + U * np.abs(f.y)
    e_s = e_y @ np.abs(cs.U).T + gam(ld + 2) * (np.abs(f.y) @ np.abs(cs.U).T + np.abs(cs.c))
    eps_h = e_s.max(0) + U * np.abs(f.S - f.S.max(0, keepdims=True)).max(0)
    rho_p = np.expm1(2 * eps_h) + gam(block_depth(n) + 6)
    e_ybar = (f.P * (rho_p + gam(-(-n // 4) + 4))).T @ np.abs(f.y) + f.P.T @ e_y
    # the bound test_pool_kernel_matches_float64 asserts: the one above is never looser
    A = (np.abs(f.y) @ np.abs(cs.U).T).max()
    old = (d + n + 16) * U * (2 * A + 1) * np.abs(f.y).max()
    return SimpleNamespace(mu=e_mu, r=f.r * rho_r, P=f.P * rho_p, ybar=e_ybar, ybar_old=old)


@pytest.mark.parametrize("n,d,heads,b", GEOMS)
def test_pool_stage_by_stage(n, d, heads, b):
    cs = case(n, d, heads, b)
    dv, ws = cs.device(), cs.workspace()
    ybar = host(pool(dv.x, dv.g, dv.be, dv.U, dv.c, ws))
    wsh = host(ws)
    tag = f"n={n} d={d} heads={heads}"
    for i in range(b):
        f, bd = cs.fw[i], pool_bounds(cs, i)
        st = cs.region(wsh, i, "stats", 2 * n).reshape(n, 2)
        _judge(f"stats.mean {tag}", st[:, 0], f.mu, bd.mu, cap=False)        # a mean near 0 is not a small output: x is the scale
        assert float(bd.mu.max()) <= (CAP * np.abs(cs.x64[i]).max() if cs.capped else np.inf)
        _judge(f"stats.rstd {tag}", st[:, 1], f.r, bd.r, cap=cs.capped)
        Pd = cs.region(wsh, i, "P", n * heads).reshape(n, heads)
        _judge(f"softmax {tag}", Pd, f.P, bd.P, cap=cs.capped)
        assert float(np.abs(Pd.sum(0) - 1.0).max()) <= n * U
        assert float(bd.ybar.max()) <= bd.ybar_old
        _judge(f"ybar {tag}", ybar[i], f.ybar, bd.ybar, cap=cs.capped)
    if not cs.capped:
        print(f"[gradcam] full size: bounds relative to max |ref|: rstd {float((bd.r / f.r).max()):.2e}, P "
              f"{float(bd.P.max() / f.P.max()):.2e}, ybar {float(bd.ybar.max() / np.abs(f.ybar).max()):.2e}")


# ---- B: mirx_gradcam_tokens on a planted workspace ---------------------------------------------------------------------------
def tokens_reference(cs, i):
    """What mirx_gradcam_tokens must leave for image i when the workspace holds (mu, r, P) = the float64 forward rounded to
    fp32: dP, dsum and the block partials in float64 from those rounded values, with their bounds."""
    x, n, d, heads = cs.x64[i], cs.n, cs.d, cs.heads
    f = cs.fw[i]
    mu, r, Pm = f32(f.mu), f32(f.r), f32(f.P)
    g, be, Um, w, e = cs.g, cs.be, cs.U, cs.w[i], cs.e[i]
    xh = (x - mu[:, None]) * r[:, None]
    y = xh * g + be
    dP = y @ w.T + e
    dsum = (Pm * dP).sum(0)
    a = Pm * (dP - dsum)
    gy = a @ Um + Pm @ w
    gh = g * gy
    mg, mgx = gh.mean(-1, keepdims=True), (gh * xh).mean(-1, keepdims=True)
    gx = r[:, None] * ((gh - mg) - xh * mgx)
    ld, rc = wave_depth(d), r[:, None]
    e_xh = 2 * U * np.abs(xh)
    e_y = 3 * U * np.abs(g * xh) + U * np.abs(y)
    e_dp = e_y @ np.abs(w).T + gam(ld + 2) * (np.abs(y) @ np.abs(w).T + np.abs(e))
    e_dsum = (Pm * e_dp).sum(0) + gam(block_depth(n) + 1) * np.abs(Pm * dP).sum(0)
    e_a = Pm * (e_dp + e_dsum) + 2 * U * Pm * (np.abs(dP) + np.abs(dsum))
    e_gy = e_a @ np.abs(Um) + gam(2 * heads + 1) * (np.abs(a) @ np.abs(Um) + Pm @ np.abs(w))
    e_gh = np.abs(g) * e_gy + U * np.abs(gh)
    e_mg = e_gh.mean(-1, keepdims=True) + gam(ld + 1) * np.abs(gh).mean(-1, keepdims=True)
    e_mgx = (e_gh * np.abs(xh) + np.abs(gh) * e_xh).mean(-1, keepdims=True) + gam(ld + 2) * np.abs(gh * xh).mean(-1, keepdims=True)
    e_gx = rc * (e_gh + e_mg + e_xh * np.abs(mgx) + np.abs(xh) * e_mgx) + gam(4) * rc * (np.abs(gh) + np.abs(mg) + np.abs(xh * mgx))
    e_part = _block_sum(e_gx) + gam(4) * _block_sum(np.abs(gx))
    return SimpleNamespace(stats=np.stack([mu, r], 1), P=Pm, dP=dP, dsum=dsum, gx=gx, parts=_block_sum(gx), e_dP=e_dp,
                           e_dsum=e_dsum, e_parts=e_part)


@pytest.mark.parametrize("n,d,heads,b", GEOMS)
def test_tokens_stage_by_stage(n, d, heads, b):
    cs = case(n, d, heads, b)
    dv, ws = cs.device(), cs.workspace()
    refs = [tokens_reference(cs, i) for i in range(b)]
    # the reference's g_x is trace's: the same formula on the unrounded operands
    assert np.allclose(refs[0].gx, cs.tr[0]["g_x"], rtol=1e-3, atol=1e-5 * np.abs(cs.tr[0]["g_x"]).max())
    for i, rf in enumerate(refs):
        cs.region(ws, i, "stats", 2 * n).copy_(dev(rf.stats.reshape(-1)))
        cs.region(ws, i, "P", n * heads).copy_(dev(rf.P.reshape(-1)))
    tokens(dv.x, dv.g, dv.be, dv.U, dv.w, dv.e, ws)
    wsh = host(ws)
    tag = f"n={n} d={d} heads={heads}"
    nb = -(-n // 4)
    for i, rf in enumerate(refs):
        _judge(f"dP {tag}", cs.region(wsh, i, "dP", n * heads).reshape(n, heads), rf.dP, rf.e_dP, cap=cs.capped)
        _judge(f"dsum {tag}", cs.region(wsh, i, "dsum", heads), rf.dsum, rf.e_dsum, cap=cs.capped)
        _judge(f"partials {tag}", cs.region(wsh, i, "partials", nb * d).reshape(nb, d), rf.parts, rf.e_parts, cap=cs.capped)
        assert np.array_equal(cs.region(wsh, i, "stats", 2 * n), rf.stats.reshape(-1))          # read, not written
        assert np.array_equal(cs.region(wsh, i, "P", n * heads), rf.P.reshape(-1))
    if not cs.capped:
        rf = refs[-1]
        print(f"[gradcam] full size: bounds relative to max |ref|: dP {float(rf.e_dP.max() / np.abs(rf.dP).max()):.2e}, dsum "
              f"{float(rf.e_dsum.max() / np.abs(rf.dsum).max()):.2e}, partials {float(rf.e_parts.max() / np.abs(rf.parts).max()):.2e}")


# ---- C: mirx_gradcam_finish on a real workspace --------------------------------------------------------------------------
def _sizes(g):
    s = [(g, g), (35, 35), (33, 40), (40, 33), (1, 1), (17, 16)]
    return s + [(g - 1, 2 * g + 1)] if g > 1 else s


def upsample_bound(g, cam, size=None):
    """|device bilinear - float64 bilinear| of a grid: the fp32 source index errs by at most 3 u g per axis, which moves the
    value by that times the spread of the taps; five roundings in the blend.  With a size: per output pixel, from the largest
    magnitude among its taps and their neighbours (the fp32 index may fall one cell to either side of the float64 one)."""
    if size is None:
        return (8 * g + 6) * U * float(np.abs(cam).max())
    m = np.abs(np.asarray(cam, dtype=np.float64).reshape(g, g))
    pad = np.pad(m, 1, mode="edge")
    near = np.max([pad[1 + dy:1 + dy + g, 1 + dx:1 + dx + g] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    y0 = np.maximum(g / size[0] * (np.arange(size[0]) + 0.5) - 0.5, 0.0).astype(int)
    x0 = np.maximum(g / size[1] * (np.arange(size[1]) + 0.5) - 0.5, 0.0).astype(int)
    y1, x1 = np.minimum(y0 + 1, g - 1), np.minimum(x0 + 1, g - 1)
    return (8 * g + 6) * U * np.maximum(np.maximum(near[y0][:, x0], near[y0][:, x1]), np.maximum(near[y1][:, x0], near[y1][:, x1]))


def judge_finish(tag, slot, x, sl, n, d, H, W, out, capped):
    """One image's wbar, cam, min / max slots and map, each against float64 of what that stage read from the device."""
    g = int(round(n ** 0.5))
    nb = -(-n // 4)
    parts = slot[sl["partials"]:sl["partials"] + nb * d].reshape(nb, d)
    wbar = slot[sl["wbar"]:sl["wbar"] + d]
    cam = slot[sl["cam"]:sl["cam"] + n]
    _judge(f"wbar {tag}", wbar, parts.sum(0) / n, gam(nb + 1) * np.abs(parts).sum(0) / n, cap=capped)
    _judge(f"cam {tag}", cam, np.maximum(x @ wbar, 0.0), gam(wave_depth(d) + 1) * (np.abs(x) @ np.abs(wbar)), cap=capped)
    up = R.upsample(cam.reshape(g, g), (H, W))
    e_up = upsample_bound(g, cam)
    nblk = -(-H // 16)
    mm = slot[sl["minmax"]:sl["minmax"] + 2 * nblk].reshape(nblk, 2)
    ref_mm = np.stack([[up[16 * k:16 * k + 16].min(), up[16 * k:16 * k + 16].max()] for k in range(nblk)])
    e_px = upsample_bound(g, cam, (H, W))
    _judge(f"minmax {tag}", mm, ref_mm, np.stack([[e_px[16 * k:16 * k + 16].max()] * 2 for k in range(nblk)]), cap=capped)
    lo, hi = up.min(), up.max()
    assert hi - lo == 0.0 or hi - lo > 1e-6, "the input sits at numpy's 1e-8 threshold"
    if hi - lo > 1e-8:
        _judge(f"map {tag}", out, (up - lo) / (hi - lo), 4 * e_up / (hi - lo) + 2 * U, cap=capped)
        assert float(out.max()) == 1.0 and float(out.min()) == 0.0
    else:
        assert np.all(out == 0)


@pytest.mark.parametrize("n,d,heads,b", SQUARE)
def test_finish_on_a_real_workspace(n, d, heads, b):
    cs = case(n, d, heads, b)
    dv, ws = cs.device(), cs.workspace()
    chain(cs, ws)
    before = host(ws)
    for H, W in _sizes(int(round(n ** 0.5))):
        out = host(finish(dv.x, heads, ws, H, W))
        wsh = host(ws)
        for i in range(b):
            slot = wsh[i * cs.sl["per"]:(i + 1) * cs.sl["per"]]
            judge_finish(f"n={n} d={d} {H}x{W}", slot, cs.x64[i], cs.sl, n, d, H, W, out[i], cs.capped)
            o = i * cs.sl["per"]
            assert np.array_equal(wsh[o:o + cs.sl["wbar"]], before[o:o + cs.sl["wbar"]])       # stats ... partials: read only


# ---- D: mirx_gradcam_finish on a planted workspace -----------------------------------------------------------------------
def planted_finish(cam, H, W):
    """cam [b, g, g] (float32) driven through wbar = 1: d = 1, block 0's partial = n, the others 0 -> (out, workspace)."""
    b, g = cam.shape[0], cam.shape[1]
    n = g * g
    sl = R.slot_layout(n, 1, 1)
    ws = torch.zeros((b * sl["per"],), dtype=torch.float32, device=DEV)
    for i in range(b):
        ws[i * sl["per"] + sl["partials"]] = float(n)
    x = torch.from_numpy(np.ascontiguousarray(cam, dtype=np.float32).reshape(b, n, 1)).to(DEV)
    out = finish(x, 1, ws, H, W)
    wsh = host(ws)
    for i in range(b):
        assert wsh[i * sl["per"] + sl["wbar"]] == 1.0
    return out.cpu().numpy(), wsh, sl


def _pattern(g, hi, seed=0):
    """A g x g grid of {0, hi} with both values present."""
    m = (np.random.default_rng(seed).random((g, g)) < 0.5).astype(np.float32)
    m[0, 0], m[g - 1, g - 1] = 0.0, 1.0
    return m * np.float32(hi)


def test_normalise_rule_on_planted_maps():
    g = 5
    tiny = np.float32(1e-8)
    cams = {"2^-26": _pattern(g, 2.0 ** -26, 1), "2^-27": _pattern(g, 2.0 ** -27, 2), "1e-8": _pattern(g, tiny, 3),
            "next(1e-8)": _pattern(g, np.nextafter(tiny, np.float32(1)), 4), "constant": np.full((g, g), 0.75, np.float32),
            "negative": -1.0 - _pattern(g, 2.0, 5), "plain": np.random.default_rng(6).random((g, g)).astype(np.float32)}
    names = list(cams)
    x = np.stack([cams[k] for k in names])
    out, _, _ = planted_finish(x, g, g)
    for i, k in enumerate(names):
        cam = np.maximum(x[i], np.float32(0))                     # H = W = g: the bilinear weights are exactly 0 / 1
        exp = G._normalise01(cam)
        assert exp.dtype == np.float32 and np.array_equal(out[i], exp), k
    assert set(np.unique(out[names.index("2^-26")])) == {0.0, 1.0}
    assert set(np.unique(out[names.index("next(1e-8)")])) == {0.0, 1.0}
    for k in ("2^-27", "1e-8", "constant", "negative"):
        assert not out[names.index(k)].any(), k
    assert out[names.index("plain")].max() == 1.0


def test_nan_token_on_planted_maps():
    g = 5
    x = np.random.default_rng(7).standard_normal((3, g, g)).astype(np.float32)
    clean, _, _ = planted_finish(x, g, g)
    x[1, 2, 3] = np.nan
    dirty, _, _ = planted_finish(x, g, g)
    assert not dirty[1].any() and clean[1].any()
    assert np.array_equal(dirty[0], clean[0]) and np.array_equal(dirty[2], clean[2])
    assert np.array_equal(clean[0], G._normalise01(np.maximum(x[0], np.float32(0))))


@pytest.mark.parametrize("H,W", [(8192, 1), (1, 8192)])
def test_last_minmax_slot(H, W):
    cam = np.array([[[0.25, 1.0], [0.5, 2.0]]], dtype=np.float32)
    out, wsh, sl = planted_finish(cam, H, W)
    up = R.upsample(cam[0].astype(np.float64), (H, W))
    e_up = upsample_bound(2, cam)
    nblk = -(-H // 16)
    assert 2 * nblk <= R.MINMAX_FLOATS and (H != 8192 or 2 * nblk == R.MINMAX_FLOATS)
    mm = wsh[sl["minmax"]:sl["minmax"] + 2 * nblk].reshape(nblk, 2)
    ref_mm = np.stack([[up[16 * k:16 * k + 16].min(), up[16 * k:16 * k + 16].max()] for k in range(nblk)])
    _judge(f"minmax planted {H}x{W}", mm, ref_mm, e_up)
    lo, hi = up.min(), up.max()
    _judge(f"map planted {H}x{W}", out[0], (up - lo) / (hi - lo), 4 * e_up / (hi - lo) + 2 * U)


# ---- E: guard words ----------------------------------------------------------------------------------------------------
def guarded(count):
    raw = torch.full((count + 128,), SENTINEL, dtype=torch.int32, device=DEV)
    return raw, raw.view(torch.float32)[64:64 + count]


def intact(raw):
    return bool((raw[:64] == SENTINEL).all()) and bool((raw[-64:] == SENTINEL).all())


@pytest.mark.parametrize("n,d,heads,b", [(7, 40, 5, 3), (25, 64, 4, 3)])
def test_guard_words_around_the_chain(n, d, heads, b):
    cs = case(n, d, heads, b)
    dv = cs.device()
    raw_ws, ws = guarded(b * cs.sl["per"])
    raw_y, ybar = guarded(b * heads * d)
    assert ws.is_contiguous() and ws.numel() == G.workspace_floats(b, n, d, heads)
    chain(cs, ws, ybar.view(b, heads, d))
    torch.cuda.synchronize()
    assert intact(raw_ws) and intact(raw_y)
    assert not torch.isnan(ybar).any()                           # every word of ybar was written
    if int(round(n ** 0.5)) ** 2 != n:
        with pytest.raises(_lib.MirxError):
            finish(dv.x, heads, ws, 35, 35)
        return
    for H, W in ((35, 35), (33, 40), (1, 1)):
        raw_o, out = guarded(b * H * W)
        finish(dv.x, heads, ws, H, W, out.view(b, H, W))
        torch.cuda.synchronize()
        assert intact(raw_ws) and intact(raw_o) and not torch.isnan(out).any()


def test_guard_words_at_the_last_minmax_slot():
    n, H, W = 4, 8192, 1
    sl = R.slot_layout(n, 1, 1)
    raw_ws, ws = guarded(sl["per"])
    ws.zero_()
    ws[sl["partials"]] = float(n)
    raw_o, out = guarded(H * W)
    x = torch.tensor([0.25, 1.0, 0.5, 2.0], device=DEV).view(1, n, 1)
    finish(x, 1, ws, H, W, out.view(1, H, W))
    torch.cuda.synchronize()
    assert intact(raw_ws) and intact(raw_o) and not torch.isnan(out).any()
    assert float(ws[sl["minmax"] + R.MINMAX_FLOATS - 1]) > 0.0   # the last slot's max was written


# ---- F: the vector tail ------------------------------------------------------------------------------------------------
def gemv_formula(A, lda, x, xs, bias, res, rs, b, m, k, mg, rmod, acol, xg):
    """include/mirx.h, literally: out[i, j] = sum_t A[(j % rmod) * lda + (j / mg) * acol + t] * x[i * xs + (j / mg) * xg + t]
    (+ bias[j]) (+ res[i * rs + j]) on the flat buffers, and the sum of magnitudes that scales the bound."""
    A, x = A.reshape(-1), x.reshape(-1)
    j, t = np.arange(m), np.arange(k)
    ia = ((j % rmod) * lda + (j // mg) * acol)[:, None] + t[None, :]
    out, mag = np.empty((b, m)), np.empty((b, m))
    for i in range(b):
        ix = (i * xs + (j // mg) * xg)[:, None] + t[None, :]
        out[i] = (A[ia] * x[ix]).sum(1)
        mag[i] = np.abs(A[ia] * x[ix]).sum(1)
        if bias is not None:
            out[i] += bias
            mag[i] += np.abs(bias)
        if res is not None:
            rr = res.reshape(-1)[i * rs + j]
            out[i] += rr
            mag[i] += np.abs(rr)
    return out, mag


def run_gemv(tag, A, lda, x, xs, bias, res, rs, os_, b, m, k, mg, rmod, acol, xg, cap):
    """Launch on fp32 copies, judge against the formula within gamma_{k+3} of the magnitudes; the out rows' padding stays.
    The formula runs first: an index past a buffer raises here, before anything is launched."""
    ref, mag = gemv_formula(A, lda, x, xs, bias, res, rs, b, m, k, mg, rmod, acol, xg)
    raw = torch.full((b * os_ + 128,), SENTINEL, dtype=torch.int32, device=DEV)
    out = raw.view(torch.float32)[64:64 + b * os_]
    gemv(dev(A), lda, dev(x), xs, None if bias is None else dev(bias), None if res is None else dev(res), rs, out, os_, b, m, k,
         mg, rmod, acol, xg)
    torch.cuda.synchronize()
    got = out.view(b, os_)
    assert intact(raw) and bool((raw[64:64 + b * os_].view(b, os_)[:, m:] == SENTINEL).all())
    _judge(f"gemv {tag}", host(got[:, :m]), ref, gam(k + 3) * mag, cap=cap)
    return ref


@pytest.mark.parametrize("m,k", [(1, 1), (5, 63), (7, 64), (6, 65), (130, 200)])
@pytest.mark.parametrize("b", [1, 3])
def test_gemv_plain(m, k, b):
    g = np.random.default_rng(1000 * m + k)
    A, bias = f32(g.standard_normal((m, k))), f32(g.standard_normal(m))
    for xs, os_, rs in ((k, m, m), (k + 3, m + 5, m + 2)):
        x, res = f32(g.standard_normal((b, xs))), f32(g.standard_normal((b, rs)))
        for use_bias, use_res in ((False, False), (True, False), (False, True), (True, True)):
            ref = run_gemv(f"plain m={m} k={k} b={b} xs={xs} bias={use_bias} res={use_res}", A, k, x, xs, bias if use_bias else None,
                           res if use_res else None, rs, os_, b, m, k, m, m, 0, 0, cap=True)
            plain = x[:, :k] @ A.T + (bias if use_bias else 0.0) + (res[:, :m] if use_res else 0.0)
            assert np.allclose(ref, plain, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("heads,dh", [(3, 16), (5, 8), (16, 72)])
def test_gemv_grouped_forms(heads, dh):
    """The three grouped calls of gradcam_from_tokens, by the formula and by the per-head products they stand for."""
    d, b = heads * dh, 3
    g = np.random.default_rng(heads * 100 + dh)
    wv, bv = f32(g.standard_normal((d, d)) / math.sqrt(d)), f32(g.standard_normal(d))
    ybar, g_o = f32(g.standard_normal((b, heads, d))), f32(g.standard_normal((b, d)))
    wvT = np.ascontiguousarray(wv.T)
    hs = [slice(h * dh, (h + 1) * dh) for h in range(heads)]
    o = run_gemv(f"grouped o heads={heads} dh={dh}", wv, d, ybar, heads * d, bv, None, d, d, b, d, d, dh, d, 0, d, cap=d <= 257)
    assert np.allclose(o, np.stack([np.concatenate([wv[s] @ ybar[i, h] for h, s in enumerate(hs)]) + bv for i in range(b)]),
                       rtol=1e-12, atol=1e-12)
    w = run_gemv(f"grouped w heads={heads} dh={dh}", wvT, d, g_o, d, None, None, heads * d, heads * d, b, heads * d, dh, d, d, dh, dh,
                 cap=True)
    assert np.allclose(w.reshape(b, heads, d), np.stack([np.stack([wv[s].T @ g_o[i, s] for s in hs]) for i in range(b)]),
                       rtol=1e-12, atol=1e-12)
    e = run_gemv(f"grouped e heads={heads} dh={dh}", bv, 0, g_o, d, None, None, heads, heads, b, heads, dh, 1, 1, dh, dh, cap=True)
    assert np.allclose(e, np.stack([[g_o[i, s] @ bv[s] for s in hs] for i in range(b)]), rtol=1e-12, atol=1e-12)


LENGTHS = [1, 2, 255, 256, 257, 1000, 8192]


def _rows(length, seed):
    """Three rows: scale 1, scale 3 with offset 2, and (past the capped lengths) mean 1e3 with std 1, whose fp32 mean alone
    errs by gamma * 1e3.  Two elements normalise to +-1 whatever they are unless their spread is near sqrt(eps): the backward
    would be a pure cancellation, so those rows are c +- delta with delta^2 about eps."""
    g = np.random.default_rng(seed)
    if length == 2:
        return f32(0.1 * g.standard_normal((3, 1)) + 4e-3 * (1.0 + g.random((3, 1))) * np.array([[1.0, -1.0]]))
    v = g.standard_normal((3, length))
    v[1] = 2.0 + 3.0 * v[1]
    v[2] = (1e3 + v[2]) if length > 257 else (3.0 + v[2])
    return f32(v)


def _affine(length, seed):
    g = np.random.default_rng(seed)
    return f32(1.0 + 0.2 * g.standard_normal(length)), f32(0.2 * g.standard_normal(length))


def layernorm_bounds(v, gamma, beta, eps):
    length = v.shape[1]
    bd = block_depth(length)
    mu = v.mean(-1)
    var = ((v - mu[:, None]) ** 2).mean(-1)
    r = 1.0 / np.sqrt(var + eps)
    xh = (v - mu[:, None]) * r[:, None]
    y = xh * gamma + beta
    e_mu = gam(bd + div_rounds(length)) * np.abs(v).mean(-1)
    rho_r = gam(bd + 8) + e_mu ** 2 / (var + eps)
    e_y = np.abs(gamma) * (e_mu[:, None] * r[:, None] + np.abs(xh) * (rho_r[:, None] + 3 * U)) + U * np.abs(y)
    return SimpleNamespace(mu=mu, r=r, y=y, e_mu=e_mu, e_r=r * rho_r, e_y=e_y)


@pytest.mark.parametrize("length,eps", [(n, e) for n in LENGTHS for e in (1e-6, 1e-5, 0.0) if n > 1 or e > 0])   # eps = 0: no constant row
def test_layernorm(length, eps):
    v = _rows(length, 40 + length)
    gamma, beta = _affine(length, 41 + length)
    bd = layernorm_bounds(v, gamma, beta, float(np.float32(eps)))
    ln = SimpleNamespace(weight=dev(gamma), bias=dev(beta), eps=eps)
    capped = length <= 257
    for relu in (False, True):
        out, st = G._ln(dev(v), ln, relu=relu)
        st = host(st)
        tag = f"len={length} eps={eps:g} relu={int(relu)}"
        _judge(f"layernorm.mean {tag}", st[:, 0], bd.mu, bd.e_mu, cap=False)
        assert not capped or float(bd.e_mu.max()) <= CAP * np.abs(v).max()
        _judge(f"layernorm.rstd {tag}", st[:, 1], bd.r, bd.e_r, cap=capped)
        _judge(f"layernorm.out {tag}", host(out), np.maximum(bd.y, 0.0) if relu else bd.y, bd.e_y, cap=capped)
    if not capped:
        print(f"[gradcam] len={length}: out bound / max |out| {float(bd.e_y.max() / np.abs(bd.y).max()):.2e}")


def test_layernorm_relu_keeps_nan():
    v = _rows(64, 44)
    v[1, 5] = np.nan
    gamma, beta = _affine(64, 45)
    ln = SimpleNamespace(weight=dev(gamma), bias=dev(beta), eps=1e-5)
    for relu in (False, True):
        out, st = G._ln(dev(v), ln, relu=relu)
        out, st = host(out), host(st)
        assert np.isnan(out[1]).all() and np.isnan(st[1]).all()
        assert not np.isnan(out[[0, 2]]).any() and not np.isnan(st[[0, 2]]).any()
        clean, _ = G._ln(dev(v[[0, 2]]), ln, relu=relu)
        assert np.array_equal(out[[0, 2]], host(clean))


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("use_after,use_res", [(False, False), (True, False), (False, True), (True, True)])
def test_layernorm_backward(length, use_after, use_res):
    """Against float64 torch autograd of sum g * relu?(layer_norm(v)): not the restatement's _ln_bwd.  The kernel is handed
    the float64 stats rounded to fp32; `after` carries the forward's positives, and exact zeros and negatives elsewhere."""
    eps = 1e-5
    v = _rows(length, 50 + length)
    gamma, beta = _affine(length, 51 + length)
    rng = np.random.default_rng(52 + length)
    g, res = f32(rng.standard_normal(v.shape)), f32(rng.standard_normal(v.shape))
    vt = torch.from_numpy(v).requires_grad_(True)
    y = F.layer_norm(vt, (length,), torch.from_numpy(gamma), torch.from_numpy(beta), eps)
    (ref,) = torch.autograd.grad((torch.from_numpy(g) * (torch.relu(y) if use_after else y)).sum(), vt)
    ref = ref.numpy() + (res if use_res else 0.0)
    yn = y.detach().numpy()
    after = f32(yn)
    off = np.flatnonzero(yn.reshape(-1) <= 0)
    after.reshape(-1)[off[::2]] = 0.0                               # exact zeros; the other non-positives stay negative
    assert not use_after or length < 8 or ((after == 0).any() and (after < 0).any() and ((after > 0) == (yn > 0)).all())
    # bound: the stats' rounding moves xhat; then the two means and four roundings per output
    mu = v.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(((v - mu) ** 2).mean(-1, keepdims=True) + eps)
    xh = (v - mu) * r
    gh = gamma * g * ((yn > 0) if use_after else 1.0)
    mg, mgx = gh.mean(-1, keepdims=True), (gh * xh).mean(-1, keepdims=True)
    bd = block_depth(length)
    e_xh = r * U * np.abs(mu) + 3 * U * np.abs(xh)
    e_gh = U * np.abs(gh)
    e_mg = e_gh.mean(-1, keepdims=True) + gam(bd + 1) * np.abs(gh).mean(-1, keepdims=True)
    e_mgx = (e_gh * np.abs(xh) + np.abs(gh) * e_xh).mean(-1, keepdims=True) + gam(bd + 2) * np.abs(gh * xh).mean(-1, keepdims=True)
    core = r * ((gh - mg) - xh * mgx)
    bound = (r * (e_gh + e_mg + e_xh * np.abs(mgx) + np.abs(xh) * e_mgx) + gam(5) * r * (np.abs(gh) + np.abs(mg) + np.abs(xh * mgx))
             + (U * (np.abs(res) + np.abs(core)) if use_res else 0.0))
    if length == 1:                  # xhat = 0 and ghat - mean(ghat) = 0 in any precision: the result is res (or 0) exactly
        assert np.abs(ref - (res if use_res else 0.0)).max() <= 1e-9
        ref, bound = (res if use_res else np.zeros_like(v)), np.zeros_like(v)
    assert np.allclose(core + (res if use_res else 0.0), ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
    ln = SimpleNamespace(weight=dev(gamma), bias=dev(beta), eps=eps)
    got = G._ln_bwd(dev(g), dev(v), dev(np.concatenate([mu, r], 1)), ln, after=dev(after) if use_after else None,
                    res=dev(res) if use_res else None)
    _judge(f"layernorm_bwd len={length} after={int(use_after)} res={int(use_res)}", host(got), ref, bound, cap=length <= 257)
    if length > 257:
        print(f"[gradcam] len={length}: layernorm_bwd bound / max |ref| {float(bound.max() / np.abs(ref).max()):.2e}")


def _gelu_points():
    g = torch.Generator().manual_seed(60)
    special = torch.tensor([0.0, 1e-8, -1e-8, 30.0, -30.0], dtype=torch.float64)
    h = torch.cat([torch.linspace(-12, 12, 4097, dtype=torch.float64), torch.randn(4096, generator=g).double(), special])
    return h.float()


def _gelu_units(h32, g32, mode, fn):
    """Error of fn's fp32 result against float64 autograd / F.gelu, in units of u max(1, |h|) |g| (mode 0: g = 1)."""
    h64 = h32.double().requires_grad_(True)
    y = F.gelu(h64, approximate="tanh")
    if mode == 0:
        ref, scale = y.detach(), torch.clamp(h32.double().abs(), min=1.0)
    else:
        (ref,) = torch.autograd.grad((y * g32.double()).sum(), h64)
        scale = torch.clamp(h32.double().abs(), min=1.0) * g32.double().abs()
    err = (fn().double() - ref).abs()
    units = torch.where(err == 0, torch.zeros_like(err), err / (U * scale))
    return float(units.max())


@pytest.mark.parametrize("mode", [0, 1])
def test_gelu(mode):
    """The kernel may err 4 x what torch's CPU fp32 evaluation of the same formula errs on the same points (at least 4 units):
    the margin for a device tanhf a few ulp worse than the host's."""
    pts = _gelu_points()
    worst_host, worst_dev = 0.0, 0.0
    runs = []
    for count in (1, 255, 256, 257, 100003):
        gen = torch.Generator().manual_seed(61 + count)
        h = pts[torch.randperm(pts.numel(), generator=gen)].repeat(-(-count // pts.numel()))[:count].contiguous()
        if count == 100003:
            h = torch.cat([pts, h[pts.numel():]])                     # every point at least once
        g = torch.randn(count, generator=gen)
        g[::97] = 0.0

        def on_host(h=h, g=g):
            if mode == 0:
                return F.gelu(h, approximate="tanh")
            hh = h.clone().requires_grad_(True)
            return torch.autograd.grad((F.gelu(hh, approximate="tanh") * g).sum(), hh)[0]

        def on_device(h=h, g=g):
            return G._gelu(h.to(DEV), g.to(DEV) if mode == 1 else None).cpu()

        runs.append((count, _gelu_units(h, g, mode, on_host), _gelu_units(h, g, mode, on_device)))
        worst_host, worst_dev = max(worst_host, runs[-1][1]), max(worst_dev, runs[-1][2])
    allowed = max(4.0, 4.0 * worst_host)
    for count, uh, ud in runs:
        print(f"[gradcam] gelu mode={mode} count={count}: host fp32 {uh:.3f} units, kernel {ud:.3f} units (allowed {allowed:.3f})")
    WORST[f"gelu.mode{mode}"] = worst_dev / allowed
    assert worst_dev <= allowed


@pytest.mark.parametrize("e", [1, 2, 16, 255, 257, 512, 8192])
@pytest.mark.parametrize("bq", [1, 2, 5])
def test_cosine_backward(e, bq):
    """Against float64 autograd of sum_r cosine_similarity(normalize(p), q_r).  The rows of p have norms 1e-6, 1, 1e4: the
    1 / |p| that the map's normalisation hides.  Bound: gamma_k (|Qa_i| + 4 |v_i| sum_j |v_j| Qa_j) / |p|,
    k = 4 block_depth(e) + 16 + bq, Qa = sum_r |q_r| / |q_r|_2."""
    rng = np.random.default_rng(70 + e + bq)
    p = rng.standard_normal((3, e))
    p = f32(p / np.linalg.norm(p, axis=1, keepdims=True) * np.array([[1e-6], [1.0], [1e4]]))
    q = rng.standard_normal((bq, e))
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * np.array([1.0, 1e-3, 50.0, 0.0, 1.0])[:bq, None]
    q = f32(q)
    pt = torch.from_numpy(p).requires_grad_(True)
    sim = F.cosine_similarity(F.normalize(pt, dim=1)[:, None, :], torch.from_numpy(q)[None, :, :], dim=2).sum()
    (ref,) = torch.autograd.grad(sim, pt)
    ref = ref.numpy()
    got = host(G._cosine_bwd(dev(p), dev(q)))
    if e == 1:
        assert np.abs(ref * np.abs(p)).max() <= 1e-12 and not got.any()          # a unit vector in one dimension cannot turn
        return
    qn = np.linalg.norm(q, axis=1, keepdims=True)
    qa = np.abs(np.divide(q, qn, out=np.zeros_like(q), where=qn > 0)).sum(0)
    pn = np.linalg.norm(p, axis=1, keepdims=True)
    v = np.abs(p / pn)
    bound = gam(4 * block_depth(e) + 16 + bq) * (qa[None, :] + 4 * v * (v @ qa)[:, None]) / pn
    for i, norm in enumerate(("1e-6", "1", "1e4")):                  # per row: the three scales are 1e10 apart
        _judge(f"cosine_bwd e={e} bq={bq} |p|={norm}", got[i], ref[i], bound[i], cap=e <= 257)
    if e > 257:
        print(f"[gradcam] e={e}: cosine_bwd bound / max |ref| {float((bound.max(1) / np.abs(ref).max(1)).max()):.2e}")


# ---- G: the assembled gradient against autograd through the model's own modules ----------------------------------------------
def _geometry(d, heads, inter, n, seed):
    """A one-layer MedSigLIP of width d on the CPU (its tower is not run: the kernels are handed tokens), perturbed weights."""
    side = int(round(n ** 0.5))
    torch.manual_seed(seed)
    m = MedSigLIP(vision_config=dict(hidden_size=d, intermediate_size=inter, num_hidden_layers=1, num_attention_heads=heads,
                                     image_size=side * 2, patch_size=2), embed_dim=64)
    m.backbone.embeddings.num_positions = n
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g))
    return m.eval()


def _autograd_side(m, x, q):
    """wbar = mean_n d sim / d x and cam = relu(x . wbar) by autograd through post_layernorm, head, projection, normalize and
    the summed cosine, in the dtype of m / x / q, on the CPU."""
    x = x.detach().clone().requires_grad_(True)
    emb = F.normalize(m.projection(m.backbone.head(m.backbone.post_layernorm(x))), dim=-1)
    sim = F.cosine_similarity(emb[:, None, :], q[None, :, :], dim=2).sum()
    (grad,) = torch.autograd.grad(sim, x)
    wbar = grad.mean(1)
    cam = torch.relu((x.detach() * wbar[:, None, :]).sum(-1))
    return wbar.double().numpy(), cam.double().numpy()


@pytest.mark.parametrize("d,heads,inter,n", [(64, 4, 64, 25), (40, 5, 24, 49), (48, 3, 80, 9), (256, 16, 128, 121)])
@pytest.mark.parametrize("bq", [1, 2])
def test_assembled_gradient_matches_autograd(d, heads, inter, n, bq, monkeypatch):
    """Pins the un-normalised scale end to end.  Tolerance max(8 E32, gamma_{d+n} max|ref|): E32 is the error of the same torch
    modules in fp32 on the CPU against their float64 run (measured on the reference side only); 8 covers two fp32 evaluations in
    different summation orders."""
    m32 = _geometry(d, heads, inter, n, 80)
    m64 = copy.deepcopy(m32).double()
    x = _tokens(2, n, d, 81)
    q = F.normalize(torch.randn((bq, 64), generator=torch.Generator().manual_seed(82)), dim=1)
    ref_w, ref_cam = _autograd_side(m64, x.double(), q.double())
    w32, cam32 = _autograd_side(m32, x, q)
    mdev = copy.deepcopy(m32).to(DEV)
    seen, orig = [], G.gradcam_finish
    monkeypatch.setattr(G, "gradcam_finish", lambda x_, heads_, ws_, size_: (seen.append(ws_), orig(x_, heads_, ws_, size_))[1])
    side = int(round(n ** 0.5))
    with torch.no_grad():
        G.gradcam_from_tokens(mdev, q.to(DEV), x.to(DEV), (side, side))
    sl = R.slot_layout(n, d, heads)
    ws = host(seen[0]).reshape(2, sl["per"])
    for name, got, ref, r32 in (("wbar", ws[:, sl["wbar"]:sl["wbar"] + d], ref_w, w32),
                                ("cam", ws[:, sl["cam"]:sl["cam"] + n], ref_cam, cam32)):
        e32 = float(np.abs(r32 - ref).max())
        tol = max(8 * e32, gam(d + n) * float(np.abs(ref).max()))
        err = float(np.abs(got - ref).max())
        print(f"[gradcam] assembled.{name} d={d} n={n} bq={bq}: kernel error / E32 {err / e32:.3f} (error {err:.3e}, E32 {e32:.3e}, "
              f"max |ref| {float(np.abs(ref).max()):.3e}, tolerance {tol:.3e})")
        WORST[f"assembled.{name}/E32"] = max(WORST.get(f"assembled.{name}/E32", 0.0), err / e32)
        assert float(np.abs(ref).max()) > 0 and err <= tol


# ---- H: bits and containment per entry point ------------------------------------------------------------------------------
def _run_chain(cs, x, w, e, H, W):
    """pool -> tokens -> finish on x [b, n, d] with a zeroed workspace -> (ybar, workspace [b, per], out)."""
    dv = cs.device()
    b = x.shape[0]
    ws = torch.zeros((b * cs.sl["per"],), dtype=torch.float32, device=DEV)
    ybar = pool(x, dv.g, dv.be, dv.U, dv.c, ws)
    after_pool = ws.clone()
    tokens(x, dv.g, dv.be, dv.U, w, e, ws)
    after_tokens = ws.clone()
    out = finish(x, cs.heads, ws, H, W)
    return ybar, [t.view(b, -1) for t in (after_pool, after_tokens, ws)], out


def test_image_bits_do_not_depend_on_the_batch():
    cs = case(25, 64, 4, 3)
    dv = cs.device()
    x5 = _tokens(5, 25, 64, 90).to(DEV)
    w5 = torch.cat([dv.w, dv.w[:2]]).contiguous()
    e5 = torch.cat([dv.e, dv.e[:2]]).contiguous()
    y5, ws5, o5 = _run_chain(cs, x5, w5, e5, 35, 33)
    y1, ws1, o1 = _run_chain(cs, x5[2:3].contiguous(), w5[2:3].contiguous(), e5[2:3].contiguous(), 35, 33)
    assert torch.equal(y5[2], y1[0]) and torch.equal(o5[2], o1[0])
    for stage, (a, c) in zip(("pool", "tokens", "finish"), zip(ws5, ws1)):
        assert torch.equal(a[2].view(torch.int32), c[0].view(torch.int32)), stage
    assert not torch.equal(ws5[2][2], ws5[2][1])


def test_tail_bits_do_not_depend_on_the_batch():
    g = torch.Generator().manual_seed(91)
    rn = lambda *s: torch.randn(s, generator=g).to(DEV)                # noqa: E731
    m, k = 37, 70
    A, bias, x, res = rn(m, k), rn(m), rn(5, k), rn(5, m)
    one = lambda t: t[2:3].contiguous()                                  # noqa: E731
    assert torch.equal(G._gemv(A, x, m, k, 5, bias=bias, res=res)[2], G._gemv(A, one(x), m, k, 1, bias=bias, res=one(res))[0])
    heads, dh = 5, 8
    d = heads * dh
    wvT, g_o = rn(d, d), rn(5, d)
    grouped = lambda t, b: G._gemv(wvT, t, heads * d, dh, b, lda=d, xs=d, mg=d, rmod=d, acol=dh, xg=dh)      # noqa: E731
    assert torch.equal(grouped(g_o, 5)[2], grouped(one(g_o), 1)[0])
    ln = SimpleNamespace(weight=rn(300), bias=rn(300), eps=1e-5)
    v, gg = rn(5, 300), rn(5, 300)
    o5, s5 = G._ln(v, ln, relu=True)
    o1, s1 = G._ln(one(v), ln, relu=True)
    assert torch.equal(o5[2], o1[0]) and torch.equal(s5[2], s1[0])
    assert torch.equal(G._ln_bwd(gg, v, s5, ln, after=o5, res=v)[2], G._ln_bwd(one(gg), one(v), s1, ln, after=o1, res=one(v))[0])
    assert torch.equal(G._gelu(v)[2], G._gelu(one(v))[0]) and torch.equal(G._gelu(v, gg)[2], G._gelu(one(v), one(gg))[0])
    q = rn(2, 300)
    assert torch.equal(G._cosine_bwd(v, q)[2], G._cosine_bwd(one(v), q)[0])


def test_nan_tokens_stay_in_their_image():
    cs = case(25, 64, 4, 3)
    dv, sl = cs.device(), cs.sl
    clean = _run_chain(cs, dv.x, dv.w, dv.e, 35, 35)
    x = dv.x.clone()
    x[1, 7, 5] = float("nan")
    dirty = _run_chain(cs, x, dv.w, dv.e, 35, 35)
    nb = -(-cs.n // 4)
    for i in (0, 2):
        assert torch.equal(dirty[0][i], clean[0][i]) and torch.equal(dirty[2][i], clean[2][i])
        for name, count in (("partials", nb * cs.d), ("wbar", cs.d), ("cam", cs.n)):
            a, c = (t[1][2][i, sl[name]:sl[name] + count] for t in (dirty, clean))
            assert torch.equal(a, c), name
    assert torch.count_nonzero(dirty[2][1]) == 0 and torch.isnan(dirty[1][2][1, sl["cam"]:sl["cam"] + cs.n]).any()
    assert torch.count_nonzero(clean[2][1]) > 0


def test_chunked_maps_are_bit_identical(monkeypatch):
    gold = dict(np.load(GOLD))
    m = R.build_model({k[2:]: v for k, v in gold.items() if k.startswith("w/")}, dtype=torch.float32).to(DEV).eval()
    imgs = torch.randn((5, 3) + R.SIZE, generator=torch.Generator().manual_seed(92)).to(DEV)
    with torch.no_grad():
        q = m(imgs[:1])
    whole = G._native_maps(m, q, imgs)
    heads = R.VISION["num_attention_heads"]
    per = G.workspace_floats(1, R.N, R.VISION["hidden_size"], heads) + R.N * R.VISION["hidden_size"]
    calls, orig = [], G.gradcam_from_tokens
    monkeypatch.setattr(G, "gradcam_from_tokens", lambda m_, q_, x_, size_: (calls.append(x_.shape[0]), orig(m_, q_, x_, size_))[1])
    monkeypatch.setattr(G, "WORKSPACE_FLOATS", 2 * per)
    parts = G._native_maps(m, q, imgs)
    assert calls == [2, 2, 1]
    assert torch.equal(whole, parts) and float(whole.max()) == 1.0
