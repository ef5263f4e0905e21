// k_gradcam.hip -- Grad-CAM of a retrieved image's cosine similarity w.r.t. the last SigLIP encoder layer's tokens (the
// reference's medsiglip_saliency.py compute_gradcam_saliency / _compute_single_gradcam), in closed form.
// Everything between the last encoder layer's tokens x [n, d] and the similarity acts on one vector except post_layernorm
// (per token) and the pooling head's attention over the n tokens, so the gradient d sim / d x needs no backward pass through
// the tower.  With y = post_layernorm(x), the probe query folded into U [heads, d] and c [heads] (u_h = tau W_k,h^T q_h,
// c_h = tau q_h . b_k,h) and the backward vectors w [heads, d] (w_h = W_v,h^T g_o,h), e [heads] (e_h = g_o,h . b_v,h):
//
//   k_gc_stats      a wave per token: mean and 1 / sqrt(var + eps) of x (two passes, fixed order)
//   k_gc_scores     a wave per token: S[n, h] = y_n . v_h + s_h for (v, s) = (U, c) (the scores) or (w, e) (dP)
//   k_gc_softmax    a workgroup per (image, head): P = softmax_n(S) in place (NaN kept), or sum_n P dP (mode 1)
//   k_gc_pool       64 columns x 4 token quarters per workgroup: Ybar[h, :] = sum_n P[n, h] y_n, quarters added in order
//   k_gc_tokens     a wave per TB tokens: dS = P (dP - sum_n P dP), g_y = sum_h dS u_h + P w_h, the LayerNorm backward
//                   g_x = r (gamma g_y - mean(gamma g_y) - xhat mean(gamma g_y xhat)), the TB tokens' column sum of g_x
//   k_gc_wbar       wbar = (sum of the column partials in block order) / n
//   k_gc_cam        a wave per token: relu(x_n . wbar) (NaN kept)
//   k_gc_upsample   bilinear (align_corners=False) into out [b, H, W] and per-workgroup min / max (NaN kept)
//   k_gc_normalize  min / max over the workgroups in order; (v - min) / (max - min) when max - min > 1e-8, else 0
// The vector tail (pooling-head out_proj, MLP, projection, cosine) runs on k_gc_gemv and the small elementwise kernels below.
//
// Every output for image b is a fixed-order function of image b's inputs alone (no atomics, the reduction orders depend on
// n, d and heads only): bit-identical whatever b is and however the images are chunked.
#include <cmath>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_MAXH = MIRX_GRADCAM_MAX_HEADS;     // 16: one accumulator per head per lane
constexpr int GC_TB = MIRX_GRADCAM_TOKENS_PER_BLOCK;
constexpr int GC_MAP_ROWS = 16;                    // output rows per upsample workgroup
constexpr int GC_MM = 2 * ((MIRX_GRADCAM_MAX_SIZE + GC_MAP_ROWS - 1) / GC_MAP_ROWS);

// fixed-shape tree over the GC_THREADS values of a workgroup (LDS scratch of GC_THREADS floats); every thread gets the result
__device__ inline float block_sum(float v, float *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = GC_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}
__device__ inline float block_max(float v, float *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = GC_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) sh[tid] = nanmax(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// workspace of one image (floats): stats [2n] | P [n * heads] | dP [n * heads] | dsum [16] | partials [ceil(n / TB) * d] |
// wbar [d] | cam [n] | min / max [GC_MM]
struct Slot {
    int64_t stats, p, dp, dsum, part, wbar, cam, mm, per;
};
__host__ __device__ inline Slot slot_of(int n, int d, int heads) {
    Slot s;
    s.stats = 0;
    s.p = s.stats + 2 * (int64_t)n;
    s.dp = s.p + (int64_t)n * heads;
    s.dsum = s.dp + (int64_t)n * heads;
    s.part = s.dsum + GC_MAXH;
    s.wbar = s.part + (int64_t)((n + GC_TB - 1) / GC_TB) * d;
    s.cam = s.wbar + d;
    s.mm = s.cam + n;
    s.per = (s.mm + GC_MM + 3) / 4 * 4;
    return s;
}

__device__ inline float yval(float x, float mu, float r, float g, float be) { return g * ((x - mu) * r) + be; }

__global__ __launch_bounds__(GC_THREADS) void k_gc_stats(const float *x, int n, int d, float eps, float *ws, Slot sl) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t bi = blockIdx.y;
    if (t >= n) return;
    const float *xr = x + (bi * n + t) * (int64_t)d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) s += xr[j];
    const float mu = wave_sum(s) / (float)d;
    float v = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float c = xr[j] - mu;
        v += c * c;
    }
    const float var = wave_sum(v) / (float)d;
    if (lane == 0) {
        float *st = ws + bi * sl.per + sl.stats + 2 * t;
        st[0] = mu;
        st[1] = 1.f / sqrtf(var + eps);
    }
}

// S[b, t, h] = y_t . v[b, h, :] + s[b, h] (h < heads); vstride / sstride = 0 shares one (v, s) across the images
__global__ __launch_bounds__(GC_THREADS) void k_gc_scores(const float *x, int n, int d, int heads, const float *gamma, const float *beta,
                                                          const float *v, int64_t vstride, const float *s, int64_t sstride, float *ws,
                                                          Slot sl, int64_t out_off) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t bi = blockIdx.y;
    if (t >= n) return;
    const float *xr = x + (bi * n + t) * (int64_t)d;
    const float *wsb = ws + bi * sl.per;
    const float mu = wsb[sl.stats + 2 * t], r = wsb[sl.stats + 2 * t + 1];
    const float *vb = v + bi * vstride;
    float acc[GC_MAXH];
#pragma unroll
    for (int h = 0; h < GC_MAXH; ++h) acc[h] = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float y = yval(xr[j], mu, r, gamma[j], beta[j]);
#pragma unroll
        for (int h = 0; h < GC_MAXH; ++h)
            if (h < heads) acc[h] += y * vb[(int64_t)h * d + j];
    }
    float *o = ws + bi * sl.per + out_off + (int64_t)t * heads;
    const float *sb = s + bi * sstride;
#pragma unroll
    for (int h = 0; h < GC_MAXH; ++h) {
        if (h < heads) {
            const float a = wave_sum(acc[h]);
            if (lane == 0) o[h] = a + sb[h];
        }
    }
}

// mode 0: P[:, h] = softmax over the n tokens of S[:, h] (in place in the P area); mode 1: dsum[h] = sum_t P[t, h] dP[t, h]
__global__ __launch_bounds__(GC_THREADS) void k_gc_softmax(int n, int heads, float *ws, Slot sl, int mode) {
    __shared__ float sh[GC_THREADS];
    const int tid = threadIdx.x, h = blockIdx.x;
    const int64_t bi = blockIdx.y;
    float *p = ws + bi * sl.per + sl.p;
    if (mode == 1) {
        const float *dp = ws + bi * sl.per + sl.dp;
        float a = 0.f;
        for (int t = tid; t < n; t += GC_THREADS) a += p[(int64_t)t * heads + h] * dp[(int64_t)t * heads + h];
        const float s = block_sum(a, sh);
        if (tid == 0) ws[bi * sl.per + sl.dsum + h] = s;
        return;
    }
    float m = -INFINITY;
    for (int t = tid; t < n; t += GC_THREADS) m = nanmax(m, p[(int64_t)t * heads + h]);
    m = block_max(m, sh);
    float a = 0.f;
    for (int t = tid; t < n; t += GC_THREADS) a += expf(p[(int64_t)t * heads + h] - m);
    const float z = block_sum(a, sh);
    for (int t = tid; t < n; t += GC_THREADS) p[(int64_t)t * heads + h] = expf(p[(int64_t)t * heads + h] - m) / z;
}

// ybar[b, h, j] = sum_t P[t, h] y_t[j]: lane = column, wave = quarter of the tokens (ascending), quarters added in order
__global__ __launch_bounds__(GC_THREADS) void k_gc_pool(const float *x, int n, int d, int heads, const float *gamma, const float *beta,
                                                        const float *ws, Slot sl, float *ybar) {
    __shared__ float sh[4][GC_MAXH][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int64_t bi = blockIdx.y;
    const float *wsb = ws + bi * sl.per;
    const int nq = (n + 3) / 4, t0 = q * nq, t1 = min(n, t0 + nq);
    float acc[GC_MAXH];
#pragma unroll
    for (int h = 0; h < GC_MAXH; ++h) acc[h] = 0.f;
    if (j < d) {
        const float g = gamma[j], be = beta[j];
        for (int t = t0; t < t1; ++t) {
            const float y = yval(x[(bi * n + t) * (int64_t)d + j], wsb[sl.stats + 2 * t], wsb[sl.stats + 2 * t + 1], g, be);
            const float *pt = wsb + sl.p + (int64_t)t * heads;
#pragma unroll
            for (int h = 0; h < GC_MAXH; ++h)
                if (h < heads) acc[h] += pt[h] * y;
        }
    }
#pragma unroll
    for (int h = 0; h < GC_MAXH; ++h) sh[q][h][lane] = acc[h];
    __syncthreads();
    if (q == 0 && j < d) {
        for (int h = 0; h < heads; ++h)
            ybar[(bi * heads + h) * (int64_t)d + j] = ((sh[0][h][lane] + sh[1][h][lane]) + sh[2][h][lane]) + sh[3][h][lane];
    }
}

// per TB tokens of image b: g_x of each token, summed over the tokens in order into the block's column partials
__global__ __launch_bounds__(64) void k_gc_tokens(const float *x, int n, int d, int heads, const float *gamma, const float *u,
                                                  const float *w, float *ws, Slot sl) {
    const int lane = threadIdx.x;
    const int blk = blockIdx.x;
    const int64_t bi = blockIdx.y;
    float *wsb = ws + bi * sl.per;
    const float *wb = w + bi * (int64_t)heads * d;
    float a[GC_TB][GC_MAXH], p[GC_TB][GC_MAXH], mu[GC_TB], r[GC_TB];
#pragma unroll
    for (int k = 0; k < GC_TB; ++k) {
        const int t = min(blk * GC_TB + k, n - 1);
        mu[k] = wsb[sl.stats + 2 * t];
        r[k] = wsb[sl.stats + 2 * t + 1];
#pragma unroll
        for (int h = 0; h < GC_MAXH; ++h) {
            const float ph = h < heads ? wsb[sl.p + (int64_t)t * heads + h] : 0.f;
            const float dph = h < heads ? wsb[sl.dp + (int64_t)t * heads + h] : 0.f;
            const float sh = h < heads ? wsb[sl.dsum + h] : 0.f;
            p[k][h] = ph;
            a[k][h] = ph * (dph - sh);
        }
    }
    // pass 1: sum(gamma g_y) and sum(gamma g_y xhat) per token
    float sg[GC_TB], sgx[GC_TB];
#pragma unroll
    for (int k = 0; k < GC_TB; ++k) sg[k] = sgx[k] = 0.f;
    for (int j = lane; j < d; j += 64) {
        float uj[GC_MAXH], wj[GC_MAXH];
#pragma unroll
        for (int h = 0; h < GC_MAXH; ++h) {
            uj[h] = h < heads ? u[(int64_t)h * d + j] : 0.f;
            wj[h] = h < heads ? wb[(int64_t)h * d + j] : 0.f;
        }
        const float gj = gamma[j];
#pragma unroll
        for (int k = 0; k < GC_TB; ++k) {
            const int t = min(blk * GC_TB + k, n - 1);
            float gy = 0.f;
#pragma unroll
            for (int h = 0; h < GC_MAXH; ++h) gy = (gy + a[k][h] * uj[h]) + p[k][h] * wj[h];
            const float gh = gj * gy;
            const float xh = (x[(bi * n + t) * (int64_t)d + j] - mu[k]) * r[k];
            sg[k] += gh;
            sgx[k] += gh * xh;
        }
    }
    float mg[GC_TB], mgx[GC_TB];
#pragma unroll
    for (int k = 0; k < GC_TB; ++k) {
        mg[k] = wave_sum(sg[k]) / (float)d;
        mgx[k] = wave_sum(sgx[k]) / (float)d;
    }
    // pass 2: g_x per token (recomputed), the block's tokens summed in order
    float *part = wsb + sl.part + (int64_t)blk * d;
    for (int j = lane; j < d; j += 64) {
        float uj[GC_MAXH], wj[GC_MAXH];
#pragma unroll
        for (int h = 0; h < GC_MAXH; ++h) {
            uj[h] = h < heads ? u[(int64_t)h * d + j] : 0.f;
            wj[h] = h < heads ? wb[(int64_t)h * d + j] : 0.f;
        }
        const float gj = gamma[j];
        float col = 0.f;
#pragma unroll
        for (int k = 0; k < GC_TB; ++k) {
            const int t = blk * GC_TB + k;
            if (t < n) {
                float gy = 0.f;
#pragma unroll
                for (int h = 0; h < GC_MAXH; ++h) gy = (gy + a[k][h] * uj[h]) + p[k][h] * wj[h];
                const float gh = gj * gy;
                const float xh = (x[(bi * n + t) * (int64_t)d + j] - mu[k]) * r[k];
                col += r[k] * ((gh - mg[k]) - xh * mgx[k]);
            }
        }
        part[j] = col;
    }
}

__global__ __launch_bounds__(GC_THREADS) void k_gc_wbar(int n, int d, float *ws, Slot sl) {
    const int j = blockIdx.x * GC_THREADS + threadIdx.x;
    const int64_t bi = blockIdx.y;
    if (j >= d) return;
    float *wsb = ws + bi * sl.per;
    const int nb = (n + GC_TB - 1) / GC_TB;
    float s = 0.f;
    for (int k = 0; k < nb; ++k) s += wsb[sl.part + (int64_t)k * d + j];
    wsb[sl.wbar + j] = s / (float)n;
}

__global__ __launch_bounds__(GC_THREADS) void k_gc_cam(const float *x, int n, int d, float *ws, Slot sl) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t bi = blockIdx.y;
    if (t >= n) return;
    float *wsb = ws + bi * sl.per;
    const float *xr = x + (bi * n + t) * (int64_t)d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) s += xr[j] * wsb[sl.wbar + j];
    s = wave_sum(s);
    if (lane == 0) wsb[sl.cam + t] = relu_nan(s);
}

// bilinear, align_corners=False (ATen's upsample_bilinear2d source index: max(scale * (dst + 0.5) - 0.5, 0)), and the
// workgroup's min / max (NaN kept)
__global__ __launch_bounds__(GC_THREADS) void k_gc_upsample(int g, int H, int W, float *ws, Slot sl, float *out) {
    __shared__ float smap[MIRX_GRADCAM_MAX_N];
    __shared__ float sh[GC_THREADS];
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.y;
    float *wsb = ws + bi * sl.per;
    for (int i = tid; i < g * g; i += GC_THREADS) smap[i] = wsb[sl.cam + i];
    __syncthreads();
    const float sc = (float)g / (float)H, sw = (float)g / (float)W;
    const int y_lo = blockIdx.x * GC_MAP_ROWS, y_hi = min(H, y_lo + GC_MAP_ROWS);
    float *ob = out + bi * (int64_t)H * W;
    const int64_t cnt = (int64_t)(y_hi - y_lo) * W;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t e = tid; e < cnt; e += GC_THREADS) {
        const int y = y_lo + (int)(e / W), xx = (int)(e % W);
        const float fy = fmaxf(sc * ((float)y + 0.5f) - 0.5f, 0.f);
        const float fx = fmaxf(sw * ((float)xx + 0.5f) - 0.5f, 0.f);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < g - 1 ? 1 : 0), x1 = x0 + (x0 < g - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        const float v = hy * (hx * smap[y0 * g + x0] + lx * smap[y0 * g + x1]) + ly * (hx * smap[y1 * g + x0] + lx * smap[y1 * g + x1]);
        ob[(int64_t)y * W + xx] = v;
        mn = nanmin(mn, v);
        mx = nanmax(mx, v);
    }
    mx = block_max(mx, sh);
    mn = -block_max(-mn, sh);
    if (tid == 0) {
        wsb[sl.mm + 2 * blockIdx.x] = mn;
        wsb[sl.mm + 2 * blockIdx.x + 1] = mx;
    }
}

// numpy float32: cam_max - cam_min > 1e-8 -> (cam - cam_min) / (cam_max - cam_min), else 0 (a NaN anywhere -> 0)
__global__ __launch_bounds__(GC_THREADS) void k_gc_normalize(int H, int W, const float *ws, Slot sl, float *out) {
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.y;
    const float *wsb = ws + bi * sl.per;
    const int nblk = (H + GC_MAP_ROWS - 1) / GC_MAP_ROWS;
    float mn = wsb[sl.mm], mx = wsb[sl.mm + 1];
    for (int k = 1; k < nblk; ++k) {
        mn = nanmin(mn, wsb[sl.mm + 2 * k]);
        mx = nanmax(mx, wsb[sl.mm + 2 * k + 1]);
    }
    const float diff = mx - mn;
    const bool ok = diff > 1e-8f;
    const int y_lo = blockIdx.x * GC_MAP_ROWS, y_hi = min(H, y_lo + GC_MAP_ROWS);
    float *ob = out + bi * (int64_t)H * W + (int64_t)y_lo * W;
    const int64_t cnt = (int64_t)(y_hi - y_lo) * W;
    for (int64_t e = tid; e < cnt; e += GC_THREADS) ob[e] = ok ? (ob[e] - mn) / diff : 0.f;
}

// ---- the vector tail ----
// out[b, j] = dot + bias[j] + res[b, j], dot = sum_t A[(j % rmod) * lda + (j / mg) * acol + t] * x[b * xs + (j / mg) * xg + t]
// (a wave per output: lane-strided ascending, then the butterfly)
__global__ __launch_bounds__(GC_THREADS) void k_gc_gemv(const float *A, int64_t lda, const float *x, int64_t xs, const float *bias,
                                                        const float *res, int64_t rs, float *out, int64_t os, int m, int k, int mg,
                                                        int rmod, int64_t acol, int64_t xg) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t bi = blockIdx.y;
    if (j >= m) return;
    const int grp = j / mg;
    const float *ar = A + (int64_t)(j % rmod) * lda + grp * acol;
    const float *xr = x + bi * xs + grp * xg;
    float s = 0.f;
    for (int t = lane; t < k; t += 64) s += ar[t] * xr[t];
    s = wave_sum(s);
    if (lane == 0) {
        if (bias) s = s + bias[j];
        if (res) s = s + res[bi * rs + j];
        out[bi * os + j] = s;
    }
}

// vector LayerNorm over rows of len: out = gamma * (v - mu) r + beta (relu: then max(., 0), NaN kept), stats [b, 2] = (mu, r)
__global__ __launch_bounds__(GC_THREADS) void k_gc_layernorm(const float *v, int len, const float *gamma, const float *beta, float eps,
                                                             int relu, float *out, float *stats) {
    __shared__ float sh[GC_THREADS];
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.x;
    const float *vr = v + bi * len;
    float s = 0.f;
    for (int i = tid; i < len; i += GC_THREADS) s += vr[i];
    const float mu = block_sum(s, sh) / (float)len;
    float q = 0.f;
    for (int i = tid; i < len; i += GC_THREADS) {
        const float c = vr[i] - mu;
        q += c * c;
    }
    const float r = 1.f / sqrtf(block_sum(q, sh) / (float)len + eps);
    for (int i = tid; i < len; i += GC_THREADS) {
        const float y = gamma[i] * ((vr[i] - mu) * r) + beta[i];
        out[bi * len + i] = relu ? relu_nan(y) : y;
    }
    if (tid == 0) {
        stats[2 * bi] = mu;
        stats[2 * bi + 1] = r;
    }
}

// LayerNorm backward: gh = gamma * g (times (after > 0) when `after` is given: the ReLU behind it), out = r (gh - mean(gh)
// - xhat mean(gh xhat)) (+ res)
__global__ __launch_bounds__(GC_THREADS) void k_gc_layernorm_bwd(const float *g, const float *after, const float *v, const float *stats,
                                                                 const float *gamma, int len, const float *res, float *out) {
    __shared__ float sh[GC_THREADS];
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.x;
    const float mu = stats[2 * bi], r = stats[2 * bi + 1];
    float s = 0.f, sx = 0.f;
    for (int i = tid; i < len; i += GC_THREADS) {
        float gi = g[bi * len + i];
        if (after) gi = after[bi * len + i] > 0.f ? gi : 0.f;
        const float gh = gamma[i] * gi;
        s += gh;
        sx += gh * ((v[bi * len + i] - mu) * r);
    }
    const float mg = block_sum(s, sh) / (float)len;
    const float mgx = block_sum(sx, sh) / (float)len;
    for (int i = tid; i < len; i += GC_THREADS) {
        float gi = g[bi * len + i];
        if (after) gi = after[bi * len + i] > 0.f ? gi : 0.f;
        const float gh = gamma[i] * gi;
        const float xh = (v[bi * len + i] - mu) * r;
        float o = r * ((gh - mg) - xh * mgx);
        if (res) o = res[bi * len + i] + o;
        out[bi * len + i] = o;
    }
}

// tanh-GELU (mode 0: out = gelu(h)) and its derivative (mode 1: out = g * gelu'(h)), as ATen writes them
__global__ __launch_bounds__(GC_THREADS) void k_gc_gelu(const float *h, const float *g, int64_t count, int mode, float *out) {
    const int64_t i = (int64_t)blockIdx.x * GC_THREADS + threadIdx.x;
    if (i >= count) return;
    const float kBeta = 0.7978845608028654f, kKappa = 0.044715f;
    const float x = h[i];
    const float x2 = x * x;
    const float inner = kBeta * (x + kKappa * (x2 * x));
    const float th = tanhf(inner);
    if (mode == 0) {
        out[i] = 0.5f * x * (1.f + th);
    } else {
        const float left = 0.5f * x, right = 1.f + th;
        const float dl = 0.5f * right;
        const float dr = left * (1.f - th * th) * kBeta * (1.f + 3.f * kKappa * x2);
        out[i] = g[i] * (dl + dr);
    }
}

// d/dp sum_r cos(normalize(p), q_r) for p [b, e], q [bq, e] (normalize: p / max(|p|, 1e-12); cos: unit vectors, eps 1e-8)
__global__ __launch_bounds__(GC_THREADS) void k_gc_cosine_bwd(const float *p, int e, const float *q, int64_t bq, float *out) {
    __shared__ float sh[GC_THREADS];
    __shared__ float qs[MIRX_GRADCAM_MAX_EMBED];
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.x;
    for (int i = tid; i < e; i += GC_THREADS) qs[i] = 0.f;
    for (int64_t rr = 0; rr < bq; ++rr) {
        float s = 0.f;
        for (int i = tid; i < e; i += GC_THREADS) s += q[rr * e + i] * q[rr * e + i];
        const float qn = fmaxf(sqrtf(block_sum(s, sh)), 1e-8f);
        for (int i = tid; i < e; i += GC_THREADS) qs[i] += q[rr * e + i] / qn;
    }
    const float *pr = p + bi * e;
    float s = 0.f;
    for (int i = tid; i < e; i += GC_THREADS) s += pr[i] * pr[i];
    const float pn = fmaxf(sqrtf(block_sum(s, sh)), 1e-12f);
    // v = p / pn; g_v = Q / |v| - (v . Q) v / |v|^3
    float vv = 0.f, vq = 0.f;
    for (int i = tid; i < e; i += GC_THREADS) {
        const float v = pr[i] / pn;
        vv += v * v;
        vq += v * qs[i];
    }
    const float vn = fmaxf(sqrtf(block_sum(vv, sh)), 1e-8f);
    vq = block_sum(vq, sh);
    const float c1 = 1.f / vn, c2 = vq / (vn * vn * vn);
    // g_p = (g_v - v (v . g_v)) / pn  for |p| > 1e-12
    float vg = 0.f;
    for (int i = tid; i < e; i += GC_THREADS) {
        const float v = pr[i] / pn;
        vg += v * (qs[i] * c1 - v * c2);
    }
    vg = block_sum(vg, sh);
    for (int i = tid; i < e; i += GC_THREADS) {
        const float v = pr[i] / pn;
        out[bi * e + i] = ((qs[i] * c1 - v * c2) - v * vg) / pn;
    }
}

}  // namespace

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

static bool gc_dims_ok(int64_t b, int n, int d, int heads) {
    return b >= 0 && b <= MIRX_GRADCAM_MAX_IMAGES && n >= 1 && n <= MIRX_GRADCAM_MAX_N && heads >= 1 && heads <= MIRX_GRADCAM_MAX_HEADS &&
           d >= 1 && d <= MIRX_GRADCAM_MAX_WIDTH && d % heads == 0;
}
static bool aligned4(const void *p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }
#define GC_DIMS_MSG "b in [0, 65535], n in [1, 1024], heads in [1, 16], d in [1, 8192] and a multiple of heads"

extern "C" int64_t mirx_gradcam_workspace_floats(int64_t b, int n, int d, int heads) {
    if (!gc_dims_ok(b, n, d, heads)) return fail(MIRX_EINVAL, "gradcam_workspace_floats: " GC_DIMS_MSG);
    return b * slot_of(n, d, heads).per;
}

extern "C" int mirx_gradcam_pool(const float *x, int64_t b, int n, int d, int heads, const float *gamma, const float *beta, float eps,
                                 const float *u, const float *c, float *workspace, int64_t workspace_floats, float *ybar, void *stream) {
    if (!gc_dims_ok(b, n, d, heads)) return fail(MIRX_EINVAL, "gradcam_pool: " GC_DIMS_MSG);
    if (!(eps >= 0.f) || std::isinf(eps)) return fail(MIRX_EINVAL, "gradcam_pool: eps must be finite and >= 0");
    if (!x || !gamma || !beta || !u || !c || !workspace || !ybar) return fail(MIRX_EINVAL, "gradcam_pool: null buffer");
    if (!aligned4(x) || !aligned4(gamma) || !aligned4(beta) || !aligned4(u) || !aligned4(c) || !aligned4(workspace) || !aligned4(ybar))
        return fail(MIRX_EINVAL, "gradcam_pool: buffers must be 4-byte aligned");
    const Slot sl = slot_of(n, d, heads);
    if (workspace_floats < b * sl.per) return fail(MIRX_EINVAL, "gradcam_pool: workspace smaller than mirx_gradcam_workspace_floats()");
    if (b == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 tok((unsigned)((n + 3) / 4), (unsigned)b);
    hipLaunchKernelGGL(k_gc_stats, tok, dim3(GC_THREADS), 0, st, x, n, d, eps, workspace, sl);
    hipLaunchKernelGGL(k_gc_scores, tok, dim3(GC_THREADS), 0, st, x, n, d, heads, gamma, beta, u, (int64_t)0, c, (int64_t)0, workspace, sl,
                       sl.p);
    hipLaunchKernelGGL(k_gc_softmax, dim3((unsigned)heads, (unsigned)b), dim3(GC_THREADS), 0, st, n, heads, workspace, sl, 0);
    hipLaunchKernelGGL(k_gc_pool, dim3((unsigned)((d + 63) / 64), (unsigned)b), dim3(GC_THREADS), 0, st, x, n, d, heads, gamma, beta,
                       workspace, sl, ybar);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_tokens(const float *x, int64_t b, int n, int d, int heads, const float *gamma, const float *beta, const float *u,
                                   const float *w, const float *e, float *workspace, int64_t workspace_floats, void *stream) {
    if (!gc_dims_ok(b, n, d, heads)) return fail(MIRX_EINVAL, "gradcam_tokens: " GC_DIMS_MSG);
    if (!x || !gamma || !beta || !u || !w || !e || !workspace) return fail(MIRX_EINVAL, "gradcam_tokens: null buffer");
    if (!aligned4(x) || !aligned4(gamma) || !aligned4(beta) || !aligned4(u) || !aligned4(w) || !aligned4(e) || !aligned4(workspace))
        return fail(MIRX_EINVAL, "gradcam_tokens: buffers must be 4-byte aligned");
    const Slot sl = slot_of(n, d, heads);
    if (workspace_floats < b * sl.per) return fail(MIRX_EINVAL, "gradcam_tokens: workspace smaller than mirx_gradcam_workspace_floats()");
    if (b == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_gc_scores, dim3((unsigned)((n + 3) / 4), (unsigned)b), dim3(GC_THREADS), 0, st, x, n, d, heads, gamma, beta, w,
                       (int64_t)heads * d, e, (int64_t)heads, workspace, sl, sl.dp);
    hipLaunchKernelGGL(k_gc_softmax, dim3((unsigned)heads, (unsigned)b), dim3(GC_THREADS), 0, st, n, heads, workspace, sl, 1);
    hipLaunchKernelGGL(k_gc_tokens, dim3((unsigned)((n + GC_TB - 1) / GC_TB), (unsigned)b), dim3(64), 0, st, x, n, d, heads, gamma, u, w,
                       workspace, sl);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_finish(const float *x, int64_t b, int n, int d, int heads, float *workspace, int64_t workspace_floats, int H,
                                   int W, float *out, void *stream) {
    if (!gc_dims_ok(b, n, d, heads)) return fail(MIRX_EINVAL, "gradcam_finish: " GC_DIMS_MSG);
    int g = 0;
    while ((g + 1) * (g + 1) <= n) ++g;
    if (g * g != n) return fail(MIRX_EINVAL, "gradcam_finish: n must be a square (the tokens form a square grid)");
    if (H < 1 || H > MIRX_GRADCAM_MAX_SIZE || W < 1 || W > MIRX_GRADCAM_MAX_SIZE)
        return fail(MIRX_EINVAL, "gradcam_finish: H, W must be in [1, 8192]");
    if (!x || !workspace || !out) return fail(MIRX_EINVAL, "gradcam_finish: null buffer");
    if (!aligned4(x) || !aligned4(workspace) || !aligned4(out)) return fail(MIRX_EINVAL, "gradcam_finish: buffers must be 4-byte aligned");
    const Slot sl = slot_of(n, d, heads);
    if (workspace_floats < b * sl.per) return fail(MIRX_EINVAL, "gradcam_finish: workspace smaller than mirx_gradcam_workspace_floats()");
    if (b == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_gc_wbar, dim3((unsigned)((d + GC_THREADS - 1) / GC_THREADS), (unsigned)b), dim3(GC_THREADS), 0, st, n, d,
                       workspace, sl);
    hipLaunchKernelGGL(k_gc_cam, dim3((unsigned)((n + 3) / 4), (unsigned)b), dim3(GC_THREADS), 0, st, x, n, d, workspace, sl);
    const dim3 rows((unsigned)((H + GC_MAP_ROWS - 1) / GC_MAP_ROWS), (unsigned)b);
    hipLaunchKernelGGL(k_gc_upsample, rows, dim3(GC_THREADS), 0, st, g, H, W, workspace, sl, out);
    hipLaunchKernelGGL(k_gc_normalize, rows, dim3(GC_THREADS), 0, st, H, W, workspace, sl, out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_gemv(const float *A, int64_t lda, const float *x, int64_t xs, const float *bias, const float *res, int64_t rs,
                                 float *out, int64_t os, int64_t b, int m, int k, int mg, int rmod, int64_t acol, int64_t xg, void *stream) {
    if (b < 0 || b > MIRX_GRADCAM_MAX_IMAGES || m < 1 || k < 1 || mg < 1 || rmod < 1 || lda < 0 || xs < 0 || rs < 0 || os < 0 || acol < 0 ||
        xg < 0)
        return fail(MIRX_EINVAL, "gradcam_gemv: b in [0, 65535], m, k, mg, rmod >= 1, strides >= 0");
    if (!A || !x || !out) return fail(MIRX_EINVAL, "gradcam_gemv: null buffer");
    if (!aligned4(A) || !aligned4(x) || !aligned4(out) || !aligned4(bias) || !aligned4(res))
        return fail(MIRX_EINVAL, "gradcam_gemv: buffers must be 4-byte aligned");
    if (b == 0) return MIRX_OK;
    hipLaunchKernelGGL(k_gc_gemv, dim3((unsigned)((m + 3) / 4), (unsigned)b), dim3(GC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), A,
                       lda, x, xs, bias, res, rs, out, os, m, k, mg, rmod, acol, xg);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_layernorm(const float *v, int64_t b, int len, const float *gamma, const float *beta, float eps, int relu,
                                      float *out, float *stats, void *stream) {
    if (b < 0 || b > MIRX_GRADCAM_MAX_IMAGES || len < 1 || len > MIRX_GRADCAM_MAX_EMBED)
        return fail(MIRX_EINVAL, "gradcam_layernorm: b in [0, 65535], len in [1, 8192]");
    if (!(eps >= 0.f) || std::isinf(eps)) return fail(MIRX_EINVAL, "gradcam_layernorm: eps must be finite and >= 0");
    if (!v || !gamma || !beta || !out || !stats) return fail(MIRX_EINVAL, "gradcam_layernorm: null buffer");
    if (b == 0) return MIRX_OK;
    hipLaunchKernelGGL(k_gc_layernorm, dim3((unsigned)b), dim3(GC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), v, len, gamma, beta,
                       eps, relu, out, stats);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_layernorm_bwd(const float *g, const float *after, const float *v, const float *stats, const float *gamma,
                                          int64_t b, int len, const float *res, float *out, void *stream) {
    if (b < 0 || b > MIRX_GRADCAM_MAX_IMAGES || len < 1 || len > MIRX_GRADCAM_MAX_EMBED)
        return fail(MIRX_EINVAL, "gradcam_layernorm_bwd: b in [0, 65535], len in [1, 8192]");
    if (!g || !v || !stats || !gamma || !out) return fail(MIRX_EINVAL, "gradcam_layernorm_bwd: null buffer");
    if (b == 0) return MIRX_OK;
    hipLaunchKernelGGL(k_gc_layernorm_bwd, dim3((unsigned)b), dim3(GC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g, after, v, stats,
                       gamma, len, res, out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_gelu(const float *h, const float *g, int64_t count, int mode, float *out, void *stream) {
    if (count < 0 || count > (1LL << 31)) return fail(MIRX_EINVAL, "gradcam_gelu: count must be in [0, 2^31]");
    if (mode != 0 && mode != 1) return fail(MIRX_EINVAL, "gradcam_gelu: mode must be 0 (gelu) or 1 (g * gelu')");
    if (!h || !out || (mode == 1 && !g)) return fail(MIRX_EINVAL, "gradcam_gelu: null buffer");
    if (count == 0) return MIRX_OK;
    hipLaunchKernelGGL(k_gc_gelu, dim3((unsigned)((count + GC_THREADS - 1) / GC_THREADS)), dim3(GC_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), h, g, count, mode, out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_gradcam_cosine_bwd(const float *p, int64_t b, int e, const float *q, int64_t bq, float *out, void *stream) {
    if (b < 0 || b > MIRX_GRADCAM_MAX_IMAGES || e < 1 || e > MIRX_GRADCAM_MAX_EMBED || bq < 1 || bq > MIRX_GRADCAM_MAX_IMAGES)
        return fail(MIRX_EINVAL, "gradcam_cosine_bwd: b in [0, 65535], e in [1, 8192], bq in [1, 65535]");
    if (!p || !q || !out) return fail(MIRX_EINVAL, "gradcam_cosine_bwd: null buffer");
    if (b == 0) return MIRX_OK;
    hipLaunchKernelGGL(k_gc_cosine_bwd, dim3((unsigned)b), dim3(GC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), p, e, q, bq, out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}
