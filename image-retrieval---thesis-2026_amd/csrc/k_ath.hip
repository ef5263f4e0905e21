// k_ath.hip -- the forward of the reference's ATHNet (ath_model.py there) in fp32 on the VALU, NCHW maps, BatchNorm folded into the
// convolutions by the caller (w' = w g / sqrt(v + eps), b' = beta - mean g / sqrt(v + eps)).  The layers are 1-16 channels wide:
// far too narrow for the MFMA path to pay, so every kernel is a thread per output pixel with all its output channels in registers
// and the (wave-uniform) weights in scalar registers.
//
//   k_ath_conv       y = [relu](b' + sum_{ci, ky, kx} w' x), 3x3, pad 1, stride 1 or 2            (a ResBlock's first conv)
//   k_ath_conv_res   y = relu((b2' + sum w2' t) + (bd' + sum wd' x))                               (its second conv + downsample)
//   k_ath_pool_sa    m = MaxPool3x3/s1/p1(r) (-inf padding); s = (mean_c m, max_c m)
//   k_ath_sa_mul     y[c] = m[c] sigmoid(sum_{j, ky, kx} w_sa s), zero padding                     (SpatialAttention, x * sa(x))
//   k_ath_avgpool    y = (sum of the 3x3 neighbourhood, zero padding) / 9                          (count_include_pad=True)
//   k_ath_heads      hash = x W_h^T + b_h, logits = x W_t^T + b_t                                  (a thread per output)
//
// Every output is a fixed-order sum over its own image's inputs (taps in (ci, ky, kx) order, the two branches of a ResBlock added
// last), so an image's bits do not depend on its batch mates, and a non-finite image reaches only its own outputs.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int ATH_THREADS = 256;

template <int CIN, int COUT, int STRIDE>
__device__ inline void conv_acc(const float *__restrict__ xb, int h, int w, int oy, int ox, const float *__restrict__ wt,
                                float (&acc)[COUT]) {
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
        const float *xc = xb + (int64_t)ci * h * w;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * STRIDE + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * STRIDE + kx - 1;
                const float v = (iy >= 0 && iy < h && ix >= 0 && ix < w) ? xc[iy * w + ix] : 0.f;
#pragma unroll
                for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wt[(co * CIN + ci) * 9 + ky * 3 + kx], v, acc[co]);
            }
        }
    }
}

// x [n, CIN, h, w] -> y [n, COUT, h / STRIDE, w / STRIDE]
template <int CIN, int COUT, int STRIDE, bool RELU>
__global__ __launch_bounds__(ATH_THREADS) void k_ath_conv(const float *__restrict__ x, int64_t n, int h, int w,
                                                          const float *__restrict__ wt, const float *__restrict__ bias,
                                                          float *__restrict__ y) {
    const int ho = h / STRIDE, wo = w / STRIDE;
    const int64_t i = (int64_t)blockIdx.x * ATH_THREADS + threadIdx.x;
    if (i >= n * ho * wo) return;
    const int64_t b = i / ((int64_t)ho * wo);
    const int p = (int)(i - b * ho * wo), oy = p / wo, ox = p - oy * wo;
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = bias[co];
    conv_acc<CIN, COUT, STRIDE>(x + b * CIN * h * w, h, w, oy, ox, wt, acc);
    float *yb = y + b * COUT * ho * wo + p;
#pragma unroll
    for (int co = 0; co < COUT; ++co) yb[(int64_t)co * ho * wo] = RELU ? relu_nan(acc[co]) : acc[co];
}

// t [n, COUT, h / 2, w / 2] (the first conv's output), x [n, CIN, h, w] (the block's input) -> y [n, COUT, h / 2, w / 2]
template <int CIN, int COUT>
__global__ __launch_bounds__(ATH_THREADS) void k_ath_conv_res(const float *__restrict__ t, const float *__restrict__ x, int64_t n,
                                                              int h, int w, const float *__restrict__ w2, const float *__restrict__ b2,
                                                              const float *__restrict__ wd, const float *__restrict__ bd,
                                                              float *__restrict__ y) {
    const int ho = h / 2, wo = w / 2;
    const int64_t i = (int64_t)blockIdx.x * ATH_THREADS + threadIdx.x;
    if (i >= n * ho * wo) return;
    const int64_t b = i / ((int64_t)ho * wo);
    const int p = (int)(i - b * ho * wo), oy = p / wo, ox = p - oy * wo;
    float a[COUT], d[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
        a[co] = b2[co];
        d[co] = bd[co];
    }
    conv_acc<COUT, COUT, 1>(t + b * COUT * ho * wo, ho, wo, oy, ox, w2, a);
    conv_acc<CIN, COUT, 2>(x + b * CIN * h * w, h, w, oy, ox, wd, d);
    float *yb = y + b * COUT * ho * wo + p;
#pragma unroll
    for (int co = 0; co < COUT; ++co) yb[(int64_t)co * ho * wo] = relu_nan(a[co] + d[co]);
}

// r [n, C, h, w] -> m [n, C, h, w] (3x3 max pool), s [n, 2, h, w] (channel mean, channel max of m)
template <int C>
__global__ __launch_bounds__(ATH_THREADS) void k_ath_pool_sa(const float *__restrict__ r, int64_t n, int h, int w,
                                                             float *__restrict__ m, float *__restrict__ s) {
    const int64_t i = (int64_t)blockIdx.x * ATH_THREADS + threadIdx.x;
    if (i >= n * h * w) return;
    const int64_t b = i / ((int64_t)h * w);
    const int p = (int)(i - b * h * w), oy = p / w, ox = p - oy * w;
    float sum = 0.f, mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float *rc = r + (b * C + c) * h * w;
        float v = -INFINITY;
#pragma unroll
        for (int ky = -1; ky <= 1; ++ky) {
            const int iy = oy + ky;
            if (iy < 0 || iy >= h) continue;
#pragma unroll
            for (int kx = -1; kx <= 1; ++kx) {
                const int ix = ox + kx;
                if (ix < 0 || ix >= w) continue;
                const float u = rc[iy * w + ix];
                v = (u > v || u != u) ? u : v;                    // NaN propagates, as max_pool2d
            }
        }
        m[(b * C + c) * h * w + p] = v;
        sum += v;
        mx = (v > mx || v != v) ? v : mx;
    }
    s[(b * 2) * h * w + p] = sum / (float)C;
    s[(b * 2 + 1) * h * w + p] = mx;
}

// y[c] = m[c] * sigmoid(conv3x3(s; w_sa[1, 2, 3, 3]))
template <int C>
__global__ __launch_bounds__(ATH_THREADS) void k_ath_sa_mul(const float *__restrict__ m, const float *__restrict__ s, int64_t n, int h,
                                                            int w, const float *__restrict__ wsa, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * ATH_THREADS + threadIdx.x;
    if (i >= n * h * w) return;
    const int64_t b = i / ((int64_t)h * w);
    const int p = (int)(i - b * h * w), oy = p / w, ox = p - oy * w;
    float acc[1] = {0.f};
    conv_acc<2, 1, 1>(s + b * 2 * h * w, h, w, oy, ox, wsa, acc);
    const float g = 1.f / (1.f + expf(-acc[0]));
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t o = (b * C + c) * h * w + p;
        y[o] = g * m[o];
    }
}

template <int C>
__global__ __launch_bounds__(ATH_THREADS) void k_ath_avgpool(const float *__restrict__ x, int64_t n, int h, int w, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * ATH_THREADS + threadIdx.x;
    if (i >= n * h * w) return;
    const int64_t b = i / ((int64_t)h * w);
    const int p = (int)(i - b * h * w), oy = p / w, ox = p - oy * w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float *xc = x + (b * C + c) * h * w;
        float v = 0.f;
#pragma unroll
        for (int ky = -1; ky <= 1; ++ky) {
#pragma unroll
            for (int kx = -1; kx <= 1; ++kx) {
                const int iy = oy + ky, ix = ox + kx;
                v += (iy >= 0 && iy < h && ix >= 0 && ix < w) ? xc[iy * w + ix] : 0.f;
            }
        }
        y[(b * C + c) * h * w + p] = v / 9.f;
    }
}

// x [n, f] -> hash [n, nh], logits [n, nc]; four partial sums over f (element e into sum e % 4), added as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(ATH_THREADS) void k_ath_heads(const float *__restrict__ x, int64_t n, int f, const float *__restrict__ wh,
                                                           const float *__restrict__ bh, int nh, const float *__restrict__ wt,
                                                           const float *__restrict__ bt, int nc, float *__restrict__ hash,
                                                           float *__restrict__ logits) {
    const int no = nh + nc;
    const int64_t i = (int64_t)blockIdx.x * ATH_THREADS + threadIdx.x;
    if (i >= n * no) return;
    const int64_t b = i / no;
    const int j = (int)(i - b * no);
    const float *wr = j < nh ? wh + (int64_t)j * f : wt + (int64_t)(j - nh) * f;
    const float *xr = x + b * f;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int e = 0;
    for (; e + 4 <= f; e += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] = fmaf(xr[e + u], wr[e + u], s[u]);
    }
    for (; e < f; ++e) s[e & 3] = fmaf(xr[e], wr[e], s[e & 3]);
    const float v = ((s[0] + s[1]) + (s[2] + s[3])) + (j < nh ? bh[j] : bt[j - nh]);
    if (j < nh) hash[b * nh + j] = v;
    else logits[b * nc + (j - nh)] = v;
}

inline dim3 grid_for(int64_t threads) { return dim3((unsigned)((threads + ATH_THREADS - 1) / ATH_THREADS)); }

}  // namespace

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

extern "C" int64_t mirx_ath_workspace_floats(int64_t n, int size) {
    if (n < 0 || size < 8 || size % 8 || size > MIRX_ATH_MAX_SIZE) return fail(MIRX_EINVAL, "ath_workspace_floats: size must be a multiple of 8 in [8, 1024], n >= 0");
    const int64_t s2 = (int64_t)(size / 2) * (size / 2);
    return n * (16 * s2 * 2 + 2 * s2);
}

extern "C" int mirx_ath_forward(const float *x, int64_t n, int size, const float *params, int hash_size, int num_classes,
                                float *workspace, int64_t workspace_floats, float *hash_out, float *logits_out, void *stream) {
    if (size < 8 || size % 8 || size > MIRX_ATH_MAX_SIZE) return fail(MIRX_EINVAL, "ath_forward: size must be a multiple of 8 in [8, 1024]");
    if (n < 0 || n > MIRX_ATH_MAX_BATCH) return fail(MIRX_EINVAL, "ath_forward: n must be in [0, 65536]");
    if (hash_size < 1 || num_classes < 1 || hash_size + num_classes > 65536)
        return fail(MIRX_EINVAL, "ath_forward: hash_size and num_classes must be >= 1 (sum <= 65536)");
    if (n == 0) return MIRX_OK;
    if (!x || !params || !workspace || !hash_out || !logits_out) return fail(MIRX_EINVAL, "ath_forward: null buffer");
    if (workspace_floats < mirx_ath_workspace_floats(n, size))
        return fail(MIRX_EINVAL, "ath_forward: workspace smaller than mirx_ath_workspace_floats()");
    if (((uintptr_t)x | (uintptr_t)params | (uintptr_t)workspace) % 16) return fail(MIRX_EINVAL, "ath_forward: buffers must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int s1 = size / 2, s2 = size / 4, s3 = size / 8;
    const int64_t a1 = (int64_t)s1 * s1;
    // params: the layout of include/mirx.h (MIRX_ATH_P_*), heads after the convolutions
    const float *p = params;
    const float *w11 = p + MIRX_ATH_P_W11, *b11 = p + MIRX_ATH_P_B11, *w12 = p + MIRX_ATH_P_W12, *b12 = p + MIRX_ATH_P_B12;
    const float *w1d = p + MIRX_ATH_P_W1D, *b1d = p + MIRX_ATH_P_B1D, *wsa = p + MIRX_ATH_P_WSA;
    const float *w21 = p + MIRX_ATH_P_W21, *b21 = p + MIRX_ATH_P_B21, *w22 = p + MIRX_ATH_P_W22, *b22 = p + MIRX_ATH_P_B22;
    const float *w2d = p + MIRX_ATH_P_W2D, *b2d = p + MIRX_ATH_P_B2D;
    const float *w31 = p + MIRX_ATH_P_W31, *b31 = p + MIRX_ATH_P_B31, *w32 = p + MIRX_ATH_P_W32, *b32 = p + MIRX_ATH_P_B32;
    const float *w3d = p + MIRX_ATH_P_W3D, *b3d = p + MIRX_ATH_P_B3D;
    const int f = s3 * s3;
    const float *wh = p + MIRX_ATH_P_HEADS, *bh = wh + (int64_t)hash_size * f;
    const float *wt = bh + hash_size, *bt = wt + (int64_t)num_classes * f;
    // workspace: A, B [n, 16, s1, s1] and S [n, 2, s1, s1]; stage 2 and 3 reuse A and B
    float *A = workspace, *B = A + n * 16 * a1, *S = B + n * 16 * a1;
    const dim3 blk(ATH_THREADS);
    // stage 1: ResBlock(3 -> 16, s2), MaxPool, spatial attention
    hipLaunchKernelGGL((k_ath_conv<3, 16, 2, true>), grid_for(n * a1), blk, 0, st, x, n, size, size, w11, b11, A);
    hipLaunchKernelGGL((k_ath_conv_res<3, 16>), grid_for(n * a1), blk, 0, st, A, x, n, size, size, w12, b12, w1d, b1d, B);
    hipLaunchKernelGGL((k_ath_pool_sa<16>), grid_for(n * a1), blk, 0, st, B, n, s1, s1, A, S);
    hipLaunchKernelGGL((k_ath_sa_mul<16>), grid_for(n * a1), blk, 0, st, A, S, n, s1, s1, wsa, B);
    // stage 2: ResBlock(16 -> 8, s2), AvgPool, ResBlock(8 -> 1, s2)
    const int64_t a2 = (int64_t)s2 * s2, a3 = (int64_t)s3 * s3;
    float *T = A, *R = A + n * 8 * a2, *P = S;
    hipLaunchKernelGGL((k_ath_conv<16, 8, 2, true>), grid_for(n * a2), blk, 0, st, B, n, s1, s1, w21, b21, T);
    hipLaunchKernelGGL((k_ath_conv_res<16, 8>), grid_for(n * a2), blk, 0, st, T, B, n, s1, s1, w22, b22, w2d, b2d, R);
    hipLaunchKernelGGL((k_ath_avgpool<8>), grid_for(n * a2), blk, 0, st, R, n, s2, s2, P);
    float *T3 = B, *R3 = B + n * a3;
    hipLaunchKernelGGL((k_ath_conv<8, 1, 2, true>), grid_for(n * a3), blk, 0, st, P, n, s2, s2, w31, b31, T3);
    hipLaunchKernelGGL((k_ath_conv_res<8, 1>), grid_for(n * a3), blk, 0, st, T3, P, n, s2, s2, w32, b32, w3d, b3d, R3);
    // heads
    hipLaunchKernelGGL(k_ath_heads, grid_for(n * (hash_size + num_classes)), blk, 0, st, R3, n, f, wh, bh, hash_size, wt, bt, num_classes,
                       hash_out, logits_out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}
