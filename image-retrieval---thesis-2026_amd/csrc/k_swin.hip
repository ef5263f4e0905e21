// k_swin.hip -- the memory-bound glue of SwinV2's res-post-norm blocks (timm 0.9.7 SwinTransformerV2Block / PatchMerging, the
// backbone of the reference's SwinV2, model.py:418-446 there), so that no library op is left between its Linears:
//
//   k_postnorm_rows    out = x + LayerNorm(y) over the channel rows (x may be absent: out = LayerNorm(y), the LayerNorm that
//                      starts a stage; out may be x itself), one wavefront per row with the row of y kept in registers (the
//                      k_layernorm_rows recipe: two-pass mean / variance in fp32); optionally out is also written as terms rows
//                      of scale * out (k_linear_t2.hip layout) for the Linear that reads the residual stream next (qkv, fc1).
//   k_patch_merge      the 2 x 2 quads of [n, h, w, c] fp32 rows gathered into terms rows [n, h / 2, w / 2, 4 c] of scale * x in
//                      timm's order -- quad (0, 0), (1, 0), (0, 1), (1, 1) as (row, column) offsets -- for the reduction Linear.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

// store_terms4's layout addressed inside one terms row by quad: 4 values at feature 4 i (line i >> 3: 64 bytes of high terms, then
// 64 of low terms).  Kept beside store_terms4: the quad-index form compiles to a different instruction order.
__device__ inline void put_terms4(char *trow, int i, const f32x4 &o, float scale) {
    unsigned h0, l0, h1, l1;
    split2h_pair(o[0] * scale, o[1] * scale, h0, l0);
    split2h_pair(o[2] * scale, o[3] * scale, h1, l1);
    const u32x2 hi = {h0, h1}, lo = {l0, l1};
    char *dst = trow + (i >> 3) * 128 + (i & 7) * 8;
    *reinterpret_cast<u32x2 *>(dst) = hi;
    *reinterpret_cast<u32x2 *>(dst + 64) = lo;
}

// grid: ceil(m / 4) workgroups of 4 waves; wave w owns row 4 blockIdx.x + w; c % 32 == 0, c <= 256 RV
template <int RV>
__global__ __launch_bounds__(256) void k_postnorm_rows(const float *x, const float *__restrict__ y, int64_t m, int c,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                       float *out, char *__restrict__ out_t, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const int nv = c >> 2;
    const f32x4 *yr = reinterpret_cast<const f32x4 *>(y + row * c);
    f32x4 v[RV];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < RV; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < nv ? yr[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    }
    const float mean = wave_sum(s) / (float)c;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < RV; ++j) {
        if (lane + 64 * j < nv) {
            const float d0 = v[j][0] - mean, d1 = v[j][1] - mean, d2 = v[j][2] - mean, d3 = v[j][3] - mean;
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)c + eps);
    const f32x4 *xr = reinterpret_cast<const f32x4 *>(x + row * c);
    f32x4 *orow = reinterpret_cast<f32x4 *>(out + row * c);
    char *trow = out_t ? out_t + row * ((int64_t)c * 4) : nullptr;
#pragma unroll
    for (int j = 0; j < RV; ++j) {
        const int i = lane + 64 * j;
        if (i >= nv) continue;
        const f32x4 g = reinterpret_cast<const f32x4 *>(gamma)[i], b = reinterpret_cast<const f32x4 *>(beta)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[j][e] - mean) * rstd * g[e] + b[e];
        if (x) {
            const f32x4 r = xr[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = r[e] + o[e];
        }
        orow[i] = o;
        if (trow) put_terms4(trow, i, o, scale);
    }
}

// one thread per 4 output features: output row r = (image, i, j), feature 4 v of 4 c: quad q = 4 v / c in timm's order
// (dy = q & 1, dx = q >> 1), channel 4 v % c of pixel (2 i + dy, 2 j + dx)
__global__ __launch_bounds__(256) void k_patch_merge(const float *__restrict__ x, int64_t total, int h, int w, int c, float scale,
                                                     char *__restrict__ out_t) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= total) return;
    const int64_t orow = item / c;
    const int v = (int)(item - orow * c);
    const int q = (4 * v) / c, ch = 4 * v - q * c;
    const int dy = q & 1, dx = q >> 1;
    const int ho = h >> 1, wo = w >> 1;
    const int64_t im = orow / ((int64_t)ho * wo);
    const int rem = (int)(orow - im * ho * wo), i = rem / wo, j = rem - (rem / wo) * wo;
    const int64_t src = (im * h + 2 * i + dy) * w + 2 * j + dx;
    const f32x4 val = *reinterpret_cast<const f32x4 *>(x + src * c + ch);
    put_terms4(out_t + orow * ((int64_t)c * 16), v, val, scale);
}

}  // namespace

hipError_t launch_postnorm_rows(const float *x, const float *y, int64_t m, int c, const float *gamma, const float *beta, float eps,
                                float *out, void *out_t, float scale, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (c < 32 || c % 32 || c > 1024) return hipErrorInvalidValue;
    const int64_t blocks = (m + 3) / 4;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    char *ot = reinterpret_cast<char *>(out_t);
    if (c <= 256)
        hipLaunchKernelGGL(k_postnorm_rows<1>, dim3((unsigned)blocks), dim3(256), 0, st, x, y, m, c, gamma, beta, eps, out, ot, scale);
    else if (c <= 512)
        hipLaunchKernelGGL(k_postnorm_rows<2>, dim3((unsigned)blocks), dim3(256), 0, st, x, y, m, c, gamma, beta, eps, out, ot, scale);
    else
        hipLaunchKernelGGL(k_postnorm_rows<4>, dim3((unsigned)blocks), dim3(256), 0, st, x, y, m, c, gamma, beta, eps, out, ot, scale);
    return hipGetLastError();
}

hipError_t launch_patch_merge(const float *x, int64_t n, int h, int w, int c, float scale, void *out_t, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (h < 2 || w < 2 || h % 2 || w % 2 || c < 8 || c % 8) return hipErrorInvalidValue;
    const int64_t total = n * (h / 2) * (w / 2) * (int64_t)c;       // 4-feature items: 4 c / 4 per output row
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_patch_merge, dim3((unsigned)blocks), dim3(256), 0, st, x, total, h, w, c, scale,
                       reinterpret_cast<char *>(out_t));
    return hipGetLastError();
}

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

extern "C" int mirx_swin_postnorm(const float *x_or_null, const float *y, int64_t m, int c, const float *gamma, const float *beta,
                                  float eps, float *out, void *out_terms_or_null, float terms_scale, void *stream) {
    MIRX_CHECK(m >= 0 && c >= 32 && c % 32 == 0 && c <= 1024, "swin_postnorm: c must be a multiple of 32, at most 1024");
    MIRX_CHECK(m == 0 || (y && gamma && beta && out), "swin_postnorm: null buffer");
    MIRX_CHECK(eps >= 0.f && (!out_terms_or_null || terms_scale > 0.f), "swin_postnorm: eps >= 0 and terms_scale > 0");
    MIRX_CHECK(y != out, "swin_postnorm: out may alias x, not y");
    MIRX_CHECK(((uintptr_t)x_or_null | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out |
                (uintptr_t)out_terms_or_null) % 16 == 0, "swin_postnorm: buffers must be 16-byte aligned");
    MIRX_HIP(launch_postnorm_rows(x_or_null, y, m, c, gamma, beta, eps, out, out_terms_or_null, terms_scale,
                                  reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

extern "C" int mirx_patch_merge_terms(const float *x, int64_t n, int h, int w, int c, float scale, void *out_terms, void *stream) {
    MIRX_CHECK(n >= 0 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "patch_merge: h and w must be even");
    MIRX_CHECK(c >= 8 && c % 8 == 0, "patch_merge: c must be a multiple of 8");
    MIRX_CHECK(scale > 0.f, "patch_merge: scale must be positive");
    MIRX_CHECK(n == 0 || (x && out_terms), "patch_merge: null buffer");
    MIRX_CHECK(((uintptr_t)x | (uintptr_t)out_terms) % 16 == 0, "patch_merge: buffers must be 16-byte aligned");
    MIRX_HIP(launch_patch_merge(x, n, h, w, c, scale, out_terms, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}
