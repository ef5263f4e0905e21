// k_sbsm.hip -- SBSM sliding-window occlusion saliency without materialised masks (gfx950, wave64; include/mirx.h).
//
// SBSM occludes one window of an image at a time, embeds every occluded image and credits each pixel with the mean embedding
// distance gain of the windows that cover it.  The windows of a sliding-window set are the outer product of nr row intervals and
// nc column intervals (clipped, half-open): mask n = i * nc + j zeroes row_iv[i] x col_iv[j].  Two small int32 arrays describe
// what the reference keeps as a uint8 [N, 1, H, W] tensor and the torch path as a dense fp32 [HW, N] matrix.  Three entry points:
//   1. compose     k_sb_compose: images [g0, g0 + n) of the n-major job list (image g = mask g / B on image g % B).  Every
//                  value is the IEEE product x * (inside ? 0.0f : 1.0f): the bits of torch's mask.float() * x, -0.0 and the NaN
//                  of inf * 0 included.  A thread owns four consecutive floats of the [C, H, W] image (16-byte loads and
//                  stores) when C * H * W % 4 == 0 and the buffers are 16-byte aligned, one float otherwise; (y, x) is divided
//                  out once per group and stepped along it.
//   2. gain        k_sb_gain: one wave per (row, mask).  Differences, squares, the sum (lane-strided fma, then
//                  wave_butterfly_sum) and the root in fp64.  Pairs subtract the unmasked distance, recomputed by the same wave
//                  in the same order, and clamp at 0 keeping a NaN.
//   3. accumulate  k_sb_cols then k_sb_rows: the sum over the covering windows is separable.  k_sb_cols: T[r, i, x] = sum over
//                  the column intervals j that hold x, j ascending, of gain[r, i * nc + j] (fp64, workspace).  k_sb_rows:
//                  sal[r, y, x] = fp32((sum over the row intervals i that hold y, i ascending, of T[r, i, x]) / (cr[y] * cc[x]))
//                  with cr / cc the interval counts: 0 / 0 = NaN where no window covers.  A gain is ADDED where its window
//                  covers, never multiplied by 0 where it does not.
// The interval arrays are device data the host never reads: the kernels only COMPARE against them (no address is derived from
// an interval), so any content stays in bounds.  No host synchronisation, no atomic; launch boundaries are the only
// synchronisation between workgroups, every sum has a fixed order: repeated calls are bit-identical.
//
// Reference behaviour replaced: SBSMBatch.forward / weighted_avg (explanations.py:75-79, 105-152).
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

#include <algorithm>

namespace mirx {

namespace {

constexpr int SB_THREADS = 256;

// ---- 1. compose -------------------------------------------------------------------------------------------------------------
template <int VEC> struct SbVec;
template <> struct SbVec<4> { typedef f32x4 vals; };
template <> struct SbVec<1> { typedef float vals; };

__device__ inline float &sb_at(f32x4 &v, int e) { return reinterpret_cast<float *>(&v)[e]; }
__device__ inline float &sb_at(float &v, int) { return v; }

template <int VEC>
__global__ __launch_bounds__(SB_THREADS) void k_sb_compose(const float *__restrict__ x, int64_t b_imgs, int chw, int h, int w,
                                                           const int32_t *__restrict__ row_iv, const int32_t *__restrict__ col_iv,
                                                           int nc, int64_t g0, int64_t n, float *__restrict__ out) {
    typedef typename SbVec<VEC>::vals vals_t;
    const int hw = h * w, groups = chw / VEC;
    for (int64_t img = blockIdx.y; img < n; img += gridDim.y) {
        const int64_t g = g0 + img, m = g / b_imgs, b = g - m * b_imgs;
        const int i = (int)(m / nc), j = (int)(m - (int64_t)i * nc);
        const int r0 = row_iv[2 * i], r1 = row_iv[2 * i + 1], c0 = col_iv[2 * j], c1 = col_iv[2 * j + 1];
        const vals_t *src = reinterpret_cast<const vals_t *>(x + b * chw);
        vals_t *dst = reinterpret_cast<vals_t *>(out + img * chw);
        for (int gi = blockIdx.x * SB_THREADS + threadIdx.x; gi < groups; gi += gridDim.x * SB_THREADS) {
            const int pix = (gi * VEC) % hw;
            int yy = pix / w, xx = pix - yy * w;
            vals_t v = src[gi];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const bool inside = yy >= r0 && yy < r1 && xx >= c0 && xx < c1;
                sb_at(v, e) = sb_at(v, e) * (inside ? 0.0f : 1.0f);
                if (++xx == w) {
                    xx = 0;
                    if (++yy == h) yy = 0;                               // the group runs on into the next channel
                }
            }
            dst[gi] = v;
        }
    }
}

// ---- 2. gain ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SB_THREADS) void k_sb_gain(const float *__restrict__ e_q, const float *__restrict__ e_m,
                                                        const float *__restrict__ e_r, int64_t n_masks, int64_t b_imgs, int d,
                                                        int64_t total, double *__restrict__ gain) {
    const int lane = lane_id();
    const int64_t idx = (int64_t)blockIdx.x * (SB_THREADS / WAVE) + (threadIdx.x >> 6);
    if (idx >= total) return;                                            // wave-uniform
    const int64_t r = idx / n_masks, n = idx - r * n_masks;
    const int64_t q = e_r ? r / b_imgs : r, b = e_r ? r - q * b_imgs : r;
    const float *pq = e_q + q * d, *pm = e_m + (n * b_imgs + b) * d;
    double sm = 0.0, so = 0.0;
    if (e_r) {
        const float *pr = e_r + b * d;
        for (int e = lane; e < d; e += WAVE) {
            const double a = (double)pq[e];
            const double dm = a - (double)pm[e], dr = a - (double)pr[e];
            sm = fma(dm, dm, sm);
            so = fma(dr, dr, so);
        }
        so = wave_butterfly_sum(so);
    } else {
        for (int e = lane; e < d; e += WAVE) {
            const double dm = (double)pq[e] - (double)pm[e];
            sm = fma(dm, dm, sm);
        }
    }
    sm = wave_butterfly_sum(sm);
    if (lane == 0) {
        double v = sqrt(sm);
        if (e_r) {
            v -= sqrt(so);
            v = (v > 0.0 || v != v) ? v : 0.0;                          // clamp(min=0): a NaN stays
        }
        gain[idx] = v;
    }
}

// ---- 3. accumulate ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SB_THREADS) void k_sb_cols(const double *__restrict__ gain, int64_t rows, int nr, int nc, int w,
                                                        const int32_t *__restrict__ col_iv, double *__restrict__ t) {
    const int cells = nr * w;                                            // <= 4096 * 2^20 / h: checked < 2^31 by the ABI
    const int64_t n_masks = (int64_t)nr * nc;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        for (int c = blockIdx.x * SB_THREADS + threadIdx.x; c < cells; c += gridDim.x * SB_THREADS) {
            const int i = c / w, xx = c - i * w;
            const double *gr = gain + r * n_masks + (int64_t)i * nc;
            double acc = 0.0;
            for (int j = 0; j < nc; ++j)
                if (xx >= col_iv[2 * j] && xx < col_iv[2 * j + 1]) acc += gr[j];
            t[r * cells + c] = acc;
        }
    }
}

__global__ __launch_bounds__(SB_THREADS) void k_sb_rows(const double *__restrict__ t, int64_t rows, int nr, int nc, int h, int w,
                                                        const int32_t *__restrict__ row_iv, const int32_t *__restrict__ col_iv,
                                                        float *__restrict__ sal) {
    const int hw = h * w;
    const int64_t cells = (int64_t)nr * w;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        for (int p = blockIdx.x * SB_THREADS + threadIdx.x; p < hw; p += gridDim.x * SB_THREADS) {
            const int yy = p / w, xx = p - yy * w;
            int cc = 0, cr = 0;
            for (int j = 0; j < nc; ++j) cc += (xx >= col_iv[2 * j] && xx < col_iv[2 * j + 1]) ? 1 : 0;
            const double *tr = t + r * cells + xx;
            double acc = 0.0;
            for (int i = 0; i < nr; ++i)
                if (yy >= row_iv[2 * i] && yy < row_iv[2 * i + 1]) {
                    acc += tr[(int64_t)i * w];
                    ++cr;
                }
            sal[r * hw + p] = (float)(acc / ((double)cr * (double)cc));
        }
    }
}

}  // namespace

hipError_t launch_sbsm_compose(const float *x, int64_t b, int c, int h, int w, const int32_t *row_iv, const int32_t *col_iv, int nc,
                               int64_t g0, int64_t n, float *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int chw = c * h * w;
    const bool vec = chw % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int groups = vec ? chw / 4 : chw;
    const dim3 grid((unsigned)std::min((groups + SB_THREADS - 1) / SB_THREADS, 1024), (unsigned)std::min<int64_t>(n, 65535));
    if (vec)
        hipLaunchKernelGGL(k_sb_compose<4>, grid, dim3(SB_THREADS), 0, st, x, b, chw, h, w, row_iv, col_iv, nc, g0, n, out);
    else
        hipLaunchKernelGGL(k_sb_compose<1>, grid, dim3(SB_THREADS), 0, st, x, b, chw, h, w, row_iv, col_iv, nc, g0, n, out);
    return hipGetLastError();
}

hipError_t launch_sbsm_gain(const float *e_q, const float *e_m, const float *e_r, int64_t rows, int64_t n_masks, int64_t b, int d,
                            double *gain, hipStream_t st) {
    const int64_t total = rows * n_masks;
    const int per = SB_THREADS / WAVE;
    hipLaunchKernelGGL(k_sb_gain, dim3((unsigned)((total + per - 1) / per)), dim3(SB_THREADS), 0, st, e_q, e_m, e_r, n_masks, b, d,
                       total, gain);
    return hipGetLastError();
}

int64_t sbsm_workspace_bytes(int64_t rows, int nr, int w) { return rows * nr * (int64_t)w * (int64_t)sizeof(double); }

hipError_t launch_sbsm_accumulate(const double *gain, int64_t rows, const int32_t *row_iv, int nr, const int32_t *col_iv, int nc, int h,
                                  int w, void *workspace, float *sal, hipStream_t st) {
    double *t = reinterpret_cast<double *>(workspace);
    const unsigned gy = (unsigned)std::min<int64_t>(rows, 65535);
    const int64_t cells = (int64_t)nr * w, hw = (int64_t)h * w;
    hipLaunchKernelGGL(k_sb_cols, dim3((unsigned)std::min<int64_t>((cells + SB_THREADS - 1) / SB_THREADS, 65536), gy), dim3(SB_THREADS),
                       0, st, gain, rows, nr, nc, w, col_iv, t);
    hipLaunchKernelGGL(k_sb_rows, dim3((unsigned)std::min<int64_t>((hw + SB_THREADS - 1) / SB_THREADS, 65536), gy), dim3(SB_THREADS), 0,
                       st, t, rows, nr, nc, h, w, row_iv, col_iv, sal);
    return hipGetLastError();
}

}  // namespace mirx
