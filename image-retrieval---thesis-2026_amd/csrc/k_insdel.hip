// k_insdel.hip -- the insertion / deletion game of one query as one device job (gfx950, wave64; include/mirx.h).
//
// A curve modifies `step` pixels of an image per step, most salient first, and scores every intermediate image against the
// query.  Image s of a curve is where(t < s, finish, start) with t[p] = rank of pixel p in decreasing saliency / step, so all
// images of all curves of a query are known up front.  Four entry points:
//   1. steps    k_id_build -> launch_rank_sort (k_ranksort.hip, the low 32 key bits) -> k_id_steps
//               key = a 32-bit image of the fp32 saliency that ascends as the value descends (-0.0 as +0.0, every NaN before
//               +inf), payload = the pixels in DESCENDING index order: the sort is stable, so equal values keep that order.
//               That is np.flip(np.argsort(sal, kind="stable")).  t[payload[j]] = j / step.
//   2. blur     k_blur2d: zero-padded cross-correlation of every plane with one [klen, klen] kernel.  A workgroup owns a
//               32 x 32 output tile; the (32 + klen - 1)^2 input patch and the taps (as fp64) sit in LDS.  A thread owns four
//               consecutive pixels of a row and slides a four-value window along the patch row: per tap one 4-byte LDS read, one
//               broadcast tap read and four fp64 FMAs.  Products of two fp32 values are exact in fp64 and the taps are added in
//               (ky, kx) order, so a pixel is the correctly rounded sum up to ~klen^2 * 2^-53: its bits depend on its own
//               plane alone, never on n or on the tile it falls in.
//               LDS banking: ds_read_b32 conflicts are per 32-lane half over 32 banks.  A half is 8 threads along x (4 dwords
//               apart) by 4 rows; the patch row stride is odd, so row r adds r (mod 4) to a multiple of 4: 32 distinct banks.
//   3. compose  k_id_compose: images [g0, g0 + n) of the job's flat image list, a bit-exact select on 32-bit patterns; t is read
//               once per group of four pixels (16 bytes) and reused for the three channels, 16-byte loads and stores.
//   4. curves   k_id_cos (one wave per image: fp64 cosine of fp32 rows, norms clamped at 1e-8) and k_id_auc (one workgroup per
//               curve: negatives counted and set to 0, the area summed in index order by one thread).
// No host synchronisation, no floating atomic; launch boundaries are the only synchronisation between workgroups.
//
// Reference behaviour replaced: CausalMetric.single_run (evaluation.py:65-138) / the milvus driver's evaluate
// (evaluate_test_dataset_milvus.py:32-85) called twice per hit by InsDel (evaluate_saliency.py:33-91).
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

#include <algorithm>

namespace mirx {

namespace {

constexpr int ID_THREADS = 256;

size_t id_align256(size_t v) { return (v + 255) & ~(size_t)255; }
unsigned id_grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + ID_THREADS - 1) / ID_THREADS, 4096); }

// ---- 1. steps ---------------------------------------------------------------------------------------------------------------
// key(a) < key(b) iff a > b; -0.0 takes +0.0's key; every NaN takes the key of the positive quiet NaN, which is below +inf's.
__device__ inline uint32_t saliency_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (v != v) u = 0x7fc00000u;
    if ((u << 1) == 0) u = 0;
    return (u >> 31) ? u : (~u ^ 0x80000000u);
}

__global__ __launch_bounds__(ID_THREADS) void k_id_build(const float *__restrict__ sal, int64_t hw, uint64_t *__restrict__ keys,
                                                         int32_t *__restrict__ pay) {
    const int64_t k = blockIdx.y;
    for (int64_t j = (int64_t)blockIdx.x * ID_THREADS + threadIdx.x; j < hw; j += (int64_t)gridDim.x * ID_THREADS) {
        const int64_t p = hw - 1 - j;
        keys[k * hw + j] = (uint64_t)saliency_key(sal[k * hw + p]);
        pay[k * hw + j] = (int32_t)p;
    }
}

__global__ __launch_bounds__(ID_THREADS) void k_id_steps(const int32_t *__restrict__ pay, int64_t hw, int32_t step,
                                                         int32_t *__restrict__ t) {
    const int64_t k = blockIdx.y;
    for (int64_t j = (int64_t)blockIdx.x * ID_THREADS + threadIdx.x; j < hw; j += (int64_t)gridDim.x * ID_THREADS) {
        const int32_t p = pay[k * hw + j];
        if ((uint32_t)p < (uint64_t)hw) t[k * hw + p] = (int32_t)j / step;      // always, for a sorted payload: keeps a bug in bounds
    }
}

// ---- 2. blur ----------------------------------------------------------------------------------------------------------------
constexpr int BL_TILE = 32;          // output tile side
constexpr int BL_PX = 4;             // consecutive pixels of a row per thread
static_assert(BL_TILE / BL_PX * BL_TILE == ID_THREADS, "one thread per four pixels of the tile");

__host__ __device__ inline int blur_patch_stride(int klen) { return (BL_TILE + klen - 1) | 1; }
size_t blur_lds_bytes(int klen) {
    return (size_t)klen * klen * sizeof(double) + (size_t)(BL_TILE + klen - 1) * blur_patch_stride(klen) * sizeof(float);
}

__global__ __launch_bounds__(ID_THREADS) void k_blur2d(const float *__restrict__ x, const float *__restrict__ kern, int h, int w,
                                                       int klen, int ntx, int nty, float *__restrict__ y) {
    extern __shared__ double bl_lds[];
    double *taps = bl_lds;                                               // [klen][klen]
    float *patch = reinterpret_cast<float *>(taps + klen * klen);        // [BL_TILE + klen - 1][stride]
    const int pad = klen >> 1, side = BL_TILE + klen - 1, stride = blur_patch_stride(klen);
    const int64_t bid = blockIdx.x;
    const int x0 = (int)(bid % ntx) * BL_TILE, y0 = (int)((bid / ntx) % nty) * BL_TILE;
    const int64_t plane = bid / ((int64_t)ntx * nty);
    const float *xp = x + plane * (int64_t)h * w;

    for (int i = threadIdx.x; i < klen * klen; i += ID_THREADS) taps[i] = (double)kern[i];
    for (int r = threadIdx.x / 32; r < side; r += ID_THREADS / 32) {
        const int gy = y0 + r - pad;
        const bool row_in = gy >= 0 && gy < h;
        for (int c = threadIdx.x % 32; c < side; c += 32) {
            const int gx = x0 + c - pad;
            patch[r * stride + c] = (row_in && gx >= 0 && gx < w) ? xp[(int64_t)gy * w + gx] : 0.f;
        }
    }
    __syncthreads();

    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const int oy = y0 + ty, ox = x0 + tx * BL_PX;
    if (oy >= h || ox >= w) return;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    for (int ky = 0; ky < klen; ++ky) {
        const float *p = patch + (ty + ky) * stride + tx * BL_PX;
        const double *wr = taps + ky * klen;
        double a0 = (double)p[0], a1 = (double)p[1], a2 = (double)p[2];
#pragma unroll 4
        for (int kx = 0; kx < klen; ++kx) {
            const double a3 = (double)p[kx + 3];
            const double wv = wr[kx];
            acc0 = fma(wv, a0, acc0);
            acc1 = fma(wv, a1, acc1);
            acc2 = fma(wv, a2, acc2);
            acc3 = fma(wv, a3, acc3);
            a0 = a1; a1 = a2; a2 = a3;
        }
    }
    float *yp = y + plane * (int64_t)h * w + (int64_t)oy * w + ox;
    const f32x4 o = {(float)acc0, (float)acc1, (float)acc2, (float)acc3};
    if (ox + BL_PX <= w && (reinterpret_cast<uintptr_t>(yp) & 15) == 0) {
        *reinterpret_cast<f32x4 *>(yp) = o;
    } else {
#pragma unroll
        for (int i = 0; i < BL_PX; ++i)
            if (ox + i < w) yp[i] = o[i];
    }
}

// ---- 3. compose -------------------------------------------------------------------------------------------------------------
// VEC = 4: hw % 4 == 0 and 16-byte aligned buffers, a thread handles four pixels of the three channels; VEC = 1: any hw.
template <int VEC> struct IdVec;
template <> struct IdVec<4> { typedef u32x4 bits; typedef __attribute__((ext_vector_type(4))) int steps; };
template <> struct IdVec<1> { typedef uint32_t bits; typedef int32_t steps; };

__device__ inline u32x4 id_select(const __attribute__((ext_vector_type(4))) int &tv, int s, const u32x4 &fi, const u32x4 &st) {
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = tv[i] < s ? fi[i] : st[i];
    return o;
}
__device__ inline uint32_t id_select(const int32_t &tv, int s, const uint32_t &fi, const uint32_t &st) { return tv < s ? fi : st; }

template <int VEC>
__global__ __launch_bounds__(ID_THREADS) void k_id_compose(const int32_t *__restrict__ t, int64_t n_rows, int64_t hw,
                                                           const float *__restrict__ bank, int64_t n_bank,
                                                           const int32_t *__restrict__ start, const int32_t *__restrict__ finish,
                                                           const int32_t *__restrict__ row, int64_t per_curve, int64_t g0, int64_t n,
                                                           float *__restrict__ out) {
    typedef typename IdVec<VEC>::bits bits_t;
    typedef typename IdVec<VEC>::steps steps_t;
    const int64_t groups = hw / VEC;
    const bits_t zero = {};
    for (int64_t img = blockIdx.y; img < n; img += gridDim.y) {
        const int64_t g = g0 + img, j = g / per_curve;
        const int s = (int)(g - j * per_curve);
        int64_t st = start[j], fi = finish[j], rw = row[j];
        if (st < -1 || st >= n_bank || fi < -1 || fi >= n_bank || rw < 0 || rw >= n_rows) { st = fi = -1; rw = 0; }   // the ABI checks
        // the arrays' sizes, not their device contents: a bad entry gives the all-zero image and stays in bounds
        const steps_t *tp = reinterpret_cast<const steps_t *>(t + rw * hw);
        for (int64_t gi = (int64_t)blockIdx.x * ID_THREADS + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * ID_THREADS) {
            const steps_t tv = tp[gi];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const bits_t a = st >= 0 ? reinterpret_cast<const bits_t *>(bank + (st * 3 + c) * hw)[gi] : zero;
                const bits_t b = fi >= 0 ? reinterpret_cast<const bits_t *>(bank + (fi * 3 + c) * hw)[gi] : zero;
                reinterpret_cast<bits_t *>(out + (img * 3 + c) * hw)[gi] = id_select(tv, s, b, a);
            }
        }
    }
}

// ---- 4. curves --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ID_THREADS) void k_id_cos(const float *__restrict__ q, const float *__restrict__ r, int64_t rows, int d,
                                                       double *__restrict__ scores) {
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * (ID_THREADS / WAVE) + (threadIdx.x >> 6);
    if (i >= rows) return;
    const float *ri = r + i * d;
    double qr = 0.0, qq = 0.0, rr = 0.0;
    for (int e = lane; e < d; e += WAVE) {
        const double a = (double)q[e], b = (double)ri[e];
        qr = fma(a, b, qr);
        qq = fma(a, a, qq);
        rr = fma(b, b, rr);
    }
    qr = wave_butterfly_sum(qr);
    qq = wave_butterfly_sum(qq);
    rr = wave_butterfly_sum(rr);
    if (lane == 0) scores[i] = qr / (fmax(sqrt(qq), 1e-8) * fmax(sqrt(rr), 1e-8));
}

constexpr int ID_AUC_CHUNK = 2048;
__global__ __launch_bounds__(ID_THREADS) void k_id_auc(double *__restrict__ scores, int64_t n_steps, double *__restrict__ auc,
                                                       int64_t *__restrict__ zero_counter) {
    __shared__ double buf[ID_AUC_CHUNK];
    __shared__ unsigned long long negatives;
    const int64_t len = n_steps + 1;
    double *s = scores + (int64_t)blockIdx.x * len;
    if (threadIdx.x == 0) negatives = 0ull;
    double sum = 0.0, first = 0.0, last = 0.0;                            // thread 0's
    for (int64_t c0 = 0; c0 < len; c0 += ID_AUC_CHUNK) {
        const int m = len - c0 < ID_AUC_CHUNK ? (int)(len - c0) : ID_AUC_CHUNK;
        __syncthreads();
        unsigned mine = 0;
        for (int i = threadIdx.x; i < m; i += ID_THREADS) {
            double v = s[c0 + i];
            if (v < 0.0) {                                                // a NaN is not negative: it stays, as in the reference
                v = 0.0;
                s[c0 + i] = v;
                ++mine;
            }
            buf[i] = v;
        }
        if (mine) atomicAdd(&negatives, (unsigned long long)mine);
        __syncthreads();
        if (threadIdx.x == 0) {
            if (c0 == 0) first = buf[0];
            last = buf[m - 1];
            for (int i = 0; i < m; ++i) sum += buf[i];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        auc[blockIdx.x] = (sum - first / 2 - last / 2) / (double)n_steps;
        zero_counter[blockIdx.x] = (int64_t)negatives;
    }
}

}  // namespace

int64_t insdel_steps_workspace_bytes(int64_t k, int64_t hw) {
    const size_t tot = (size_t)k * hw, tiles = (size_t)k * rank_sort_tiles(hw);
    return (int64_t)(2 * id_align256(tot * 8) + 2 * id_align256(tot * 4) + id_align256(tiles * 256 * 4));
}

hipError_t launch_insdel_steps(const float *sal, int64_t k, int64_t hw, int64_t step, void *workspace, int32_t *t, hipStream_t st) {
    const size_t tot = (size_t)k * hw, tiles = (size_t)k * rank_sort_tiles(hw);
    char *ws = reinterpret_cast<char *>(workspace);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(ws);
    ws += id_align256(tot * 8);
    uint64_t *keys_b = reinterpret_cast<uint64_t *>(ws);
    ws += id_align256(tot * 8);
    int32_t *pay_a = reinterpret_cast<int32_t *>(ws);
    ws += id_align256(tot * 4);
    int32_t *pay_b = reinterpret_cast<int32_t *>(ws);
    ws += id_align256(tot * 4);
    unsigned *hist = reinterpret_cast<unsigned *>(ws);
    (void)tiles;
    const dim3 grid(id_grid_for(hw), (unsigned)k);
    hipLaunchKernelGGL(k_id_build, grid, dim3(ID_THREADS), 0, st, sal, hw, keys_a, pay_a);
    const hipError_t e = launch_rank_sort(keys_a, pay_a, keys_b, pay_b, hist, hw, (int)k, st, 32);
    if (e != hipSuccess) return e;
    const int32_t step32 = (int32_t)std::min<int64_t>(step, INT32_MAX);       // ranks are below 2^20: a larger step gives 0 as well
    hipLaunchKernelGGL(k_id_steps, grid, dim3(ID_THREADS), 0, st, pay_a, hw, step32, t);
    return hipGetLastError();
}

int64_t blur2d_blocks(int64_t planes, int h, int w) {
    return planes * ((w + BL_TILE - 1) / BL_TILE) * (int64_t)((h + BL_TILE - 1) / BL_TILE);
}

hipError_t launch_blur2d_same(const float *x, int64_t planes, int h, int w, const float *kern, int klen, float *y, hipStream_t st) {
    if (planes <= 0) return hipSuccess;
    const int ntx = (w + BL_TILE - 1) / BL_TILE, nty = (h + BL_TILE - 1) / BL_TILE;
    const size_t lds = blur_lds_bytes(klen);                               // 66 KiB at klen = 63, 47 KiB at 51
    const hipError_t e = set_dynamic_lds(k_blur2d, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_blur2d, dim3((unsigned)blur2d_blocks(planes, h, w)), dim3(ID_THREADS), lds, st, x, kern, h, w, klen, ntx, nty,
                       y);
    return hipGetLastError();
}

hipError_t launch_insdel_compose(const int32_t *t, int64_t n_rows, int64_t hw, const float *bank, int64_t n_bank, const int32_t *start,
                                 const int32_t *finish, const int32_t *row, int64_t n_steps, int64_t g0, int64_t n, float *out,
                                 hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const bool vec = hw % 4 == 0 && ((reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(bank) |
                                      reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int64_t groups = vec ? hw / 4 : hw;
    const dim3 grid((unsigned)std::min<int64_t>((groups + ID_THREADS - 1) / ID_THREADS, 1024), (unsigned)std::min<int64_t>(n, 65535));
    if (vec)
        hipLaunchKernelGGL(k_id_compose<4>, grid, dim3(ID_THREADS), 0, st, t, n_rows, hw, bank, n_bank, start, finish, row, n_steps + 1,
                           g0, n, out);
    else
        hipLaunchKernelGGL(k_id_compose<1>, grid, dim3(ID_THREADS), 0, st, t, n_rows, hw, bank, n_bank, start, finish, row, n_steps + 1,
                           g0, n, out);
    return hipGetLastError();
}

hipError_t launch_insdel_curves(const float *q, const float *r, int64_t n_curves, int64_t n_steps, int d, double *scores, double *auc,
                                int64_t *zero_counter, hipStream_t st) {
    const int64_t rows = n_curves * (n_steps + 1);
    const int per = ID_THREADS / WAVE;
    hipLaunchKernelGGL(k_id_cos, dim3((unsigned)((rows + per - 1) / per)), dim3(ID_THREADS), 0, st, q, r, rows, d, scores);
    hipLaunchKernelGGL(k_id_auc, dim3((unsigned)n_curves), dim3(ID_THREADS), 0, st, scores, n_steps, auc, zero_counter);
    return hipGetLastError();
}

}  // namespace mirx
