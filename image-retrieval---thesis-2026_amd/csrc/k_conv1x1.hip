// k_conv1x1.hip -- DenseNet dense-layer front half as ONE fp32 MFMA kernel:
//     y = act_out( W * act_in(x) + bias )        (1x1 convolution = GEMM over channels)
// with act_in(x)[k] = relu(x[k] * scale[k] + shift[k]) applied while the activation tile is staged
// (norm1 + relu1 of torchvision's _DenseLayer) and act_out = relu (norm2's shift is the bias, its
// scale is folded into W by the caller) -- so the concatenated feature buffer is read ONCE per layer
// instead of three times (BN pass, ReLU pass, conv read).  Replaces norm1 -> relu1 -> conv1 -> norm2
// -> relu2 of model.py:53's densenet121 (and, with the prologue off, the transition 1x1 conv).
//
// x is the channel-prefix view of the block buffer: image b, channel k, pixel p at
// x[b * x_batch_stride + k * hw + p].  y is packed NCHW [n, cout, hw].
//
// v_mfma_f32_32x32x2_f32 (exact fp32 FMA chain, 64 FLOP/clk/SIMD): workgroup tile = 128 output
// channels x 64 pixels, 4 waves as 2 (channels) x 2 (pixels), K staged 16 channels at a time through
// a double-buffered LDS image (A = W^T [k][128], B = act [k][64], 16 channels per stage); both operand reads are one
// ds_read_b32 per lane with consecutive lanes on consecutive words (conflict-free).
#include <cstdlib>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int CM = 128;   // output channels per workgroup

// NREP = 32-pixel tiles per wave: workgroup tile = 128 channels x (64 * NREP) pixels
template <bool VEC4, bool PROLOGUE, bool RELU_OUT, int NREP, int KC>
__global__ __launch_bounds__(256) void k_conv1x1(const float *__restrict__ x, int64_t xbs, int cin,
                                                 const float *__restrict__ scale,
                                                 const float *__restrict__ shift,
                                                 const float *__restrict__ wt, const float *__restrict__ bias,
                                                 int64_t n, int hw, int cout, float *__restrict__ y) {
    constexpr int CP = 64 * NREP;
    __shared__ __attribute__((aligned(16))) float sA[2][KC][CM];
    __shared__ __attribute__((aligned(16))) float sB[2][KC][CP];
    __shared__ float sBias[CM];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t total = n * (int64_t)hw;
    const int64_t p0 = (int64_t)blockIdx.x * CP;
    const int co0 = blockIdx.y * CM;

    // Staging assignments.  A (weights): thread -> rows a_k and a_k + 8, channels 4 a_m4 .. +3.
    // B (activations), VEC4: thread -> row b_k, pixels 4 b_p4 .. +3; scalar path (7x7 maps, hw % 4 != 0):
    // thread -> pixel tid % 64, rows tid / 64 + 4 i.  Out-of-range pixels read pixel 0 (never stored).
    // With NREP = 2 (128-pixel tile, VEC4 only) a thread stages rows b_k and b_k + 8 of its 4 pixels.
    static_assert(KC == 16 && (NREP == 1 || (NREP == 2 && VEC4)), "staging below is written for 16-channel stages");
    const int a_k = threadIdx.x >> 5, a_m4 = threadIdx.x & 31;
    const int b_k = VEC4 ? threadIdx.x / (16 * NREP) : threadIdx.x >> 6;
    const int b_p = VEC4 ? 4 * (threadIdx.x % (16 * NREP)) : threadIdx.x & 63;
    int64_t b_off = 0;
    {
        const int64_t pp = p0 + b_p;
        if (pp < total) b_off = (pp / hw) * xbs + (pp % hw);
    }
    const float *wsrc = wt + (int64_t)a_k * cout + co0 + 4 * a_m4;
    const float *xsrc = x + b_off + (int64_t)b_k * hw;

    // Register-prefetched, branch-free pipeline: the global loads of stage kt+1 are issued before the
    // MFMAs of stage kt and written to the idle LDS buffer after them (the last iteration re-stages its
    // own K slice into the idle buffer, which nobody reads).
    float4 ra0, ra1, rb, rb2;
    float rs0, rs1, rs2, rs3, sc0 = 1.f, sh0 = 0.f, sc1 = 1.f, sh1 = 0.f, sc2 = 1.f, sh2 = 0.f, sc3 = 1.f, sh3 = 0.f;
#define MIRX_C1_LOAD(k0)                                                                           \
    do {                                                                                           \
        ra0 = *reinterpret_cast<const float4 *>(wsrc + (int64_t)(k0) * cout);                      \
        ra1 = *reinterpret_cast<const float4 *>(wsrc + (int64_t)((k0) + 8) * cout);                \
        if (VEC4) {                                                                                \
            rb = *reinterpret_cast<const float4 *>(xsrc + (int64_t)(k0) * hw);                     \
            if (PROLOGUE) { sc0 = scale[(k0) + b_k]; sh0 = shift[(k0) + b_k]; }                    \
            if (NREP == 2) {                                                                       \
                rb2 = *reinterpret_cast<const float4 *>(xsrc + (int64_t)((k0) + 8) * hw);          \
                if (PROLOGUE) { sc1 = scale[(k0) + b_k + 8]; sh1 = shift[(k0) + b_k + 8]; }        \
            }                                                                                      \
        } else {                                                                                   \
            rs0 = xsrc[(int64_t)(k0) * hw];                                                        \
            rs1 = xsrc[(int64_t)((k0) + 4) * hw];                                                  \
            rs2 = xsrc[(int64_t)((k0) + 8) * hw];                                                  \
            rs3 = xsrc[(int64_t)((k0) + 12) * hw];                                                 \
            if (PROLOGUE) {                                                                        \
                sc0 = scale[(k0) + b_k]; sh0 = shift[(k0) + b_k];                                  \
                sc1 = scale[(k0) + b_k + 4]; sh1 = shift[(k0) + b_k + 4];                          \
                sc2 = scale[(k0) + b_k + 8]; sh2 = shift[(k0) + b_k + 8];                          \
                sc3 = scale[(k0) + b_k + 12]; sh3 = shift[(k0) + b_k + 12];                        \
            }                                                                                      \
        }                                                                                          \
    } while (0)
#define MIRX_C1_ACT(v, sc, sh) (PROLOGUE ? fmaxf(fmaf((v), (sc), (sh)), 0.f) : (v))
#define MIRX_C1_STORE(buf)                                                                         \
    do {                                                                                           \
        *reinterpret_cast<float4 *>(&sA[buf][a_k][4 * a_m4]) = ra0;                                \
        *reinterpret_cast<float4 *>(&sA[buf][a_k + 8][4 * a_m4]) = ra1;                            \
        if (VEC4) {                                                                                \
            float4 v;                                                                              \
            v.x = MIRX_C1_ACT(rb.x, sc0, sh0); v.y = MIRX_C1_ACT(rb.y, sc0, sh0);                  \
            v.z = MIRX_C1_ACT(rb.z, sc0, sh0); v.w = MIRX_C1_ACT(rb.w, sc0, sh0);                  \
            *reinterpret_cast<float4 *>(&sB[buf][b_k][b_p]) = v;                                   \
            if (NREP == 2) {                                                                       \
                v.x = MIRX_C1_ACT(rb2.x, sc1, sh1); v.y = MIRX_C1_ACT(rb2.y, sc1, sh1);            \
                v.z = MIRX_C1_ACT(rb2.z, sc1, sh1); v.w = MIRX_C1_ACT(rb2.w, sc1, sh1);            \
                *reinterpret_cast<float4 *>(&sB[buf][b_k + 8][b_p]) = v;                           \
            }                                                                                      \
        } else {                                                                                   \
            sB[buf][b_k][b_p] = MIRX_C1_ACT(rs0, sc0, sh0);                                        \
            sB[buf][b_k + 4][b_p] = MIRX_C1_ACT(rs1, sc1, sh1);                                    \
            sB[buf][b_k + 8][b_p] = MIRX_C1_ACT(rs2, sc2, sh2);                                    \
            sB[buf][b_k + 12][b_p] = MIRX_C1_ACT(rs3, sc3, sh3);                                   \
        }                                                                                          \
    } while (0)

    f32x16 acc[2][NREP];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < NREP; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int nk = cin / KC;
    if (threadIdx.x < CM) sBias[threadIdx.x] = bias ? bias[co0 + threadIdx.x] : 0.f;
    MIRX_C1_LOAD(0);
    MIRX_C1_STORE(0);
    const int kh = lane >> 5, nn = wn * 32 * NREP + (lane & 31), m0 = wm * 64 + (lane & 31);
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        __syncthreads();                                   // stage kt visible; buffer cur^1 free
        const int knext = (kt + 1 < nk ? kt + 1 : kt) * KC;
        MIRX_C1_LOAD(knext);
        __builtin_amdgcn_sched_barrier(0);                 // keep the loads ahead of the MFMAs
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk) {
            float bv[NREP];
#pragma unroll
            for (int ni = 0; ni < NREP; ++ni) bv[ni] = sB[cur][2 * kk + kh][nn + 32 * ni];
            const float a0 = sA[cur][2 * kk + kh][m0];
            const float a1 = sA[cur][2 * kk + kh][m0 + 32];
#pragma unroll
            for (int ni = 0; ni < NREP; ++ni) {
                acc[0][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[ni], acc[0][ni], 0, 0, 0);
                acc[1][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[ni], acc[1][ni], 0, 0, 0);
            }
        }
        MIRX_C1_STORE(cur ^ 1);
    }
#undef MIRX_C1_LOAD
#undef MIRX_C1_STORE
#undef MIRX_C1_ACT

    // epilogue: register r of tile (mi, ni) = channel co0 + 64 wm + 32 mi + (r&3) + 8 (r>>2) + 4 (lane>>5),
    // pixel p0 + 32 NREP wn + 32 ni + (lane & 31)
#pragma unroll
    for (int ni = 0; ni < NREP; ++ni) {
        const int64_t pp = p0 + wn * 32 * NREP + 32 * ni + (lane & 31);
        if (pp >= total) continue;
        const int64_t bimg = pp / hw, off = pp % hw;
        float *yo = y + bimg * (int64_t)cout * hw + off;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = co0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = acc[mi][ni][r] + sBias[ch - co0];
                if (RELU_OUT) v = fmaxf(v, 0.f);
                yo[(int64_t)ch * hw] = v;
            }
    }
}

template <bool VEC4, int NREP, int KC>
hipError_t launch_v(const float *x, int64_t xbs, int cin, const float *scale, const float *shift, const float *wt,
                    const float *bias, int64_t n, int hw, int cout, int relu_out, float *y, hipStream_t st) {
    constexpr int CP = 64 * NREP;
    const dim3 grid((unsigned)((n * (int64_t)hw + CP - 1) / CP), (unsigned)(cout / CM));
#define MIRX_C1(P, R)                                                                                       \
    hipLaunchKernelGGL((k_conv1x1<VEC4, P, R, NREP, KC>), grid, dim3(256), 0, st, x, xbs, cin, scale, shift, wt, bias, n, \
                       hw, cout, y)
    if (scale) {
        if (relu_out) MIRX_C1(true, true); else MIRX_C1(true, false);
    } else {
        if (relu_out) MIRX_C1(false, true); else MIRX_C1(false, false);
    }
#undef MIRX_C1
    return hipGetLastError();
}

}  // namespace

hipError_t launch_conv1x1(const float *x, int64_t xbs, int cin, const float *scale, const float *shift,
                          const float *wt, const float *bias, int64_t n, int hw, int cout, int relu_out, float *y,
                          hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (cin % 32 || cout % CM) return hipErrorInvalidValue;
    // Tile choice, measured on DenseNet-121 end to end: 64 pixels x 16 channels per stage (24 KiB LDS, 6
    // workgroups per CU) is the default; 64 x 32 and 64 x 8 channel stages were 3-5 % slower.  A 128-pixel
    // tile (NREP = 2, weights reused twice, MIRX_C1_NREP=2) is within 1.5 % either way per layer since the
    // K loop prefetches through registers (24.8 vs 25.1 ms over the 61 launches of a 1024-image forward).
    if ((hw & 3) == 0 && (xbs & 3) == 0) {
        static const int nrep = [] { const char *e = getenv("MIRX_C1_NREP"); return e && e[0] == '2' ? 2 : 1; }();
        if (nrep == 2) return launch_v<true, 2, 16>(x, xbs, cin, scale, shift, wt, bias, n, hw, cout, relu_out, y, st);
        return launch_v<true, 1, 16>(x, xbs, cin, scale, shift, wt, bias, n, hw, cout, relu_out, y, st);
    }
    return launch_v<false, 1, 16>(x, xbs, cin, scale, shift, wt, bias, n, hw, cout, relu_out, y, st);
}

}  // namespace mirx
