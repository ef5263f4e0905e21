// k_conv_t2.hip -- general convolution (kernel 1 or 3, stride 1 or 2, "same" padding) over channels-last maps stored as
// TERMS ROWS (include/mirx.h, mirx_linear_terms: one row per pixel, ceil(c / 32) lines of 128 B, fp16 hi | lo of s * x), as
// an implicit GEMM on two fp16 terms per operand: three MFMAs per product block (wl xh + wh xl + wh xh), fp32 accumulation --
// k_linear_t2's arithmetic.  Written for ResNet-50 (mirx.model.ResNet50): its 1x1 / 3x3 convolutions, residual epilogue.
//
//   y[b, oy, ox, o] = epi( oscale[o] / x_scale[b] * sum_{ky, kx, c} xt[b, s oy + ky - p, s ox + kx - p, c] * wt[o, ky, kx, c] )
//   epi(v) = relu?( v + bias[o] (+ residual[b, oy, ox, o]) )
//
// GEMM view: M = output pixels of the whole call (n * ho * wo; a 128-pixel tile may straddle images), N = cout, K = (ky, kx, c)
// in STAGES of 32 channels of one tap -- one 128-byte line of one source pixel per (pixel, stage), so a stage of the pixel
// operand is a gather of whole lines.  Both operands go global -> LDS by `buffer_load ... lds` DMA (no staging registers):
//   * pixel rows: the per-lane offset holds the whole source address (image, row, column, stage) relative to the tile's first
//     image; a padding tap or a pixel beyond M gets an offset past the descriptor, so the load returns zeros (the offset is in
//     the VGPR, which the range check covers; nothing rides in soffset);
//   * weight rows: terms rows of W * ws (ws a power of two per output channel), padded with zero rows to a multiple of 128.
// LDS image of an operand row as in k_linear_t2: 16-byte chunk c of row r at r * 128 + ((c ^ ((r >> 1) & 7)) << 4) (the XOR is
// applied to the DMA's source chunk), chunks 0-3 hi, 4-7 lo; a 16x16x32 fragment read is conflict-free.
//
// Tiles: 128 pixels x TN outputs (TN = 128, or 64 for cout = 64 layers, where a 128-wide tile would waste half its MFMAs), four
// waves in 2 (pixels) x 2 (outputs), wave tile 64 pixels x TN / 2 outputs.  Two LDS buffers: the DMA of stage k + 1 is issued
// before the MFMAs of stage k, one barrier per stage.  No split along K: every output element is the same sum in the same
// order whatever the batch, so an image's embedding does not depend on its batch mates.
//
// Scales are per image: x_scale[b] is the power of two the input rows were written with; a terms output is written with
//   y_scale[b] = 2^(14 - floor(log2 bound_b)),  bound_b = x_range[b] * w_abs_sum + bias_abs_max (+ res_range[b])
// (>= every |y| of image b: max_o sum |W[o, :]| * max |x| + max |bias| + max |res|), a function of ranges complete before the
// launch; the workgroup that holds image b's first pixel stores it for the consumer.  The epilogue folds max |y| of every image
// into out_range (unsigned atomic max on the float bits, mirx_device.h), which the next layer's bound starts from.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int CT_TM = 128;                 // pixels per workgroup
constexpr int CT_LINE = 128;               // bytes of one row of one stage: 32 channels x (hi | lo)
constexpr int CT_A_BYTES = CT_TM * CT_LINE;
constexpr unsigned CT_OUT = 0x80000000u;   // an offset past every descriptor of this file: the load returns zeros

template <int TN>
struct ConvTile {
    static constexpr int B_BYTES = TN * CT_LINE;
    static constexpr int STAGE = CT_A_BYTES + B_BYTES;
    static constexpr int LDS = 2 * STAGE;
    static constexpr int OI = TN / 32;     // 16-output tiles per wave
};

// the power of two a terms output of image b is written with (see the header): 0 -> 1, non-finite -> NaN
__device__ inline float ct_out_scale(float x_range, float w_abs_sum, float bias_abs_max, float res_range) {
    float s, inv;
    range_scales(x_range * w_abs_sum + bias_abs_max + res_range, s, inv);
    return s;
}

__device__ inline float ct_decode(unsigned h, unsigned l, int half) {
    const f16x2 hv = __builtin_bit_cast(f16x2, h), lv = __builtin_bit_cast(f16x2, l);
    return (float)hv[half] + (float)lv[half];
}

template <int TN, bool RES>
__global__ __launch_bounds__(256, 2) void k_conv_t2(const char *__restrict__ xt, const float *__restrict__ x_scale,
                                                    const float *__restrict__ x_range, int64_t n, int h, int w, int cin,
                                                    int ho, int wo, int ksz, int stride, int pad,
                                                    const char *__restrict__ wt, const float *__restrict__ oscale,
                                                    const float *__restrict__ bias, int cout, float w_abs_sum, float bias_abs_max,
                                                    const char *__restrict__ rt, const float *__restrict__ r_scale,
                                                    const float *__restrict__ r_range, int relu, char *__restrict__ yt,
                                                    float *__restrict__ y_scale, float *__restrict__ y,
                                                    unsigned *__restrict__ out_range, int64_t ntiles, int64_t per_xcd, int ntn) {
    typedef ConvTile<TN> T;
    extern __shared__ __attribute__((aligned(16))) char sm[];
    // workgroups are dealt to the XCDs round robin: give each XCD a contiguous run of tiles, output tiles of one pixel tile
    // next to each other (they read the same input lines through that XCD's L2)
    const int64_t tile = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (tile >= ntiles) return;
    const int64_t hwo = (int64_t)ho * wo, m_all = n * hwo;
    const int64_t m0 = (tile / ntn) * CT_TM;
    const int n0 = (int)(tile % ntn) * TN;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int wp = wave >> 1, wq = wave & 1;                  // this wave: pixels 64 wp .., outputs TN / 2 * wq ..
    const int pitch = cin * 4;                                // bytes of an input terms row
    const int kdim = ksz * ksz * cin;
    const int wpitch = kdim * 4;                              // bytes of a weight terms row
    const int ncs = cin >> 5, nk = ksz * ksz * ncs;           // stages per tap, stages in all

    // images this tile touches: [b0, b1]; the pixel descriptor spans exactly them
    const int64_t b0 = m0 / hwo;
    const int64_t m_end = m0 + CT_TM < m_all ? m0 + CT_TM : m_all;
    const int64_t b1 = (m_end - 1) / hwo;
    const int64_t img_bytes = (int64_t)h * w * pitch;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(xt + b0 * img_bytes), 0, (int)((b1 - b0 + 1) * img_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)(wt + (int64_t)n0 * wpitch), 0, TN * wpitch,
                                                                         0x00020000);

    if (yt && n0 == 0 && (int)threadIdx.x <= (int)(b1 - b0)) {      // the consumer's scale of every image that starts here
        const int64_t b = b0 + threadIdx.x;
        if (b * hwo >= m0)
            y_scale[b] = ct_out_scale(x_range[b], w_abs_sum, bias_abs_max, RES ? r_range[b] : 0.f);
    }

    // ---- DMA addressing.  Piece p = operand rows 8 p .. 8 p + 7 (1 KiB); wave w moves pieces w, w + 4, ..  Lane l: row
    // 8 p + (l >> 3), LDS slot l & 7 <- source chunk (l & 7) ^ ((row >> 1) & 7) (the same for every piece of the lane).
    const int prow = wave * 8 + (lane >> 3);
    const int pchunk = (lane & 7) ^ ((prow >> 1) & 7);
    int abase[4], aiy[4], aix[4];                             // pixel rows 32 i + prow of the tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + 32 * i + prow;
        if (m < m_all) {
            const int64_t b = m / hwo;
            const int rem = (int)(m - b * hwo);
            const int oy = rem / wo, ox = rem - (rem / wo) * wo;
            aiy[i] = oy * stride - pad;
            aix[i] = ox * stride - pad;
            abase[i] = (int)(((b - b0) * h + aiy[i]) * (int64_t)w + aix[i]) * pitch + pchunk * 16;
        } else {
            aiy[i] = -0x40000000;                             // never inside: reads zeros
            aix[i] = 0;
            abase[i] = 0;
        }
    }
    const unsigned bbase = (unsigned)(prow * wpitch + pchunk * 16);
    int dky = 0, dkx = 0, dcs = 0, dk = 0;                    // the next stage to fetch: tap (dky, dkx), channel stage dcs
    auto dma = [&](int buf) __attribute__((always_inline)) {
        char *dst = sm + buf * T::STAGE;
        const int tapoff = (dky * w + dkx) * pitch + dcs * CT_LINE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = (unsigned)(aiy[i] + dky) < (unsigned)h && (unsigned)(aix[i] + dkx) < (unsigned)w;
            const unsigned vo = in ? (unsigned)(abase[i] + tapoff) : CT_OUT;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, LDS_PTR(dst + (4 * i + wave) * 1024), 16, vo, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < TN / 32; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, LDS_PTR(dst + CT_A_BYTES + (4 * j + wave) * 1024), 16,
                                                     bbase + (unsigned)(j * 32 * wpitch + dk * CT_LINE), 0, 0, 0);
        ++dk;
        if (++dcs == ncs) {
            dcs = 0;
            if (++dkx == ksz) {
                dkx = 0;
                ++dky;
            }
        }
    };

    // ---- fragment addressing: lane -> row (lane & 15), chunk (lane >> 4) of the hi term; lo = hi ^ 64 -------------------
    const int fr = (((lane >> 4) ^ ((lane & 15) >> 1)) << 4);
    const int xh = (wp * 64 + (lane & 15)) * CT_LINE + fr;
    const int wh = CT_A_BYTES + (wq * (TN / 2) + (lane & 15)) * CT_LINE + fr;

    // accumulator register r of tile (oi, ti): output TN / 2 wq + 16 oi + 4 (lane >> 4) + r, pixel 64 wp + 16 ti + (lane & 15)
    f32x4 acc[T::OI][4];
#pragma unroll
    for (int oi = 0; oi < T::OI; ++oi)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) acc[oi][ti] = f32x4{0.f, 0.f, 0.f, 0.f};

    dma(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) dma(buf ^ 1);
        const char *s = sm + buf * T::STAGE;
        f16x8 fw[T::OI][2];
#pragma unroll
        for (int oi = 0; oi < T::OI; ++oi) {
            fw[oi][0] = *reinterpret_cast<const f16x8 *>(s + wh + oi * 16 * CT_LINE);
            fw[oi][1] = *reinterpret_cast<const f16x8 *>(s + (wh ^ 64) + oi * 16 * CT_LINE);
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
            const f16x8 xhi = *reinterpret_cast<const f16x8 *>(s + xh + ti * 16 * CT_LINE);
            const f16x8 xlo = *reinterpret_cast<const f16x8 *>(s + (xh ^ 64) + ti * 16 * CT_LINE);
#pragma unroll
            for (int oi = 0; oi < T::OI; ++oi) {
                // the stage's 32-channel partial sum starts from zero and is added once: the fp32 rounding grows with
                // 32 + stages instead of K additions (a single running sum measured 1.1e-6 of max |y| at K = 2304)
                f32x4 part = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[oi][1], xhi, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                part = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[oi][0], xlo, part, 0, 0, 0);
                part = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[oi][0], xhi, part, 0, 0, 0);
                acc[oi][ti] += part;
            }
        }
        // the next stage has landed, and every wave is done with this buffer before the DMA after next overwrites it
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // ---- epilogue ----------------------------------------------------------------------------------------------------
    const int ybytes = cout * 4;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const int64_t m = m0 + wp * 64 + ti * 16 + (lane & 15);
        const bool mok = m < m_all;
        const int64_t b = (mok ? m : m_all - 1) / hwo;
        const float inv_x = 1.f / x_scale[b];
        const float inv_r = RES ? 1.f / r_scale[b] : 0.f;
        const float ys = yt ? ct_out_scale(x_range[b], w_abs_sum, bias_abs_max, RES ? r_range[b] : 0.f) : 0.f;
        float vmax = 0.f;
#pragma unroll
        for (int oi = 0; oi < T::OI; ++oi) {
            const int o = n0 + wq * (TN / 2) + oi * 16 + 4 * (lane >> 4);
            if (!mok || o >= cout) continue;
            const f32x4 os = *reinterpret_cast<const f32x4 *>(oscale + o);
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + o);
            const int64_t lo_off = m * ybytes + (o >> 5) * CT_LINE + (o & 31) * 2;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[oi][ti][e] * (os[e] * inv_x) + bv[e];
            if (RES) {
                const u32x2 rh = *reinterpret_cast<const u32x2 *>(rt + lo_off);
                const u32x2 rl = *reinterpret_cast<const u32x2 *>(rt + lo_off + 64);
                v[0] += ct_decode(rh[0], rl[0], 0) * inv_r;
                v[1] += ct_decode(rh[0], rl[0], 1) * inv_r;
                v[2] += ct_decode(rh[1], rl[1], 0) * inv_r;
                v[3] += ct_decode(rh[1], rl[1], 1) * inv_r;
            }
            if (relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];    // keeps a NaN (fmaxf would drop it)
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) vmax = range_max(vmax, v[e]);
            if (y) *reinterpret_cast<f32x4 *>(y + m * cout + o) = v;
            if (yt) {
                unsigned h0, l0, h1, l1;
                split2h_pair(v[0] * ys, v[1] * ys, h0, l0);
                split2h_pair(v[2] * ys, v[3] * ys, h1, l1);
                *reinterpret_cast<u32x2 *>(yt + lo_off) = u32x2{h0, h1};
                *reinterpret_cast<u32x2 *>(yt + lo_off + 64) = u32x2{l0, l1};
            }
        }
        if (out_range) range_publish_lanes(out_range, (int)b, vmax, lane);
    }
}

// ---- NCHW fp32 (the stem's output) -> terms rows, image b scaled by 2^(14 - floor(log2 range[b])) ----------------------
// grid (ceil(hw / 64), n), 256 threads: lane -> pixel, wave -> every 4th group of 8 channels (16 B of hi + 16 B of lo)
__global__ __launch_bounds__(256) void k_nchw_to_terms(const float *__restrict__ x, int64_t xbs, int c, int hw,
                                                       const float *__restrict__ range, float *__restrict__ scale_row,
                                                       char *__restrict__ xt) {
    const int64_t b = blockIdx.y;
    float s, inv;
    range_scales(range[b], s, inv);
    if (blockIdx.x == 0 && threadIdx.x == 0) scale_row[b] = s;
    const int p = blockIdx.x * 64 + (threadIdx.x & 63);
    if (p >= hw) return;
    const float *xb = x + b * xbs + p;
    char *row = xt + (b * hw + p) * (int64_t)(c * 4);
    for (int g = threadIdx.x >> 6; g < (c >> 3); g += 4) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = xb[(int64_t)(8 * g + j) * hw] * s;
        u32x4 hi, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned a, d;
            split2h_pair(v[2 * j], v[2 * j + 1], a, d);
            hi[j] = a;
            lo[j] = d;
        }
        char *dst = row + (g >> 2) * CT_LINE + (g & 3) * 16;
        *reinterpret_cast<u32x4 *>(dst) = hi;
        *reinterpret_cast<u32x4 *>(dst + 64) = lo;
    }
}

// ---- head: y[b, :] = mean over the hw pixels of x[b, p, :] (fp32 rows), then optionally / max(||y||, 1e-12) -----------
__global__ __launch_bounds__(256) void k_gap_nhwc(const float *__restrict__ x, int hw, int c, int normalize,
                                                  float *__restrict__ y) {
    __shared__ float s_part[4];
    const int64_t b = blockIdx.x;
    const float *xb = x + b * hw * (int64_t)c;
    float *yb = y + b * c;
    const float rhw = 1.f / (float)hw;
    float ss = 0.f;
    for (int ch = threadIdx.x * 4; ch < c; ch += 1024) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int p = 0; p < hw; ++p) a += *reinterpret_cast<const f32x4 *>(xb + (int64_t)p * c + ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = a[e] * rhw;
            ss += a[e] * a[e];
        }
        *reinterpret_cast<f32x4 *>(yb + ch) = a;
    }
    if (!normalize) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float tot = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    const float nrm = sqrtf(tot);
    const float sc = 1.f / (nrm > 1e-12f ? nrm : 1e-12f);
    for (int ch = threadIdx.x * 4; ch < c; ch += 1024) {      // the values this thread wrote above
        f32x4 a = *reinterpret_cast<const f32x4 *>(yb + ch);
        *reinterpret_cast<f32x4 *>(yb + ch) = a * sc;
    }
}

}  // namespace

hipError_t launch_conv_t2(const void *xt, const float *x_scale, const float *x_range, int64_t n, int h, int w, int cin, int ksz,
                          int stride, const void *wt, const float *oscale, const float *bias, int cout, float w_abs_sum,
                          float bias_abs_max, const void *rt, const float *r_scale, const float *r_range, int relu, void *yt,
                          float *y_scale, float *y, float *out_range, hipStream_t st) {
    const int pad = (ksz - 1) / 2;
    const int ho = (h + 2 * pad - ksz) / stride + 1, wo = (w + 2 * pad - ksz) / stride + 1;
    const int64_t m_all = n * (int64_t)ho * wo;
    if (m_all == 0) return hipSuccess;
    // offsets inside a tile's descriptor are 32-bit: the images one tile can touch must fit in 2 GiB
    const int64_t img_bytes = (int64_t)h * w * cin * 4;
    const int64_t span = CT_TM / ((int64_t)ho * wo) + 2;
    if (span * img_bytes >= 0x7fffffffLL || (int64_t)128 * ksz * ksz * cin * 4 >= 0x7fffffffLL) return hipErrorInvalidValue;
    const bool wide = cout % 128 == 0 || cout > 64;
    const int tn = wide ? 128 : 64;
    const int ntn = (cout + tn - 1) / tn;
    const int64_t ntiles = (m_all + CT_TM - 1) / CT_TM * ntn;
    const int64_t per_xcd = (ntiles + 7) / 8;
    if (per_xcd * 8 > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(per_xcd * 8));
#define MIRX_CT2(TN, R)                                                                                                \
    {                                                                                                                  \
        static std::atomic<unsigned long long> attr_devs{0};                                                                       \
        hipError_t e = set_dynamic_lds(k_conv_t2<TN, R>, ConvTile<TN>::LDS, &attr_devs);    \
        if (e != hipSuccess) return e;                                                                             \
        hipLaunchKernelGGL((k_conv_t2<TN, R>), grid, dim3(256), ConvTile<TN>::LDS, st,                                 \
                           reinterpret_cast<const char *>(xt), x_scale, x_range, n, h, w, cin, ho, wo, ksz, stride, pad, \
                           reinterpret_cast<const char *>(wt), oscale, bias, cout, w_abs_sum, bias_abs_max,            \
                           reinterpret_cast<const char *>(rt), r_scale, r_range, relu, reinterpret_cast<char *>(yt),   \
                           y_scale, y, reinterpret_cast<unsigned *>(out_range), ntiles, per_xcd, ntn);                 \
    }
    if (wide) {
        if (rt) MIRX_CT2(128, true) else MIRX_CT2(128, false)
    } else {
        if (rt) MIRX_CT2(64, true) else MIRX_CT2(64, false)
    }
#undef MIRX_CT2
    return hipGetLastError();
}

hipError_t launch_nchw_to_terms(const float *x, int64_t xbs, int64_t n, int c, int hw, const float *range, float *scale_row,
                                void *xt, hipStream_t st) {
    if (n == 0 || hw == 0) return hipSuccess;
    hipLaunchKernelGGL(k_nchw_to_terms, dim3((unsigned)((hw + 63) / 64), (unsigned)n), dim3(256), 0, st, x, xbs, c, hw, range,
                       scale_row, reinterpret_cast<char *>(xt));
    return hipGetLastError();
}

hipError_t launch_gap_nhwc(const float *x, int64_t n, int hw, int c, int normalize, float *y, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gap_nhwc, dim3((unsigned)n), dim3(256), 0, st, x, hw, c, normalize, y);
    return hipGetLastError();
}

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

extern "C" int mirx_conv_terms(const void *xt, const float *x_scale, const float *x_range, int64_t n, int h, int w, int cin,
                               int ksize, int stride, const void *wt, const float *oscale, const float *bias, int cout,
                               float w_abs_sum, float bias_abs_max, const void *res_or_null, const float *res_scale,
                               const float *res_range, int relu, void *yt_or_null, float *y_scale_or_null, float *y_or_null,
                               float *out_range_or_null, void *stream) {
    MIRX_CHECK(n >= 0 && h >= 1 && w >= 1, "conv_terms: bad geometry");
    MIRX_CHECK(ksize == 1 || ksize == 3, "conv_terms: kernel size must be 1 or 3");
    MIRX_CHECK(stride == 1 || stride == 2, "conv_terms: stride must be 1 or 2");
    MIRX_CHECK(cin >= 32 && cin % 32 == 0 && cout >= 32 && cout % 32 == 0, "conv_terms: cin and cout must be multiples of 32");
    MIRX_CHECK(xt && x_scale && x_range && wt && oscale && bias, "conv_terms: null input");
    MIRX_CHECK(yt_or_null || y_or_null, "conv_terms: no output");
    MIRX_CHECK(!yt_or_null || y_scale_or_null, "conv_terms: a terms output needs its scale row");
    MIRX_CHECK(!res_or_null || (res_scale && res_range), "conv_terms: a residual needs its scale and range rows");
    MIRX_CHECK(((uintptr_t)oscale | (uintptr_t)bias | (uintptr_t)y_or_null) % 16 == 0 &&
                   ((uintptr_t)xt | (uintptr_t)wt | (uintptr_t)res_or_null | (uintptr_t)yt_or_null) % 16 == 0,
               "conv_terms: buffers must be 16-byte aligned");
    MIRX_HIP(launch_conv_t2(xt, x_scale, x_range, n, h, w, cin, ksize, stride, wt, oscale, bias, cout, w_abs_sum, bias_abs_max,
                            res_or_null, res_scale, res_range, relu, yt_or_null, y_scale_or_null, y_or_null, out_range_or_null,
                            reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

extern "C" int mirx_nchw_to_terms(const float *x, int64_t x_batch_stride, int64_t n, int c, int hw, const float *range_row,
                                  float *scale_row, void *xt, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && hw >= 0, "nchw_to_terms: batch must be in [0, 65535]");
    MIRX_CHECK(c >= 32 && c % 32 == 0, "nchw_to_terms: c must be a multiple of 32");
    MIRX_CHECK(x_batch_stride >= (int64_t)c * hw, "nchw_to_terms: batch stride smaller than c * hw");
    MIRX_CHECK(n == 0 || hw == 0 || (x && range_row && scale_row && xt), "nchw_to_terms: null buffer");
    MIRX_CHECK((uintptr_t)xt % 16 == 0, "nchw_to_terms: xt must be 16-byte aligned");
    MIRX_HIP(launch_nchw_to_terms(x, x_batch_stride, n, c, hw, range_row, scale_row, xt, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

extern "C" int mirx_gap_nhwc_l2norm(const float *x, int64_t n, int hw, int c, int normalize, float *y, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 0x7fffffff && hw >= 1 && c >= 4 && c % 4 == 0, "gap_nhwc: bad shape (c % 4 == 0, hw >= 1)");
    MIRX_CHECK(n == 0 || (x && y), "gap_nhwc: null buffer");
    MIRX_CHECK(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "gap_nhwc: buffers must be 16-byte aligned");
    MIRX_HIP(launch_gap_nhwc(x, n, hw, c, normalize, y, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}
