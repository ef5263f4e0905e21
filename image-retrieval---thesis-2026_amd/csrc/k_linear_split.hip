// k_linear_split.hip -- fp32-grade Linear layer  y = epi(x W^T + b)  for the token-major models (DINOv2 / MedSigLIP blocks,
// ConvNeXtV2 point-wise MLPs): fp32 in, fp32 out, every fp32 operand carried as a few 16-bit terms on the matrix pipe.  ONE kernel
// template over a term scheme S (mirx_device.h), two schemes:
//
//   SplitBf16x3 (launch_linear_s3): THREE bf16 terms, 6 v_mfma_f32_32x32x16_bf16 per product block; the dropped cross terms are
//       <= 3 * 2^-24 |w x|, the rounding class of one fp32 product.  bf16 has fp32's exponent: no range information needed.
//   SplitF16x2 (launch_linear_h2): TWO fp16 terms (x = xh + xl exactly to 22 bits), 3 v_mfma_f32_32x32x16_f16 per product block
//       (the dropped xl wl is 2^-22 of the product): half the matrix work and 4 instead of 6 LDS bytes per element at the same
//       measured error (both are dominated by the fp32 accumulation).  301-330 TFLOP/s fp32-equivalent on the DINOv2 shapes vs
//       171-199 for the bf16 scheme (the chip holds 1.7 instead of 1.36 GHz under it).
//       fp16 has 5 exponent bits, so the CALLER supplies range information: the weights arrive multiplied by a power of two
//       (mirx.model._linear_h2_weights: largest |w| in [2^13, 2^14)), x is multiplied by the power of two `x_scale` while it is
//       staged, and the accumulator by `out_scale` = 1 / (x_scale * w_scale) before bias / activation -- all exact.
//       Contract: |x * x_scale| <= 65504 for every element (mirx.model uses it where a bound is provable: the inputs that come
//       out of a LayerNorm).  Every range step is compiled for this scheme only (S::SCALED).
//
//   x   [m][k] fp32, k contiguous (tokens x features)        -> MFMA row operand, split while it is staged
//   w   [ceil(n / 128)][k / 16][S::T terms][128][16] 16-bit, rows >= n zero -> MFMA column operand
//       (mirx.model._split3_weights / _linear_h2_weights)
//   y   [m][n] fp32:  v = acc + bias[n];  ACT == 1: v = gelu(v) (erf form), ACT == 2: tanh form;
//                     RES: v = res[m][n] + gamma[n] * v  (LayerScale + residual; y may alias res)
//   NCHW variant (ConvNeXt block tail): token t = image t / tpi, pixel t % tpi; y and res are [image][n][tpi].
//   The MFMA operand roles are swapped (rows = outputs, lanes = tokens) so that a half-wave still stores 128
//   contiguous bytes.
//
// Workgroup tile 128 tokens x 128 outputs, 4 waves (2 x 2, 64 x 64 each), 16 features per stage, double-buffered LDS
// (2 * 2 T * 4 KiB: 48 KiB for three terms, 32 KiB for two; 3 workgroups per CU).  The weights go global -> LDS by DMA (no
// registers); the activations are register-prefetched one stage ahead, two stages per load group so that each 128-byte line of
// a token row is fetched while it is still in the vector L1.  The output tile index runs with n fastest and is laid out per XCD
// (workgroup id % 8 = XCD on gfx950), so the n-tiles that share a token tile are resident on the SAME L2 at the same time: x is
// read from HBM once per token tile.
//
// Measured and not kept: two token tiles per workgroup against one staged copy of the weights -- the change that gave the
// DenseNet 1x1 conv 6 % -- was built on the fp16 scheme and measured 7-10 % SLOWER on all three token-major backbones: 212 VGPRs,
// two workgroups per CU instead of three, and this kernel lives on the matrix pipe, not on the bytes it pulls in.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {
// A stage is published by a barrier only after THIS wave's LDS DMA has landed: the compiler's own s_waitcnt
// before s_barrier covers the registers it knows about, not the asynchronous buffer_load ... lds writes.
#define STAGE_BARRIER()                                      \
    do {                                                     \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     \
        __syncthreads();                                     \
    } while (0)

// Diagnostic builds of the fp16 scheme (results wrong; attribute the kernel's time): -DMIRX_LH2_EXP=1 no fp16 split (raw bits
// staged), 2 no x loads inside the K loop, 3 plain-store epilogue (no activation / residual), 4 no MFMAs
#ifndef MIRX_LH2_EXP
#define MIRX_LH2_EXP 0
#endif

constexpr int TM = 128;            // tokens per workgroup
constexpr int TN = 128;            // outputs per workgroup
constexpr int KC = 16;             // features per stage
constexpr int PLANE = 128 * KC * 2;            // bytes of one term of one operand stage (4 KiB)

// SQ (fp16 scheme, row-major outputs only): the workgroup also returns the column sums of v^2 over its token rows, split by image
// (a tile of 128 rows spans at most two images when tokens_per_image >= 128): sq_out[tile_m][0 / 1][n] -- the partial sums of
// ConvNeXtV2's global response norm ||hid[b, :, c]||_2, so that no separate pass has to read the 4C-wide hidden map again.
// Fixed summation order (registers by row, the two lane halves, the two wave rows): bit-reproducible.
template <class S, int ACT, bool RES, bool NCHW, bool GRN, bool SQ = false>
__global__ __launch_bounds__(256, 3) void k_linear_split(const float *__restrict__ x, int64_t m, int k,
                                                         const uint16_t *__restrict__ w,
                                                         const float *__restrict__ bias, int n, const float *res,
                                                         const float *__restrict__ gamma, float *y, int ntn,
                                                         int64_t total_tiles, int64_t per_xcd, int tpi, float x_scale,
                                                         float out_scale, const float *__restrict__ xb_dev,
                                                         float *__restrict__ sq_out) {
    constexpr int T = S::T;                        // terms per operand
    constexpr int STAGE = 2 * T * PLANE;           // x terms [0, T), w terms [T, 2 T): 24 / 16 KiB
    constexpr int W_STAGE = T * TN * KC * 2;       // bytes of one stage of the weight image: T KiB per wave, in 1-KiB pieces
    constexpr int EXP = S::SCALED ? MIRX_LH2_EXP : 0;
    typedef typename S::frag frag;
    extern __shared__ __attribute__((aligned(16))) char sm[];
    // xb_dev: the input's bound lives (partly) on the device -- |x * gamma| <= x_scale * xb_dev[0] with `x_scale` the host's
    // bound on |x| and xb_dev[0] the largest |gamma| (ConvNeXt GRN scale, computed per forward); the kernel derives the
    // power-of-two scales itself and `out_scale` arrives as 1 / w_scale.  A non-finite bound turns every output into NaN.
    if (S::SCALED && xb_dev) {
        float xs, xi;
        range_scales(x_scale * xb_dev[0], xs, xi);
        x_scale = xs;
        out_scale *= xi;
    }
    const int64_t tile = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (tile >= total_tiles) return;
    const int tn = (int)(tile % ntn);
    const int64_t m0 = (tile / ntn) * TM;
    const int n0 = tn * TN;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int nk = k / KC;

    // ---- staging: x: thread -> token row (t >> 1), 8 features at 8 (t & 1), one 16-byte chunk per term ----------
    const int x_row = threadIdx.x >> 1, x_half = threadIdx.x & 1;
    int64_t xr = m0 + x_row;
    if (xr >= m) xr = m - 1;                                   // ragged last tile: read a valid row, never stored
    const float *xsrc = x + xr * k + 8 * x_half;
    const int x_lds = x_row * 32 + ((x_half ^ ((x_row >> 3) & 1)) << 4);               // + term * PLANE
    // w: the stage image (T planes of 4 KiB) goes global -> LDS by DMA (buffer_load ... lds: lane l of a wave writes 16 B at
    // piece base + 16 l), T 1-KiB pieces per wave.  Piece p, lane l is LDS (term p / 4, row 32 (p & 3) + l / 2, slot l & 1),
    // which holds source chunk (l & 1) ^ ((row >> 3) & 1) -- the same for every piece.
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(w + ((int64_t)tn * nk) * (T * TN * KC)), 0, nk * W_STAGE, 0x00020000);
    const int w_voff = (lane >> 1) * 32 + (((lane & 1) ^ ((lane >> 4) & 1)) << 4);

    f32x4 rx[2], rx2[2];
    // GRN (ConvNeXt block tail): x is multiplied by the per-(image, feature) scale `gamma` = [m / tpi][k] while it is
    // staged -- the GRN apply pass over the 4C-wide hidden map disappears (its shift is folded into the bias by the
    // caller: W (x s + b) = W (x s) + W b)
    f32x4 sx[2], sx2[2];
    const float *gsp = GRN ? gamma + (xr / tpi) * k + 8 * x_half : nullptr;
    auto dma_w = [&](int kt, int buf) {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const int piece = wave + 4 * i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrsrc, LDS_PTR(sm + buf * STAGE + T * PLANE + piece * 1024), 16,
                                                     w_voff, kt * W_STAGE + piece * 1024, 0, 0);
        }
    };
    auto load_x = [&](int kt, f32x4 (&r)[2], f32x4 (&sc)[2]) {
        if (EXP == 2 && kt > 1) return;
        r[0] = *reinterpret_cast<const f32x4 *>(xsrc + kt * KC);
        r[1] = *reinterpret_cast<const f32x4 *>(xsrc + kt * KC + 4);
        if (GRN) {
            sc[0] = *reinterpret_cast<const f32x4 *>(gsp + kt * KC);
            sc[1] = *reinterpret_cast<const f32x4 *>(gsp + kt * KC + 4);
        }
    };
    auto store_x = [&](int buf, const f32x4 (&r)[2], const f32x4 (&sc)[2]) {
        char *sb = sm + buf * STAGE;
        u32x4 p[T];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x2 v = {r[j >> 1][2 * (j & 1)], r[j >> 1][2 * (j & 1) + 1]};
            if (GRN) {
                v[0] *= sc[j >> 1][2 * (j & 1)];
                v[1] *= sc[j >> 1][2 * (j & 1) + 1];
            }
            unsigned t[T];
            if (EXP == 1) {
                t[0] = __float_as_uint(v[0]);
                t[1] = __float_as_uint(v[1]);
            } else {
                S::split_pair(v[0], v[1], x_scale, t);
            }
#pragma unroll
            for (int q = 0; q < T; ++q) p[q][j] = t[q];
        }
#pragma unroll
        for (int q = 0; q < T; ++q) *reinterpret_cast<u32x4 *>(sb + x_lds + q * PLANE) = p[q];
    };

    // ---- fragment addressing: lane -> row (lane & 31), K chunk (lane >> 5) -------------------------------
    const int kg = lane >> 5;
    int fx[2], fw[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int rx_ = wm * 64 + t * 32 + (lane & 31);
        fx[t] = rx_ * 32 + ((kg ^ ((rx_ >> 3) & 1)) << 4);
        const int rw_ = wn * 64 + t * 32 + (lane & 31);
        fw[t] = T * PLANE + rw_ * 32 + ((kg ^ ((rw_ >> 3) & 1)) << 4);
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    auto mfma_stage = [&](int cur) {
        const char *sb = sm + cur * STAGE;
        frag a[2][T], b[2][T];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < T; ++p) {
                a[t][p] = *reinterpret_cast<const frag *>(sb + fx[t] + p * PLANE);
                b[t][p] = *reinterpret_cast<const frag *>(sb + fw[t] + p * PLANE);
            }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                if (EXP == 4) {
                    acc[mi][ni][0] += (float)a[mi][0][0] + (float)a[mi][1][1] + (float)b[ni][0][2] + (float)b[ni][1][3];
                    continue;
                }
                // the scheme's term order; NCHW: outputs on the MFMA rows, tokens on the lanes (operand SLOTS swapped)
                S::template product<NCHW>(acc[mi][ni], a[mi], b[ni]);
            }
    };

    // Stages go in pairs: the x loads of an even and the following odd stage touch the SAME 128-byte lines
    // (16 features = 64 B per token row per stage), so both are issued together while the line is in the
    // vector L1; issued a stage apart, the second half comes from L2 again.
    dma_w(0, 0);
    load_x(0, rx, sx);
    load_x(nk > 1 ? 1 : 0, rx2, sx2);
    store_x(0, rx, sx);
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        // ---- even stage kt in buffer 0; registers: rx2 = x of stage kt + 1 -------------------------------
        STAGE_BARRIER();
        dma_w(kt + 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_stage(0);
        store_x(1, rx2, sx2);
        // ---- odd stage kt + 1 in buffer 1; loads the x of BOTH stages of the next pair -------------------
        STAGE_BARRIER();
        const int k2 = kt + 2 < nk ? kt + 2 : nk - 1, k3 = kt + 3 < nk ? kt + 3 : nk - 1;   // branch-free tail
        dma_w(k2, 0);
        load_x(k2, rx, sx);
        load_x(k3, rx2, sx2);
        __builtin_amdgcn_sched_barrier(0);
        mfma_stage(1);
        store_x(0, rx, sx);
    }
    if (kt < nk) {                                         // odd stage count: the last stage sits in buffer 0
        STAGE_BARRIER();
        mfma_stage(0);
    }

    auto unscaled = [&](float a) { return S::SCALED ? a * out_scale : a; };     // the accumulator in x W^T's own units
    if (NCHW) {
        // register r of tile (mi, ni) = output n0 + 64 wn + 32 ni + (r&3) + 8 (r>>2) + 4 (lane>>5), token
        // m0 + 64 wm + 32 mi + (lane & 31): a half-wave stores 32 consecutive pixels of one output plane
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const int64_t tok = m0 + wm * 64 + 32 * mi + (lane & 31);
            if (tok >= m) continue;
            const int64_t img = tok / tpi;
            const int64_t base = img * n * tpi + (tok - img * tpi);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int col = n0 + wn * 64 + ni * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (col >= n) continue;                     // zero-padded weight rows of the last output tile
                    float v = unscaled(acc[mi][ni][r]) + (bias ? bias[col] : 0.f);
                    if (ACT == 1) v = gelu_erf(v);
                    if (ACT == 2) v = gelu_tanh(v);
                    const int64_t idx = base + (int64_t)col * tpi;
                    if (RES) v = res[idx] + v;
                    y[idx] = v;
                }
        }
        return;
    }
    // epilogue: register r of tile (mi, ni) = token m0 + 64 wm + 32 mi + (r&3) + 8 (r>>2) + 4 (lane>>5),
    // output n0 + 64 wn + 32 ni + (lane & 31): a half-wave stores 128 contiguous bytes of one token row
    float sq[2][2] = {{0.f, 0.f}, {0.f, 0.f}};                                  // SQ: [ni][first / second image of the tile]
    const int64_t second = SQ ? (m0 / tpi + 1) * (int64_t)tpi : 0;              // first row of the tile's second image
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = n0 + wn * 64 + 32 * ni + (lane & 31);
        if (col >= n) continue;                                 // zero-padded weight rows of the last output tile
        const float bv = bias ? bias[col] : 0.f;
        const float gv = (RES && gamma && !GRN) ? gamma[col] : 1.f;       // (GRN: `gamma` is the input scale, not a LayerScale)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row >= m) continue;
                float v = unscaled(acc[mi][ni][r]) + bv;
                if (EXP != 3) {
                    if (ACT == 1) v = gelu_erf(v);
                    if (ACT == 2) v = gelu_tanh(v);
                    if (RES) v = res[row * n + col] + gv * v;
                }
                y[row * n + col] = v;
                if (SQ) {
                    if (row < second) sq[ni][0] = fmaf(v, v, sq[ni][0]);
                    else sq[ni][1] = fmaf(v, v, sq[ni][1]);
                }
            }
    }
    if (SQ) {
        __syncthreads();                                        // every wave is done with the stage buffers
        float *ssq = reinterpret_cast<float *>(sm);             // [wave row wm][image 0 / 1][128 columns]
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int im = 0; im < 2; ++im) {
                const float tot = sq[ni][im] + __shfl_xor(sq[ni][im], 32, 64);
                if (lane < 32) ssq[(wm * 2 + im) * TN + wn * 64 + ni * 32 + lane] = tot;
            }
        __syncthreads();
        const int im = threadIdx.x >> 7, cl = threadIdx.x & 127;
        if (n0 + cl < n) sq_out[((m0 / TM) * 2 + im) * (int64_t)n + n0 + cl] = ssq[im * TN + cl] + ssq[(2 + im) * TN + cl];
    }
}

// gx[img][col] = sqrt( sum over the 128-row tiles that touch image img of its partial ): k_linear_split<.., SQ>'s sq_out summed in
// tile order (deterministic).  thread -> (image, column).
__global__ __launch_bounds__(256) void k_grn_norm_partials(const float *__restrict__ part, int tpi, int64_t n_img, int c,
                                                           float *__restrict__ gx) {
    const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= n_img * c) return;
    const int64_t img = it / c;
    const int col = (int)(it - img * c);
    const int64_t t0 = img * tpi / TM, t1 = ((img + 1) * tpi - 1) / TM;
    float acc = 0.f;
    for (int64_t t = t0; t <= t1; ++t) {
        const int sel = (t * TM) / tpi == img ? 0 : 1;
        acc += part[(t * 2 + sel) * (int64_t)c + col];
    }
    gx[it] = sqrtf(acc);
}

// One launch: grid, stream and the kernel's arguments in its order.
struct LinearLaunch {
    dim3 grid;
    hipStream_t st;
    const float *x;
    int64_t m;
    int k;
    const uint16_t *w;
    const float *bias;
    int n;
    const float *res, *gamma;
    float *y;
    int ntn;
    int64_t total_tiles, per_xcd;
    int tpi;
    float x_scale, out_scale;
    const float *xb_dev;
    float *sq_out;
};

// One arm = one kernel instantiation; its dynamic-LDS limit is raised on the arm's first launch on each device.
template <class S, int ACT, bool RES, bool NCHW, bool GRN, bool SQ = false>
hipError_t launch_arm(const LinearLaunch &a) {
    static std::atomic<unsigned long long> attr_devs{0};
    constexpr size_t lds = 2 * (size_t)(2 * S::T * PLANE);
    const hipError_t e = set_dynamic_lds(k_linear_split<S, ACT, RES, NCHW, GRN, SQ>, lds, &attr_devs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_linear_split<S, ACT, RES, NCHW, GRN, SQ>), a.grid, dim3(256), lds, a.st, a.x, a.m, a.k, a.w, a.bias, a.n,
                       a.res, a.gamma, a.y, a.ntn, a.total_tiles, a.per_xcd, a.tpi, a.x_scale, a.out_scale, a.xb_dev, a.sq_out);
    return hipGetLastError();
}

// The tile geometry of a launch; false: an argument no arm takes.
bool linear_launch(LinearLaunch &a, int act) {
    if (a.k % KC || a.n < 1 || act < 0 || act > 2) return false;
    a.ntn = (a.n + TN - 1) / TN;                       // w holds ntn * 128 rows, zero beyond n
    a.total_tiles = ((a.m + TM - 1) / TM) * a.ntn;
    a.per_xcd = (a.total_tiles + 7) / 8;
    if (a.per_xcd * 8 > 0x7fffffff) return false;
    a.grid = dim3((unsigned)(a.per_xcd * 8));
    return true;
}

// The arms both schemes have.  tpi > 0: ConvNeXt block tail / downsample, NCHW output, `gamma` = GRN input scale [images][k] or null.
template <class S>
hipError_t launch_common_arm(const LinearLaunch &a, int act) {
    if (a.tpi > 0) {
        if (act) return hipErrorInvalidValue;
        if (a.gamma) return a.res ? launch_arm<S, 0, true, true, true>(a) : launch_arm<S, 0, false, true, true>(a);
        return a.res ? launch_arm<S, 0, true, true, false>(a) : launch_arm<S, 0, false, true, false>(a);
    }
    if (a.xb_dev) return hipErrorInvalidValue;
    if (a.res) {
        if (act == 2) return hipErrorInvalidValue;
        return act ? launch_arm<S, 1, true, false, false>(a) : launch_arm<S, 0, true, false, false>(a);
    }
    return act == 2 ? launch_arm<S, 2, false, false, false>(a)
                    : act ? launch_arm<S, 1, false, false, false>(a) : launch_arm<S, 0, false, false, false>(a);
}

}  // namespace

hipError_t launch_grn_norm_partials(const float *part, int tpi, int64_t n_img, int c, float *gx, hipStream_t st) {
    if (n_img <= 0) return hipSuccess;
    if (tpi < TM || c < 1) return hipErrorInvalidValue;
    const int64_t blocks = (n_img * c + 255) / 256;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_grn_norm_partials, dim3((unsigned)blocks), dim3(256), 0, st, part, tpi, n_img, c, gx);
    return hipGetLastError();
}

hipError_t launch_linear_s3(const float *x, int64_t m, int k, const uint16_t *w3, const float *bias, int n, int act,
                            const float *res, const float *gamma, float *y, int tokens_per_image, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    LinearLaunch a{dim3(), st, x, m, k, w3, bias, n, res, gamma, y, 0, 0, 0, tokens_per_image, 1.f, 1.f, nullptr, nullptr};
    if (tokens_per_image < 0 || !linear_launch(a, act)) return hipErrorInvalidValue;
    return launch_common_arm<SplitBf16x3>(a, act);
}

hipError_t launch_linear_h2(const float *x, int64_t m, int k, const uint16_t *w2, const float *bias, int n, int act,
                            const float *res, const float *gamma, float x_scale, float out_scale, float *y,
                            int tokens_per_image, const float *xb_dev, hipStream_t st, bool rows_out, float *sq_out) {
    if (m <= 0) return hipSuccess;
    LinearLaunch a{dim3(), st, x, m, k, w2, bias, n, res, gamma, y, 0, 0, 0, tokens_per_image, x_scale, out_scale, xb_dev, sq_out};
    if (!linear_launch(a, act)) return hipErrorInvalidValue;
    if (sq_out) {                                     // ConvNeXt fc1 + GELU with the GRN partial sums (row-major)
        if (act != 1 || res || gamma || xb_dev || tokens_per_image < TM) return hipErrorInvalidValue;
        return launch_arm<SplitF16x2, 1, false, false, false, true>(a);
    }
    if (tokens_per_image > 0 && rows_out) {           // ConvNeXt block tail on a channels-last stream: GRN input scale, row-major output
        if (act || !gamma) return hipErrorInvalidValue;
        return res ? launch_arm<SplitF16x2, 0, true, false, true>(a) : launch_arm<SplitF16x2, 0, false, false, true>(a);
    }
    return launch_common_arm<SplitF16x2>(a, act);
}

}  // namespace mirx
