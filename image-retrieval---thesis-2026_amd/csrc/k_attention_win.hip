// k_attention_win.hip -- SwinV2's shifted-window cosine attention (timm 0.9.7 WindowAttention inside SwinTransformerV2Block,
// the backbone of the reference's SwinV2, model.py:418-446 there), straight on the qkv Linear's fp32 raster rows:
//
//   out[pixel(t)] = sum_u softmax_u( cos(q_t, k_u) * ls[head] + bias[head, rel(t, u)] + mask(t, u) ) v_u
//
// over the tokens t, u of one window of the cyclically shifted map.  Token (ty, tx) of window (wy, wx) is pixel
// ((wy ws + ty + shift) mod side, (wx ws + tx + shift) mod side): the roll, the window partition and their inverses are
// addressing only, and the result goes back to the token's own pixel.  bias = the compact per-block table [heads, (2 ws - 1)^2]
// (already 16 sigmoid(cpb_mlp(..))), rel(t, u) = (ty - uy + ws - 1) (2 ws - 1) + (tx - ux + ws - 1); mask = -100 (timm's value,
// not -inf) where the two tokens lie in different regions of timm's three slices per axis (shift > 0 only); ls[head] =
// exp(min(logit_scale, ln 100)).  q and k are L2-normalised per (token, head) in fp32 (F.normalize, eps 1e-12).
//
// Arithmetic and LDS layouts are k_attention_split<SplitF16x2, 32>'s (k_attention_split.hip: flash attention, 128 queries per workgroup, 32-key tiles double
// buffered, every operand two fp16 terms, three v_mfma_f32_32x32x16_f16 per product block, online softmax in base 2):
//   q^ is staged as q^ * ls log2(e) * 64 (<= 9 234), k^ as k^ * 2^14: |q^|, |k^| <= 1, so no bound is needed;
//   v is staged at the power of two that puts the largest |v| of THIS (image, window, head) in [2^14, 2^15) -- a pre-pass over the
//   window's V rows (read again from L2 by the tile loop), so an image's bits never depend on its batch mates and a non-finite
//   value turns only its own window's output into NaN;
//   probabilities as p * 1024.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int DH = 32;                  // head dimension (SwinV2-B: 128 / 4, 256 / 8, 512 / 16, 1024 / 32)
constexpr int KT = 32;                  // keys per tile
constexpr int KCH = 4, KROW = 64;       // K row: 4 chunks of 8 channels (16 B per term)
constexpr int KPL = KT * KROW;          // one term of the K tile: 2 KiB
constexpr int VPL = DH * 64;            // one term of the V^T tile: 2 KiB
constexpr int TBUF = 2 * (KPL + VPL);   // 8 KiB per buffer
constexpr float LOG2E = 1.4426950408889634f;
constexpr float Q_STAGE = 64.f, K_STAGE = 16384.f;
constexpr float MASK_L2 = -100.f * LOG2E;

// region of timm's shifted-window mask along one axis: slices [0, side - ws), [side - ws, side - shift), [side - shift, side)
__device__ inline int region1(int y, int side, int ws, int shift) { return y < side - ws ? 0 : (y < side - shift ? 1 : 2); }

// grid: one workgroup per (query tile of 128, window, head, image), 1-D.  XCD-aware order as k_attention_split: the query tiles of
// one (window, head, image) -- which stream the same K and V -- are dealt to the same XCD.
template <int WS>
__global__ __launch_bounds__(256, 2) void k_attention_win(const float *__restrict__ qkv, int side, int shift, int heads,
                                                          const float *__restrict__ bias_tab, const float *__restrict__ lscale,
                                                          float *__restrict__ out, char *__restrict__ out_t, float t_scale) {
    constexpr int N = WS * WS, QTW = (N + 127) / 128, TD = 2 * WS - 1;
    __shared__ __attribute__((aligned(16))) char sm[2 * TBUF];
    __shared__ float sbias[TD * TD];                     // this head's table * log2(e)
    __shared__ unsigned red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int half = lane >> 5, nq = lane & 31;
    const int nwx = side / WS, nw = nwx * nwx;

    // ---- which (query tile, window, head, image) ----------------------------------------------------------------------
    const unsigned lin = blockIdx.x;
    const unsigned npair = gridDim.x / QTW, full = npair & ~7u;
    unsigned qt = lin % QTW, pair = lin / QTW;
    if (lin < QTW * full) {
        const unsigned j = lin >> 3;
        pair = (j / QTW) * 8 + (lin & 7);
        qt = j % QTW;
    }
    const int win = (int)(pair % nw), head = (int)((pair / nw) % heads);
    const int64_t img = pair / ((unsigned)nw * heads);
    const int wy = win / nwx, wx = win - wy * nwx;
    const int c = heads * DH;
    const int64_t tok = 3 * (int64_t)c;                  // floats per pixel row of qkv
    const float *base = qkv + img * side * side * tok;
    auto pix = [&](int t) -> int {                       // window token t -> pixel of the unshifted map
        const int ty = t / WS, tx = t - ty * WS;
        int py = wy * WS + ty + shift, px = wx * WS + tx + shift;
        if (py >= side) py -= side;
        if (px >= side) px -= side;
        return py * side + px;
    };

    // ---- the head's bias table, and the largest |v| of the window (NaN sorts above everything) -------------------------
    for (int i = threadIdx.x; i < TD * TD; i += 256) sbias[i] = bias_tab[(int64_t)head * TD * TD + i] * LOG2E;
    {
        float vm = 0.f;
        for (int it = threadIdx.x; it < N * 8; it += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(base + (int64_t)pix(it >> 3) * tok + 2 * c + head * DH + 4 * (it & 7));
            vm = range_max(range_max(range_max(range_max(vm, v[0]), v[1]), v[2]), v[3]);
        }
        unsigned a = __float_as_uint(vm);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)a, off, 64);
            a = o > a ? o : a;
        }
        if (lane == 0) red[wave] = a;
    }
    __syncthreads();
    float v_mul, v_inv;
    {
        unsigned a = red[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) a = red[w] > a ? red[w] : a;
        range_scales(__uint_as_float(a), v_mul, v_inv);
    }

    // ---- this lane's query: channels 16 ks + 8 half + i, normalised, times ls log2(e) 64 -------------------------------
    const int q_idx = qt * 128 + wave * 32 + nq;
    const bool q_live = q_idx < N;
    const int q_t = q_live ? q_idx : N - 1;
    const int q_pix = pix(q_t);
    const int qy = q_t / WS, qx = q_t - (q_t / WS) * WS;
    const int q_reg = shift ? 3 * region1(wy * WS + qy, side, WS, shift) + region1(wx * WS + qx, side, WS, shift) : 0;
    f16x8 qh[2], ql[2];
    {
        const float *qp = base + (int64_t)q_pix * tok + head * DH + 8 * half;
        float v[2][8];
        float ss = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(qp + 16 * ks), b = *reinterpret_cast<const f32x4 *>(qp + 16 * ks + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[ks][j] = a[j]; v[ks][4 + j] = b[j]; }
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(v[ks][j], v[ks][j], ss);
        }
        ss += __shfl_xor(ss, 32, 64);                     // the other 16 channels of the same query
        const float qm = lscale[head] * LOG2E * Q_STAGE / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[ks][j] *= qm;
            split2h_x8(v[ks], qh[ks], ql[ks]);
        }
    }

    // ---- staging: waves 0-1 carry K items (key it >> 2, channels 8 (it & 3) .. + 7), waves 2-3 V items (keys 2 (it >> 3),
    // + 1, channels 4 (it & 7) .. + 3).  Keys beyond N read key N - 1 (finite; their scores are -inf, probabilities 0).
    const bool is_k = threadIdx.x < 128;
    const int it = threadIdx.x & 127;
    f32x4 r[2];
    auto load_tile = [&](int kt) {
        if (is_k) {
            int key = kt * KT + (it >> 2);
            key = key < N ? key : N - 1;
            const float *p = base + (int64_t)pix(key) * tok + c + head * DH + 8 * (it & 3);
            r[0] = *reinterpret_cast<const f32x4 *>(p);
            r[1] = *reinterpret_cast<const f32x4 *>(p + 4);
        } else {
            int k0 = kt * KT + 2 * (it >> 3), k1 = k0 + 1;
            k0 = k0 < N ? k0 : N - 1;
            k1 = k1 < N ? k1 : N - 1;
            const int off = 2 * c + head * DH + 4 * (it & 7);
            r[0] = *reinterpret_cast<const f32x4 *>(base + (int64_t)pix(k0) * tok + off);
            r[1] = *reinterpret_cast<const f32x4 *>(base + (int64_t)pix(k1) * tok + off);
        }
    };
    auto store_tile = [&](int buf) {
        char *sb = sm + buf * TBUF;
        if (is_k) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) ss = fmaf(r[1][j], r[1][j], fmaf(r[0][j], r[0][j], ss));
            ss += __shfl_xor(ss, 1, 64);
            ss += __shfl_xor(ss, 2, 64);                  // the four lanes of one key
            const float km = K_STAGE / fmaxf(sqrtf(ss), 1e-12f);
            u32x4 ph, pl;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                unsigned th, tl;
                split2h_pair(r[p >> 1][2 * (p & 1)] * km, r[p >> 1][2 * (p & 1) + 1] * km, th, tl);
                ph[p] = th; pl[p] = tl;
            }
            const int key = it >> 2, ch = it & 3;
            char *d = sb + key * KROW + ((ch + (key >> 2)) % KCH) * 16;
            *reinterpret_cast<u32x4 *>(d) = ph;
            *reinterpret_cast<u32x4 *>(d + KPL) = pl;
        } else {
            const int vkey = 2 * (it >> 3), vc = it & 7;
            const int vpos = 16 * (vkey >> 4) + 8 * ((vkey >> 2) & 1) + (vkey & 3) + 4 * ((vkey >> 3) & 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned th, tl;
                split2h_pair(r[0][j] * v_mul, r[1][j] * v_mul, th, tl);
                const int d = 4 * vc + j;
                char *dst = sb + 2 * KPL + d * 64 + (((vpos >> 3) ^ ((d >> 2) & 3)) << 4) + (vpos & 7) * 2;
                *reinterpret_cast<unsigned *>(dst) = th;
                *reinterpret_cast<unsigned *>(dst + VPL) = tl;
            }
        }
    };

    int fk[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) fk[ks] = nq * KROW + ((2 * ks + half + (nq >> 2)) % KCH) * 16;
    int fv[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) fv[s] = 2 * KPL + nq * 64 + (((2 * s + half) ^ ((nq >> 2) & 3)) << 4);

    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    const float s_inv = 1.0f / (Q_STAGE * K_STAGE);

    constexpr int NTILES = (N + KT - 1) / KT;
    load_tile(0);
    store_tile(0);
    for (int kt = 0; kt < NTILES; ++kt) {
        const int cur = kt & 1;
        __syncthreads();                                  // tile kt visible; buffer cur ^ 1 free
        load_tile(kt + 1 < NTILES ? kt + 1 : kt);
        __builtin_amdgcn_sched_barrier(0);
        const char *sb = sm + cur * TBUF;

        // ---- S^T = K^ Q^T ----------------------------------------------------------------------------------------------
        f32x16 sacc;
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const f16x8 ah = *reinterpret_cast<const f16x8 *>(sb + fk[ks]);
            const f16x8 al = *reinterpret_cast<const f16x8 *>(sb + fk[ks] + KPL);
            MIRX_MFMA3(sacc, ah, al, qh[ks], ql[ks])
        }

        // ---- logits in base 2: score + bias + mask; register i holds key kt KT + 8 (i >> 2) + 4 half + (i & 3) ------------
        const int key0 = kt * KT + 4 * half;
        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + 8 * (i >> 2) + (i & 3);
            if (key < N) {
                const int ky = key / WS, kx = key - (key / WS) * WS;
                float b = sbias[(qy - ky + WS - 1) * TD + (qx - kx + WS - 1)];
                if (shift) {
                    const int kr = 3 * region1(wy * WS + ky, side, WS, shift) + region1(wx * WS + kx, side, WS, shift);
                    b += kr != q_reg ? MASK_L2 : 0.f;
                }
                sacc[i] = fmaf(sacc[i], s_inv, b);
            } else {
                sacc[i] = -INFINITY;
            }
            mt = fmaxf(mt, sacc[i]);
        }
        mt = max_over_halves(mt);                          // the other 16 keys of the same query
        const float m_new = fmaxf(m_run, mt);              // finite: every tile holds at least one key of the window
        const float alpha = exp2_raw(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sacc[i] = exp2_raw(sacc[i] - m_new);
            psum += sacc[i];
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] *= alpha;
        }

        // ---- O^T += V^T P^T --------------------------------------------------------------------------------------------
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = sacc[8 * s + j] * 1024.f;
            f16x8 bh, bl;
            split2h_x8(pv, bh, bl);
            const f16x8 ah = *reinterpret_cast<const f16x8 *>(sb + fv[s]);
            const f16x8 al = *reinterpret_cast<const f16x8 *>(sb + fv[s] + VPL);
            MIRX_MFMA3(o, ah, al, bh, bl)
        }
        store_tile(cur ^ 1);
    }

    // ---- normalise and store at the token's own pixel: register i is channel 8 (i >> 2) + 4 half + (i & 3) ---------------
    l_run += __shfl_xor(l_run, 32, 64);
    if (q_live) {
        const float inv = v_inv * (1.0f / 1024.0f) / l_run;
        const int64_t row = img * side * side + q_pix;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = o[4 * g + j] * inv;
            const int ch = head * DH + 8 * g + 4 * half;
            if (out) *reinterpret_cast<f32x4 *>(out + row * c + ch) = v;
            if (out_t) store_terms4(out_t, row, c, ch, v, t_scale);
        }
    }
}

template <int WS>
hipError_t launch_win(const float *qkv, int64_t n, int side, int shift, int heads, const float *bias_tab, const float *lscale,
                      float *out, char *out_t, float t_scale, hipStream_t st) {
    constexpr int QTW = (WS * WS + 127) / 128;
    const int64_t nw = (int64_t)(side / WS) * (side / WS);
    const int64_t blocks = (int64_t)QTW * nw * heads * n;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_attention_win<WS>, dim3((unsigned)blocks), dim3(256), 0, st, qkv, side, shift, heads, bias_tab, lscale,
                       out, out_t, t_scale);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_attention_win(const float *qkv, int64_t n, int side, int window, int shift, int heads, const float *bias_tab,
                                const float *lscale, float *out, void *out_t, float t_scale, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (heads < 1 || side < window || side % window || shift < 0 || shift >= window) return hipErrorInvalidValue;
    if (window == 24)
        return launch_win<24>(qkv, n, side, shift, heads, bias_tab, lscale, out, reinterpret_cast<char *>(out_t), t_scale, st);
    if (window == 12)
        return launch_win<12>(qkv, n, side, shift, heads, bias_tab, lscale, out, reinterpret_cast<char *>(out_t), t_scale, st);
    return hipErrorInvalidValue;
}

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

extern "C" int mirx_window_attention_split2h(const float *qkv, int64_t n, int side, int window, int shift, int heads,
                                             int head_dim, const float *bias_table, const float *logit_scale, float *out_or_null,
                                             void *out_terms_or_null, float out_scale, void *stream) {
    MIRX_CHECK(n >= 0 && heads >= 1 && head_dim == 32, "window_attention: head_dim must be 32");
    MIRX_CHECK(window == 12 || window == 24, "window_attention: window must be 12 or 24");
    MIRX_CHECK(side >= window && side % window == 0, "window_attention: side must be a multiple of the window");
    MIRX_CHECK(shift >= 0 && shift < window, "window_attention: shift must be in [0, window)");
    MIRX_CHECK(out_or_null || out_terms_or_null, "window_attention: no output");
    MIRX_CHECK(!out_terms_or_null || out_scale > 0.f, "window_attention: out_scale must be positive");
    MIRX_CHECK(n == 0 || (qkv && bias_table && logit_scale), "window_attention: null input");
    MIRX_CHECK(((uintptr_t)qkv | (uintptr_t)out_or_null | (uintptr_t)out_terms_or_null) % 16 == 0,
               "window_attention: buffers must be 16-byte aligned");
    MIRX_HIP(launch_attention_win(qkv, n, side, window, shift, heads, bias_table, logit_scale, out_or_null, out_terms_or_null,
                                  out_scale, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}
