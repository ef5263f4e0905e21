// k_attention_split.hip -- the flash attention of k_attention.hip (fp32 in, fp32 out, scores never in HBM) with BOTH GEMMs on
// the 16-bit matrix pipe, every fp32 operand carried as a few 16-bit terms (mirx_device.h "term schemes"; k_linear_split.hip
// for the arithmetic and the measured error): ONE kernel template k_attention_split<S, DH> for both schemes and every head_dim.
//   S = SplitBf16x3: x = xh + xm + xl exactly, six v_mfma_f32_32x32x16_bf16 per product block, dropped cross terms
//                    <= 3 * 2^-24 |a b| (fp32-grade); no range contract                            (launch_attention_s3)
//   S = SplitF16x2:  two fp16 terms, three v_mfma_f32_32x32x16_f16 per product block.  fp16's range is the caller's contract:
//                    `qk_bound` >= max |q|, |k| and `v_bound` >= max |v| over the packed projection (mirx.model derives them
//                    from the LayerNorm and the projection's row norms); the launcher turns them into exact power-of-two
//                    scales: Q is staged as q * (scale log2 e) * qs, K as k * ks, V as v * vs, the probabilities (in [0, 1])
//                    as p * 1024, and the accumulators are multiplied back by 1 / (qs ks) inside the softmax's exponent and
//                    by 1 / (1024 vs) at the end.  These steps exist only under S::SCALED.              (launch_attention_h2)
//   DH = 64 (ViT-B / DINOv2), 32 / 72 / 96 (72: the SigLIP-So400m tower): any multiple of 8 would do.
//   S^T[key, q] = K[key, :] . Q[q, :]         A = K tile (LDS, split while staged), B = Q (split once, registers)
//   O^T[d, q]  += V^T[d, key] . P^T[key, q]   A = V^T tile (LDS, split + transposed while staged),
//                                             B = P, split in registers straight from the S accumulators
//
// Geometry as k_attention: one workgroup = 128 queries (4 waves x 32) of one (image, head), keys 32 at a time, a lane owns one
// query (online softmax per lane + one exchange with lane ^ 32).  The accumulator layout of the first GEMM hands lane (q, h)
// the keys  kappa(r, h) = 8 (r >> 2) + (r & 3) + 4 h,  r = 0..15; the second GEMM contracts the keys in exactly that order --
// step s, k-group h, element i  <->  key kappa(8 s + i, h) -- so P never moves between lanes, and V^T is stored with its key
// axis permuted to match (position 16 s + 8 h + i).
// LDS, per term: a K plane [32 keys][KS = ceil(DH / 16) MFMA steps of 16 channels] (channels beyond DH are zero in Q and K) and
// a V^T plane [DH d][32 positions] (64 B rows, 16-byte chunk c at c ^ ((d >> 2) & 3): the chunk index changes every 256
// bytes).  The 16-byte chunks of a K row are XORed with (key >> 1) & 7 where the row is 128 bytes (head_dim 64, again every 256
// bytes) and rotated by key >> 2 otherwise (the chunk count is not a power of two; head_dim 32's four chunks keep the rotation,
// which is the layout k_attention_win shares).  The output has NT = ceil(DH / 32) tiles; the lanes of a partly filled last
// tile re-read row DH - 1 of V^T and their results are dropped.  Staging walks item lists (K: key x chunk, V: key pair x 4
// channels) of 256 threads at a time; only head_dim 64's lists divide by 256, so only there every lane always has an item.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

// Diagnostic builds (results wrong, timing only; -DMIRX_DIAG), every instantiation: bits of MIRX_ATT_EXP -- 1 no softmax
// arithmetic, 2 no tile staging after the first tile, 4 no P V MFMAs, 8 no Q K MFMAs, 16 no workgroup barrier in the K loop
#ifndef MIRX_ATT_EXP
#define MIRX_ATT_EXP 0
#endif
constexpr int KT = 32;                 // keys per tile
// bytes of one term of a tile: the K plane and the V^T plane (8 KiB at head_dim 64)
constexpr int term_bytes(int dh) { return KT * ((dh + 15) / 16) * 32 + dh * 64; }

// XCD-aware order: workgroups are dealt to the 8 XCDs round-robin in linear order (x fastest), so the query tiles of one
// (image, head) -- which all stream the same K and V -- would sit behind eight different L2s.  Re-dealt, XCD x takes the
// (image, head) pairs x, x + 8, .. query tile by query tile: K / V of a pair cross the fabric once.  (Any bijection is correct.)
__device__ inline void attention_block(int &qt, int &head, int64_t &img) {
    qt = blockIdx.x;
    head = blockIdx.y;
    img = blockIdx.z;
#ifndef MIRX_ATT_PLAIN_ORDER
    const unsigned nqt = gridDim.x, npair = gridDim.y * gridDim.z, full = npair & ~7u;
    const unsigned lin = blockIdx.x + nqt * (blockIdx.y + gridDim.y * blockIdx.z);
    if (lin < nqt * full) {
        const unsigned j = lin >> 3;
        const unsigned pair = (j / nqt) * 8 + (lin & 7);
        qt = (int)(j % nqt);
        head = (int)(pair % gridDim.y);
        img = pair / gridDim.y;
    }
#endif
}

template <class S, int DH>
__global__ __launch_bounds__(256, DH == 64 ? 3 : 2) void k_attention_split(const float *__restrict__ qkv, int n, int heads,
                                                                          float q_mul, float k_mul, float v_mul, float s_inv,
                                                                          float o_inv, float *__restrict__ out,
                                                                          char *__restrict__ out_t, float t_scale) {
    constexpr int T = S::T;                                                // terms per operand
    typedef typename S::frag frag;
    constexpr int KS = (DH + 15) / 16, KCH = 2 * KS, KROW = KCH * 16;      // K row: KCH chunks of 16 B
    constexpr int NT = (DH + 31) / 32;
    constexpr int KPL = KT * KROW, VPL = DH * 64, BUF = T * (KPL + VPL);   // = T * term_bytes(DH): 16 / 24 KiB at head_dim 64
    // chunk c of K row `key` sits at chunk k_pos(c, key) of the row
    auto k_pos = [](int c, int key) { return KROW == 128 ? c ^ ((key >> 1) & 7) : (c + (key >> 2)) % KCH; };
    extern __shared__ __attribute__((aligned(16))) char sm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int half = lane >> 5, nq = lane & 31;
    int qt, head;
    int64_t img;
    attention_block(qt, head, img);
    const int64_t tok = 3 * (int64_t)heads * DH;                          // floats per token in qkv
    const float *base = qkv + img * n * tok + head * DH;                   // q of token t: base + t*tok; k: + heads*DH; v: + 2*heads*DH
    const int q_idx = qt * 128 + wave * 32 + nq;
    const int q_ld = q_idx < n ? q_idx : n - 1;

    // this lane's query: channels 16 ks + 8 half + i, pre-multiplied by scale * log2(e) (and qs), T terms each
    frag q[KS][T];
    {
        const float *qp = base + q_ld * tok;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c0 = 16 * ks + 8 * half;                             // DH % 8 == 0: a chunk is all in or all out
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (c0 < DH) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(qp + c0), b = *reinterpret_cast<const f32x4 *>(qp + c0 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { v[j] = a[j] * q_mul; v[4 + j] = b[j] * q_mul; }
            }
            S::split_x8(v, q[ks]);
        }
    }

    // ---- staging item lists: thread t takes items t, t + 256, .. ---------------------------------------------------
    // K item: (key, chunk of 8 channels = two float4)            -> one 16-byte chunk per term
    // V item: (keys 2 m, 2 m + 1, channels 4 vc .. + 3)          -> four 16-bit pairs per term
    constexpr int NKI = KT * KCH, IPK = (NKI + 255) / 256;
    constexpr int NVI = (KT / 2) * (DH / 4), IPV = (NVI + 255) / 256;
    f32x4 rk[IPK][2], rv[IPV][2];
    // `live`: the lane has an item (always, where the list divides by 256: no predicate is compiled); a lane without one
    // loads the last item again and stores nothing
    auto k_item = [&](int i, int &key, int &c, bool &live) {
        int it = threadIdx.x + 256 * i;
        live = NKI % 256 == 0 || it < NKI;
        if (!live) it = NKI - 1;
        key = it / KCH;
        c = it % KCH;
    };
    auto v_item = [&](int i, int &m, int &vc, bool &live) {
        int it = threadIdx.x + 256 * i;
        live = NVI % 256 == 0 || it < NVI;
        if (!live) it = NVI - 1;
        m = it / (DH / 4);
        vc = it % (DH / 4);
    };
    // K / V rows come through a buffer descriptor over THIS image's n token rows: a lane's byte offset inside a tile is fixed
    // for the whole launch and the tile's offset is one scalar, so the loop holds no address arithmetic (it was ~40 of its ~250
    // vector instructions: clamps, 32-bit multiplies, 64-bit adds); rows beyond n are out of range and read as zero -- their
    // scores are set to -inf in the tail tile and their probabilities are exactly 0.
    const __amdgpu_buffer_rsrc_t kvrs = __builtin_amdgcn_make_buffer_rsrc((void *)(qkv + img * n * tok), 0,
                                                                          (unsigned)((int64_t)n * tok * 4), 0x00020000);
    const unsigned row_b = (unsigned)(tok * 4), tile_b = (unsigned)(KT * tok * 4);
    unsigned vo_k[IPK], vo_v[IPV];
#pragma unroll
    for (int i = 0; i < IPK; ++i) {
        int key, c; bool live;
        k_item(i, key, c, live);
        const int cc = 8 * c < DH ? 8 * c : DH - 8;                        // pad chunk: read something valid, store zeros
        vo_k[i] = (unsigned)((key * tok + (heads + head) * DH + cc) * 4);
    }
#pragma unroll
    for (int i = 0; i < IPV; ++i) {
        int m, vc; bool live;
        v_item(i, m, vc, live);
        vo_v[i] = (unsigned)((2 * m * tok + (2 * heads + head) * DH + 4 * vc) * 4);
    }
    auto load_tile = [&](int kt) {
        const unsigned so = (unsigned)kt * tile_b;                        // wave-uniform
#pragma unroll
        for (int i = 0; i < IPK; ++i) {
            rk[i][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(kvrs, vo_k[i], so, 0));
            rk[i][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(kvrs, vo_k[i] + 16u, so, 0));
        }
#pragma unroll
        for (int i = 0; i < IPV; ++i) {
            rv[i][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(kvrs, vo_v[i], so, 0));
            rv[i][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(kvrs, vo_v[i] + row_b, so, 0));
        }
    };
    auto store_tile = [&](int buf) {
        char *sb = sm + buf * BUF;
#pragma unroll
        for (int i = 0; i < IPK; ++i) {
            int key, c; bool live;
            k_item(i, key, c, live);
            const bool real = 8 * c < DH;
            const float km = real ? k_mul : 0.f;                           // pad chunk: zeros
            u32x4 pk[T];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float a = rk[i][p >> 1][2 * (p & 1)], b = rk[i][p >> 1][2 * (p & 1) + 1];
                if (!S::SCALED && !real) a = b = 0.f;                      // (no scale to carry the zero)
                unsigned t[T];
                S::split_pair(a, b, km, t);
#pragma unroll
                for (int j = 0; j < T; ++j) pk[j][p] = t[j];
            }
            if (live) {
                const int pos = k_pos(c, key);
                char *d = sb + key * KROW + pos * 16;
#pragma unroll
                for (int j = 0; j < T; ++j) *reinterpret_cast<u32x4 *>(d + j * KPL) = pk[j];
            }
        }
#pragma unroll
        for (int i = 0; i < IPV; ++i) {
            int m, vc; bool live;
            v_item(i, m, vc, live);
            const int vkey = 2 * m;
            // position of key k on the permuted axis: 16 (k >> 4) + 8 ((k >> 2) & 1) + (k & 3) + 4 ((k >> 3) & 1)
            const int vpos = 16 * (vkey >> 4) + 8 * ((vkey >> 2) & 1) + (vkey & 3) + 4 * ((vkey >> 3) & 1);   // even
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned t[T];
                S::split_pair(rv[i][0][j], rv[i][1][j], v_mul, t);         // keys 2m, 2m + 1 of channel 4 vc + j
                const int d = 4 * vc + j;
                char *dst = sb + T * KPL + d * 64 + (((vpos >> 3) ^ ((d >> 2) & 3)) << 4) + (vpos & 7) * 2;
                if (live) {
#pragma unroll
                    for (int u = 0; u < T; ++u) *reinterpret_cast<unsigned *>(dst + u * VPL) = t[u];
                }
            }
        }
    };

    // fragment addresses: K row nq (key), chunk 2 ks + half; V^T row 32 t + nq (d), chunk 2 s + half
    int fk[KS], fv[NT][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int pos = k_pos(2 * ks + half, nq);
        fk[ks] = nq * KROW + pos * 16;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int d = 32 * t + nq < DH ? 32 * t + nq : DH - 1;
            fv[t][s] = T * KPL + d * 64 + (((2 * s + half) ^ ((d >> 2) & 3)) << 4);
        }

    f32x16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[t][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;

    const int ntiles = (n + KT - 1) / KT;
    load_tile(0);
    store_tile(0);
    for (int kt = 0; kt < ntiles; ++kt) {
        const int cur = kt & 1;
        if (!(MIRX_ATT_EXP & 16)) __syncthreads();         // tile kt visible; buffer cur ^ 1 free
        if (!(MIRX_ATT_EXP & 2)) load_tile(kt + 1 < ntiles ? kt + 1 : kt);          // branch-free: the last tile re-loads itself
        __builtin_amdgcn_sched_barrier(0);
        const char *sb = sm + cur * BUF;

        // ---- S^T = K Q^T ----------------------------------------------------------------------------------------
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            // (here and in the second GEMM: constant indices and the scheme's product macro by name.  A loop over T and
            // S::product are the same arithmetic, but they moved the register allocation of the fp16 instantiations at head_dim
            // 72 and 96 off the code this kernel was tuned as -- profiles/r29_attention_one_source.txt)
            frag a[T];
            a[0] = *reinterpret_cast<const frag *>(sb + fk[ks]);
            a[1] = *reinterpret_cast<const frag *>(sb + fk[ks] + KPL);
            if constexpr (T == 3) a[2] = *reinterpret_cast<const frag *>(sb + fk[ks] + 2 * KPL);
            if (MIRX_ATT_EXP & 8) { sacc[ks] += (float)a[0][0] + (float)a[T - 1][1] + (float)q[ks][0][2]; continue; }
            if constexpr (T == 3) MIRX_MFMA6(sacc, a[0], a[1], a[2], q[ks][0], q[ks][1], q[ks][2]) else MIRX_MFMA3(sacc, a[0], a[1], q[ks][0], q[ks][1])
        }
        // (the scores stay unscaled: s_inv, a power of two, goes into the exponent's multiply-add below -- the same bits)

        // ---- online softmax over this lane's 16 keys (base 2) -----------------------------------------------------
        const int key0 = kt * KT + 4 * half;
        const bool tail_tile = (kt + 1) * KT > n;          // wave-uniform: only the last tile can hold keys beyond n
        float mt = -INFINITY;
        if (tail_tile) {
            // a real branch (the empty asm keeps the compiler from turning it into 16 compares, 16 selects and 16 scalar ORs
            // executed for EVERY tile: a fifth of the loop's vector instructions)
            asm volatile("" ::: "memory");
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + 8 * (r >> 2) + (r & 3);
                if (key >= n) sacc[r] = -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sacc[r]);
        mt = max_over_halves(mt);                          // the other 16 keys of the same query
        mt = S::SCALED ? mt * s_inv : mt;                  // max commutes with the positive scale
        const float m_new = fmaxf(m_run, mt);              // finite: every tile holds at least one valid key
        const float alpha = exp2_raw(m_run - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!(MIRX_ATT_EXP & 1)) sacc[r] = exp2_raw(S::SCALED ? fmaf(sacc[r], s_inv, -m_new) : sacc[r] - m_new);
            psum += sacc[r];
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
        if (!(MIRX_ATT_EXP & 1) && !__all(alpha == 1.0f)) {                       // wave-uniform: once the running maxima have settled there is nothing to rescale
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
        }

        // ---- O^T += V^T P^T: step s contracts the keys kappa(8 s + i, half) = this lane's sacc[8 s + i] -------------
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float pv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) pv[j] = S::SCALED ? sacc[8 * s + j] * 1024.f : sacc[8 * s + j];
            frag b[T];
            S::split_x8(pv, b);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                frag a[T];
                a[0] = *reinterpret_cast<const frag *>(sb + fv[t][s]);
                a[1] = *reinterpret_cast<const frag *>(sb + fv[t][s] + VPL);
                if constexpr (T == 3) a[2] = *reinterpret_cast<const frag *>(sb + fv[t][s] + 2 * VPL);
                if (MIRX_ATT_EXP & 4) { o[t][s] += (float)a[0][0] + (float)a[T - 1][1] + (float)b[0][2] + (float)b[T - 1][3]; continue; }
                if constexpr (T == 3) MIRX_MFMA6(o[t], a[0], a[1], a[2], b[0], b[1], b[2]) else MIRX_MFMA3(o[t], a[0], a[1], b[0], b[1])
            }
        }
        if (!(MIRX_ATT_EXP & 2)) store_tile(cur ^ 1);
    }

    // ---- normalise and store: register r of o[t] is channel 32 t + 8 (r >> 2) + (r & 3) + 4 half ------------------
    l_run += __shfl_xor(l_run, 32, 64);
    if (q_idx < n) {
        const float inv = (S::SCALED ? o_inv : 1.0f) / l_run;
        float *op = out + ((img * n + q_idx) * heads + head) * DH + 4 * half;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (32 * t + 8 * g + 4 * half >= DH) continue;
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = o[t][4 * g + j] * inv;
                if (out_t) store_terms4(out_t, (img * n + q_idx), heads * DH, head * DH + 4 * half + 32 * t + 8 * g, v, t_scale);
                else *reinterpret_cast<f32x4 *>(op + 32 * t + 8 * g) = v;
            }
    }
}

struct AttentionLaunch {
    const float *qkv;
    int64_t batch;
    int n, heads;
    float q_mul, k_mul, v_mul, s_inv, o_inv;               // the bf16 scheme reads q_mul alone
    float *out;
    char *out_t;
    float t_scale;
    hipStream_t st;
};

// One instantiation; its dynamic-LDS limit (72 KiB for the bf16 scheme at head_dim 96) is raised on its first launch on each device.
template <class S, int DH>
hipError_t launch_arm(const AttentionLaunch &a) {
    static std::atomic<unsigned long long> attr_devs{0};
    constexpr size_t lds = 2 * (size_t)(S::T * term_bytes(DH));
    const hipError_t e = set_dynamic_lds(k_attention_split<S, DH>, lds, &attr_devs);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((a.n + 127) / 128), (unsigned)a.heads, (unsigned)a.batch);
    hipLaunchKernelGGL((k_attention_split<S, DH>), grid, dim3(256), lds, a.st, a.qkv, a.n, a.heads, a.q_mul, a.k_mul, a.v_mul,
                       a.s_inv, a.o_inv, a.out, a.out_t, a.t_scale);
    return hipGetLastError();
}

// The argument checks both schemes share.
bool launch_args_ok(int64_t batch, int n, int heads, int head_dim) {
    if (heads <= 0 || heads > 65535 || batch > 65535) return false;
    if (head_dim != 32 && head_dim != 64 && head_dim != 72 && head_dim != 96) return false;
    return (int64_t)n * 3 * heads * head_dim * 4 < ((int64_t)1 << 31);    // an image's qkv rows: 32-bit buffer offsets
}

template <class S>
hipError_t launch_head_dim(const AttentionLaunch &a, int head_dim) {
    return head_dim == 64 ? launch_arm<S, 64>(a) : head_dim == 72 ? launch_arm<S, 72>(a)
         : head_dim == 96 ? launch_arm<S, 96>(a) : launch_arm<S, 32>(a);
}

}  // namespace

hipError_t launch_attention_s3(const float *qkv, int64_t batch, int n, int heads, int head_dim, float scale, float *out,
                               hipStream_t st) {
    if (batch <= 0 || n <= 0) return hipSuccess;
    if (!launch_args_ok(batch, n, heads, head_dim)) return hipErrorInvalidValue;
    return launch_head_dim<SplitBf16x3>({qkv, batch, n, heads, scale * 1.4426950408889634f, 1.f, 1.f, 1.f, 1.f, out, nullptr, 1.f, st},
                                        head_dim);
}

hipError_t launch_attention_h2(const float *qkv, int64_t batch, int n, int heads, int head_dim, float scale,
                               float qk_bound, float v_bound, float *out, hipStream_t st, void *out_terms, float terms_scale) {
    if (batch <= 0 || n <= 0) return hipSuccess;
    if (!launch_args_ok(batch, n, heads, head_dim)) return hipErrorInvalidValue;
    if (!(qk_bound > 0.f) || !(v_bound > 0.f) || !(scale > 0.f)) return hipErrorInvalidValue;
    if ((out != nullptr) == (out_terms != nullptr) || (heads * head_dim) % 4) return hipErrorInvalidValue;
    const float sl = scale * 1.4426950408889634f;
    // powers of two that bring each operand's bound to at most 2^14 (fp16 max 65504)
    const float qs = exp2f(floorf(log2f(16384.0f / (qk_bound * sl))));
    const float ks = exp2f(floorf(log2f(16384.0f / qk_bound)));
    const float vs = exp2f(floorf(log2f(16384.0f / v_bound)));
    return launch_head_dim<SplitF16x2>({qkv, batch, n, heads, sl * qs, ks, vs, 1.0f / (qs * ks), 1.0f / (1024.0f * vs), out,
                                        reinterpret_cast<char *>(out_terms), terms_scale, st}, head_dim);
}

}  // namespace mirx
