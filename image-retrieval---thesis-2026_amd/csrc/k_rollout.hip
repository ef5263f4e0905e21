// k_rollout.hip -- attention rollout for the SigLIP vision tower (the reference's explanations.py AttentionRolloutMedSigLIP).
// The explainer uses only rollout.mean(dim=1) = (1/N) 1^T A_{L-1} ... A_0, so the N^3 products of the reference's bmm chain
// become a vector walked from the last layer to the first.  Per layer l and image b the matrix
//     A_l = normalise(discard(fuse_h softmax((q_h k_h^T) * scale)) + I)
// is formed straight from the packed qkv [b, n, 3c] (q | k | v, heads along c) the native encoder layer computes:
//
//   k_rollout_layer   one workgroup per (image, 16 query rows, split of the heads): up to RO_HEAD_SPLIT splits of consecutive
//                     heads (a function of the head count alone), heads ascending within a split.  Per head: the Q block into
//                     LDS as float4; S = q k^T for the row block on v_mfma_f32_16x16x4_f32 (f32 operands and accumulator,
//                     each element a fixed-order reduction over head_dim; head_dim 64 / 72 compiled with the next tile's K
//                     loads in flight during the current tile's MFMA chain), times scale, into LDS (16 x 1024 floats); per
//                     row the exact softmax with a fixed-order row max and row sum (lane-local ascending, then a fixed
//                     butterfly); fused into 64 VGPRs per lane: sum, max or min, NaN kept; stored per split.
//   k_rollout_combine the splits in split order (sum then / heads, max, min), the row stage below, the stores into the workspace
//                     slot of layer l.
//   row stage         per row, one wave, 16 values per lane: the k-th smallest value by a bitwise binary search on the
//                     order-preserving keys of the fp32 bit patterns (32 exact count passes), a * (a > thr) (ties at the
//                     threshold dropped, NaN kept), + 1 on the diagonal, / (row sum + 1e-8).  Also an entry of its own
//                     (k_rollout_rows) on a caller's [rows, n] matrix, diagonal at column row % n.
//   k_rollout_chain   v <- v^T A_l for l = L-1 .. 0, v = 1/N first: one launch per layer; a workgroup owns 64 columns and one
//                     of RO_SPLITS row ranges, a lane sums its column over the rows in order; the partial sums of the
//                     RO_SPLITS ranges are added in range order by whoever reads them next.
//   k_rollout_importance  v (partials in range order), times clamp(patch . query, 0) when patches are given (a wave per
//                     token, fixed-order dot).
//   k_rollout_upsample    the h x w map in LDS, bilinear (align_corners=False) into the caller's [b, H, W].
//
// Every output for image b is a fixed-order function of image b's qkv (and patches) alone: bit-identical whatever b is.
#include <algorithm>
#include <cmath>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int RO_ROWS = 16;              // query rows per layer workgroup (one MFMA tile edge)
constexpr int RO_THREADS = 256;          // 4 waves; wave w owns rows 4w .. 4w + 3 of the block in the softmax / row stage
constexpr int RO_VALS = MIRX_ROLLOUT_MAX_N / 64;   // values per lane per row (16)
constexpr int RO_S_STRIDE = MIRX_ROLLOUT_MAX_N + 4;
constexpr int RO_Q_STRIDE = MIRX_ROLLOUT_MAX_HEAD_DIM + 4;
constexpr int RO_SPLITS = 8;             // row ranges of the chain
constexpr int RO_MAP_ROWS = 16;          // output rows per upsample workgroup
// heads per layer split over up to RO_HEAD_SPLIT workgroups per row block (a function of the head count only, never of b: the
// fusion order stays fixed); MIRX_RO_SPLIT overrides it in diagnostic builds (tools/bench_rollout.py A/Bs)
#if defined(MIRX_DIAG) && defined(MIRX_RO_SPLIT)
constexpr int RO_HEAD_SPLIT = MIRX_RO_SPLIT;
#else
constexpr int RO_HEAD_SPLIT = 4;
#endif

// order-preserving key of an fp32 bit pattern (negative values below positive ones, -0 just below +0)
__device__ inline uint32_t fkey(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float funkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The reference's per-row stage on one row held by a wave (value t of a lane is column lane + 64 t; columns >= n unused):
//   k > 0: thr = kthvalue(row, k); a = a * (a > thr)     then   a = a + I;  a = a / (a.sum() + 1e-8)
__device__ inline void row_stage(float (&v)[RO_VALS], int n, int k, int diag, int lane) {
    if (k > 0) {
        // the k-th smallest key: the largest P with #{key < P} < k, built from the top bit down (exact counts)
        uint32_t key[RO_VALS];
#pragma unroll
        for (int t = 0; t < RO_VALS; ++t) key[t] = fkey(v[t]);
        uint32_t p = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t c = p | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < RO_VALS; ++t) cnt += (lane + 64 * t < n && key[t] < c) ? 1 : 0;
            if (wave_isum(cnt) < k) p = c;
        }
        const float thr = funkey(p);
#pragma unroll
        for (int t = 0; t < RO_VALS; ++t) v[t] = v[t] * (v[t] > thr ? 1.f : 0.f);
    }
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < RO_VALS; ++t) {
        const int j = lane + 64 * t;
        if (j < n) {
            v[t] = v[t] + (j == diag ? 1.f : 0.f);
            s += v[t];
        }
    }
    const float d = wave_sum(s) + 1e-8f;
#pragma unroll
    for (int t = 0; t < RO_VALS; ++t) v[t] = v[t] / d;
}

struct LayerArgs {
    const float *qkv;        // [b, n, 3c]
    int n, heads, dh, hper;  // hper: heads per split (split s takes heads s * hper .. min(heads, (s + 1) * hper) - 1)
    int64_t c, b;
    float scale;
    int fusion;
    float *part;             // [splits][b][n][n]: each split's fused heads (sum / max / min, no division)
};

// K rows of one 16-key tile for one lane: lane group g holds d = 16 m + 4 g .. + 3 (float4 m) and the tail d = 16 NF + 4 u + g
template <int DH> struct KTile {
    static constexpr int NF = DH / 16, NT = (DH % 16) / 4;
    float4 f[NF];
    float t[NT > 0 ? NT : 1];
    // keys j >= n read row 0 instead (their S columns are never read): no branch around the loads, so the wait before a
    // tile's MFMA chain can leave the other tile's loads in flight
    __device__ inline void load(const float *base, int64_t c3, int64_t koff, int j, int n, int g) {
        const float *kr = base + (int64_t)(j < n ? j : 0) * c3 + koff;
#pragma unroll
        for (int m = 0; m < NF; ++m) f[m] = *reinterpret_cast<const float4 *>(kr + 16 * m + 4 * g);
#pragma unroll
        for (int u = 0; u < NT; ++u) t[u] = kr[16 * NF + 4 * u + g];
    }
};

// S[r, j] = sum_d q[r, d] k[j, d] for one 16 x 16 tile: one chain of v_mfma_f32_16x16x4_f32 in d order
template <int DH> __device__ inline f32x4 score_tile(const KTile<DH> &kt, const float *qrow, int g) {
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < KTile<DH>::NF; ++m) {
        const float4 q = *reinterpret_cast<const float4 *>(qrow + 16 * m + 4 * g);
        s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.x, kt.f[m].x, s4, 0, 0, 0);
        s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.y, kt.f[m].y, s4, 0, 0, 0);
        s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.z, kt.f[m].z, s4, 0, 0, 0);
        s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.w, kt.f[m].w, s4, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < KTile<DH>::NT; ++u)
        s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(qrow[16 * KTile<DH>::NF + 4 * u + g], kt.t[u], s4, 0, 0, 0);
    return s4;
}

// DH > 0: head_dim fixed at compile time, the next tile's K loads in flight during the current tile's MFMA chain;
// DH == 0: any head_dim % 4 == 0 (the K loads inside the chain)
template <int DH>
__global__ __launch_bounds__(RO_THREADS) void k_rollout_layer(LayerArgs a) {
    __shared__ float Ss[RO_ROWS * RO_S_STRIDE];
    __shared__ __attribute__((aligned(16))) float Qs[RO_ROWS * RO_Q_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bi = blockIdx.z;
    const int split = blockIdx.y;
    const int row0 = blockIdx.x * RO_ROWS;
    const int n = a.n, dh = DH > 0 ? DH : a.dh;
    const int h0 = split * a.hper, h1 = min(a.heads, h0 + a.hper);
    const int64_t c3 = 3 * a.c;
    const float *base = a.qkv + bi * (int64_t)n * c3;
    float acc[4][RO_VALS];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int t = 0; t < RO_VALS; ++t) acc[rr][t] = 0.f;
    const int ntiles = (n + 15) / 16;
    const int g = lane >> 4, l16 = lane & 15;
    const int dq = dh / 4;
    for (int h = h0; h < h1; ++h) {
        __syncthreads();                                          // the previous head's S and Q are consumed
        for (int e = tid; e < RO_ROWS * dq; e += RO_THREADS) {   // the Q block, one float4 per thread and pass
            const int r = e / dq, d = 4 * (e - r * dq);
            const float4 q = (row0 + r < n) ? *reinterpret_cast<const float4 *>(base + (int64_t)(row0 + r) * c3 + (int64_t)h * dh + d)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4 *>(Qs + r * RO_Q_STRIDE + d) = q;
        }
        __syncthreads();
        const int64_t koff = a.c + (int64_t)h * dh;
        const float *qrow = Qs + l16 * RO_Q_STRIDE;
        if constexpr (DH > 0) {
            // two tiles in flight per wave: tile t + 4 (or the last tile again) loads while tile t's chain runs
            KTile<DH> ka, kb;
            const int last = ntiles - 1;
            auto store = [&](const f32x4 &s4, int tile) {
#pragma unroll
                for (int e = 0; e < 4; ++e) Ss[(4 * g + e) * RO_S_STRIDE + tile * 16 + l16] = s4[e] * a.scale;   // row 4 g + e
            };
            if (wave <= last) {
                ka.load(base, c3, koff, wave * 16 + l16, n, g);
                for (int tile = wave;; tile += 8) {
                    kb.load(base, c3, koff, min(tile + 4, last) * 16 + l16, n, g);
                    __builtin_amdgcn_sched_barrier(0);            // keep the loads ahead of the other tile's chain
                    store(score_tile<DH>(ka, qrow, g), tile);
                    if (tile + 4 > last) break;
                    ka.load(base, c3, koff, min(tile + 8, last) * 16 + l16, n, g);
                    __builtin_amdgcn_sched_barrier(0);
                    store(score_tile<DH>(kb, qrow, g), tile + 4);
                    if (tile + 8 > last) break;
                }
            }
        } else {
            // lane group g takes d = 16 m + 4 g + s of each 16-wide block (one float4 of K), then d = d0 + g for the tail
            const int dh16 = dh & ~15;
            for (int tile = wave; tile < ntiles; tile += 4) {
                const int j = tile * 16 + l16;
                const bool jv = j < n;
                const float *kr = base + (int64_t)(jv ? j : 0) * c3 + koff;
                f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
                for (int m = 0; m < dh16; m += 16) {
                    const float4 kv = jv ? *reinterpret_cast<const float4 *>(kr + m + 4 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 q = *reinterpret_cast<const float4 *>(qrow + m + 4 * g);
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.x, kv.x, s4, 0, 0, 0);
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.y, kv.y, s4, 0, 0, 0);
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.z, kv.z, s4, 0, 0, 0);
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.w, kv.w, s4, 0, 0, 0);
                }
                for (int d0 = dh16; d0 < dh; d0 += 4)
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(qrow[d0 + g], jv ? kr[d0 + g] : 0.f, s4, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) Ss[(4 * g + e) * RO_S_STRIDE + tile * 16 + l16] = s4[e] * a.scale;
            }
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * wave + rr;
            if (row0 + r >= n) continue;                          // wave-uniform
            const float *sr = Ss + r * RO_S_STRIDE;
            float m = -INFINITY;
#pragma unroll
            for (int t = 0; t < RO_VALS; ++t)
                if (lane + 64 * t < n) m = nanmax(m, sr[lane + 64 * t]);
            m = wave_nanmax(m);
            float ev[RO_VALS], s = 0.f;
#pragma unroll
            for (int t = 0; t < RO_VALS; ++t) {
                ev[t] = (lane + 64 * t < n) ? expf(sr[lane + 64 * t] - m) : 0.f;
                s += ev[t];
            }
            s = wave_sum(s);
#pragma unroll
            for (int t = 0; t < RO_VALS; ++t) {
                const float p = ev[t] / s;
                if (h == h0) acc[rr][t] = p;
                else if (a.fusion == MIRX_ROLLOUT_FUSE_MAX) acc[rr][t] = nanmax(acc[rr][t], p);
                else if (a.fusion == MIRX_ROLLOUT_FUSE_MIN) acc[rr][t] = nanmin(acc[rr][t], p);
                else acc[rr][t] = acc[rr][t] + p;
            }
        }
    }
    float *ob = a.part + ((int64_t)split * a.b + bi) * (int64_t)n * n;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * wave + rr;
        if (row0 + r >= n) continue;
        float *orow = ob + (int64_t)(row0 + r) * n;
#pragma unroll
        for (int t = 0; t < RO_VALS; ++t)
            if (lane + 64 * t < n) orow[lane + 64 * t] = acc[rr][t];
    }
}

// the splits' fused heads combined in split order (sum then / heads, max or min), then the row stage, into A_l
__global__ __launch_bounds__(RO_THREADS) void k_rollout_combine(const float *part, int splits, int64_t b, int n, int heads, int fusion, int k,
                                                               float *out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t bi = blockIdx.y;
    if (row >= n) return;                                         // wave-uniform
    const int64_t nn = (int64_t)n * n, off = bi * nn + (int64_t)row * n;
    float v[RO_VALS];
#pragma unroll
    for (int t = 0; t < RO_VALS; ++t) v[t] = (lane + 64 * t < n) ? part[off + lane + 64 * t] : 0.f;
    for (int s = 1; s < splits; ++s) {
        const float *ps = part + (int64_t)s * b * nn + off;
#pragma unroll
        for (int t = 0; t < RO_VALS; ++t) {
            const float p = (lane + 64 * t < n) ? ps[lane + 64 * t] : 0.f;
            if (fusion == MIRX_ROLLOUT_FUSE_MAX) v[t] = nanmax(v[t], p);
            else if (fusion == MIRX_ROLLOUT_FUSE_MIN) v[t] = nanmin(v[t], p);
            else v[t] = v[t] + p;
        }
    }
    if (fusion == MIRX_ROLLOUT_FUSE_MEAN) {
#pragma unroll
        for (int t = 0; t < RO_VALS; ++t) v[t] = v[t] / (float)heads;
    }
    row_stage(v, n, k, row, lane);
    float *orow = out + off;
#pragma unroll
    for (int t = 0; t < RO_VALS; ++t)
        if (lane + 64 * t < n) orow[lane + 64 * t] = v[t];
}

__global__ __launch_bounds__(RO_THREADS) void k_rollout_rows(float *x, int64_t rows, int n, int k) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                      // wave-uniform
    float *xr = x + row * n;
    float v[RO_VALS];
#pragma unroll
    for (int t = 0; t < RO_VALS; ++t) v[t] = (lane + 64 * t < n) ? xr[lane + 64 * t] : 0.f;
    row_stage(v, n, k, (int)(row % n), lane);
#pragma unroll
    for (int t = 0; t < RO_VALS; ++t)
        if (lane + 64 * t < n) xr[lane + 64 * t] = v[t];
}

// the chain: vout[split][j] = sum over rows i of the split (ascending) of v[i] * A[i, j]; v[i] = 1 / n on the first step,
// else the sum of vin[0 .. RO_SPLITS - 1][i] in split order
__global__ __launch_bounds__(RO_THREADS) void k_rollout_chain(const float *A, const float *vin, float *vout, int n, int first) {
    __shared__ float vs[MIRX_ROLLOUT_MAX_N / RO_SPLITS];
    __shared__ float part[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bi = blockIdx.z;
    const int split = blockIdx.y;
    const int per = (n + RO_SPLITS - 1) / RO_SPLITS;
    const int i0 = split * per, i1 = min(n, i0 + per);
    const float *vb = vin + bi * (int64_t)RO_SPLITS * n;
    for (int i = i0 + tid; i < i1; i += RO_THREADS) {
        float v = 0.f;
        if (first) {
            v = 1.f / (float)n;
        } else {
#pragma unroll
            for (int s = 0; s < RO_SPLITS; ++s) v += vb[(int64_t)s * n + i];
        }
        vs[i - i0] = v;
    }
    __syncthreads();
    const int j = blockIdx.x * 64 + lane;
    const int sub = (per + 3) / 4;
    const int w0 = min(i1, i0 + wave * sub), w1 = min(i1, w0 + sub);
    float s = 0.f;
    if (j < n) {
        const float *Ab = A + bi * (int64_t)n * n + j;
        for (int i = w0; i < w1; ++i) s += vs[i - i0] * Ab[(int64_t)i * n];
    }
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && j < n)
        vout[bi * (int64_t)RO_SPLITS * n + (int64_t)split * n + j] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// imp[b, j] = (sum_s v[s][j]) * clamp(patches[b, j] . query, 0) (NaN kept), or the sum alone without patches
__global__ __launch_bounds__(RO_THREADS) void k_rollout_importance(const float *vin, const float *patches, const float *query, int64_t e,
                                                                  int n, float *imp) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t bi = blockIdx.y;
    if (j >= n) return;                                           // wave-uniform
    const float *vb = vin + bi * (int64_t)RO_SPLITS * n;
    float v = 0.f;
#pragma unroll
    for (int s = 0; s < RO_SPLITS; ++s) v += vb[(int64_t)s * n + j];
    if (patches) {
        const float *pr = patches + (bi * n + j) * e;
        float d = 0.f;
        for (int64_t c = lane; c < e; c += 64) d += pr[c] * query[c];
        d = wave_sum(d);
        v = v * ((d > 0.f || d != d) ? d : 0.f);
    }
    if (lane == 0) imp[bi * n + j] = v;
}

// bilinear, align_corners=False (ATen's upsample_bilinear2d source index: max(scale * (dst + 0.5) - 0.5, 0))
__global__ __launch_bounds__(RO_THREADS) void k_rollout_upsample(const float *imp, int h, int w, int H, int W, float *out) {
    __shared__ float smap[MIRX_ROLLOUT_MAX_N];
    const int tid = threadIdx.x;
    const int64_t bi = blockIdx.y;
    const int hw = h * w;
    for (int i = tid; i < hw; i += RO_THREADS) smap[i] = imp[bi * hw + i];
    __syncthreads();
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int y_lo = blockIdx.x * RO_MAP_ROWS, y_hi = min(H, y_lo + RO_MAP_ROWS);
    float *ob = out + bi * (int64_t)H * W;
    const int64_t cnt = (int64_t)(y_hi - y_lo) * W;
    for (int64_t e = tid; e < cnt; e += RO_THREADS) {
        const int y = y_lo + (int)(e / W), x = (int)(e % W);
        const float fy = fmaxf(sh * ((float)y + 0.5f) - 0.5f, 0.f);
        const float fx = fmaxf(sw * ((float)x + 0.5f) - 0.5f, 0.f);
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
        ob[(int64_t)y * W + x] = hy * (hx * smap[y0 * w + x0] + lx * smap[y0 * w + x1]) + ly * (hx * smap[y1 * w + x0] + lx * smap[y1 * w + x1]);
    }
}

// workspace layout (floats): [layers][b][n][n] matrices | [RO_HEAD_SPLIT][b][n][n] fused heads per split |
// [2][b][RO_SPLITS][n] chain partials | [b][n] importance
inline int64_t ws_mats(int layers, int64_t b, int64_t n) { return (int64_t)layers * b * n * n; }
inline int64_t ws_chain(int layers, int64_t b, int64_t n) { return ws_mats(layers, b, n) + (int64_t)RO_HEAD_SPLIT * b * n * n; }
inline int64_t ws_total(int layers, int64_t b, int64_t n) { return ws_chain(layers, b, n) + 2 * b * RO_SPLITS * n + b * n; }

}  // namespace

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

static int rollout_dims_ok(int layers, int64_t b, int64_t n) {
    return layers >= 1 && layers <= MIRX_ROLLOUT_MAX_LAYERS && b >= 0 && b <= MIRX_ROLLOUT_MAX_IMAGES && n >= 1 &&
           n <= MIRX_ROLLOUT_MAX_N;
}

extern "C" int64_t mirx_rollout_workspace_floats(int layers, int64_t b, int64_t n) {
    if (!rollout_dims_ok(layers, b, n))
        return fail(MIRX_EINVAL, "rollout_workspace_floats: layers must be in [1, 256], b in [0, 65535] and n in [1, 1024]");
    return ws_total(layers, b, n);
}

extern "C" int mirx_rollout_layer(const float *qkv, int64_t b, int n, int heads, int head_dim, float scale, int fusion, int k, int layer,
                                  int layers, float *workspace, int64_t workspace_floats, void *stream) {
    if (!rollout_dims_ok(layers, b, n)) return fail(MIRX_EINVAL, "rollout_layer: layers in [1, 256], b in [0, 65535], n in [1, 1024]");
    if (layer < 0 || layer >= layers) return fail(MIRX_EINVAL, "rollout_layer: layer must be in [0, layers)");
    if (heads < 1 || heads > MIRX_ROLLOUT_MAX_HEADS) return fail(MIRX_EINVAL, "rollout_layer: heads must be in [1, 256]");
    if (head_dim < 4 || head_dim > MIRX_ROLLOUT_MAX_HEAD_DIM || head_dim % 4 != 0)
        return fail(MIRX_EINVAL, "rollout_layer: head_dim must be a multiple of 4 in [4, 128]");
    if (fusion != MIRX_ROLLOUT_FUSE_MEAN && fusion != MIRX_ROLLOUT_FUSE_MAX && fusion != MIRX_ROLLOUT_FUSE_MIN)
        return fail(MIRX_EINVAL, "rollout_layer: fusion must be 0 (mean), 1 (max) or 2 (min)");
    if (k < 0 || k > n) return fail(MIRX_EINVAL, "rollout_layer: k must be in [0, n] (0: no discard)");
    if (!(scale == scale) || std::isinf(scale)) return fail(MIRX_EINVAL, "rollout_layer: scale must be finite");
    if (b == 0) return MIRX_OK;
    if (!qkv || !workspace) return fail(MIRX_EINVAL, "rollout_layer: null buffer");
    if (reinterpret_cast<uintptr_t>(qkv) % 16 != 0) return fail(MIRX_EINVAL, "rollout_layer: qkv must be 16-byte aligned");
    if (workspace_floats < ws_total(layers, b, n))
        return fail(MIRX_EINVAL, "rollout_layer: workspace smaller than mirx_rollout_workspace_floats()");
    const int splits = std::min(heads, RO_HEAD_SPLIT);
    LayerArgs la{};
    la.qkv = qkv;
    la.n = n;
    la.heads = heads;
    la.dh = head_dim;
    la.hper = (heads + splits - 1) / splits;
    la.c = (int64_t)heads * head_dim;
    la.b = b;
    la.scale = scale;
    la.fusion = fusion;
    la.part = workspace + ws_mats(layers, b, n);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + RO_ROWS - 1) / RO_ROWS), (unsigned)((heads + la.hper - 1) / la.hper), (unsigned)b);
    if (head_dim == 72) hipLaunchKernelGGL(k_rollout_layer<72>, grid, dim3(RO_THREADS), 0, st, la);
    else if (head_dim == 64) hipLaunchKernelGGL(k_rollout_layer<64>, grid, dim3(RO_THREADS), 0, st, la);
    else hipLaunchKernelGGL(k_rollout_layer<0>, grid, dim3(RO_THREADS), 0, st, la);
    MIRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rollout_combine, dim3((unsigned)((n + 3) / 4), (unsigned)b), dim3(RO_THREADS), 0, st, la.part, (int)grid.y, b, n,
                       heads, fusion, k, workspace + (int64_t)layer * b * n * n);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_rollout_rows(float *a, int64_t rows, int n, int k, void *stream) {
    if (rows < 0 || rows > MIRX_ROLLOUT_MAX_ROWS) return fail(MIRX_EINVAL, "rollout_rows: rows must be in [0, 2^26]");
    if (n < 1 || n > MIRX_ROLLOUT_MAX_N) return fail(MIRX_EINVAL, "rollout_rows: n must be in [1, 1024]");
    if (k < 0 || k > n) return fail(MIRX_EINVAL, "rollout_rows: k must be in [0, n] (0: no discard)");
    if (rows == 0) return MIRX_OK;
    if (!a) return fail(MIRX_EINVAL, "rollout_rows: null buffer");
    hipLaunchKernelGGL(k_rollout_rows, dim3((unsigned)((rows + 3) / 4)), dim3(RO_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
                       rows, n, k);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_rollout_finish(float *workspace, int64_t workspace_floats, int layers, int64_t b, int h, int w, const float *patches,
                                   const float *query, int64_t e, int H, int W, float *out, void *stream) {
    const int64_t n = (int64_t)h * w;
    if (h < 1 || w < 1 || !rollout_dims_ok(layers, b, n))
        return fail(MIRX_EINVAL, "rollout_finish: layers in [1, 256], b in [0, 65535], h, w >= 1 and h * w <= 1024");
    if (H < 1 || W < 1 || H > MIRX_ROLLOUT_MAX_SIZE || W > MIRX_ROLLOUT_MAX_SIZE)
        return fail(MIRX_EINVAL, "rollout_finish: H, W must be in [1, 8192]");
    if ((patches == nullptr) != (query == nullptr)) return fail(MIRX_EINVAL, "rollout_finish: patches and query go together");
    if (patches && (e < 1 || e > MIRX_ROLLOUT_MAX_EMBED)) return fail(MIRX_EINVAL, "rollout_finish: e must be in [1, 65536]");
    if (b == 0) return MIRX_OK;
    if (!workspace || !out) return fail(MIRX_EINVAL, "rollout_finish: null buffer");
    if (workspace_floats < ws_total(layers, b, n))
        return fail(MIRX_EINVAL, "rollout_finish: workspace smaller than mirx_rollout_workspace_floats()");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *part = workspace + ws_chain(layers, b, n);
    const int64_t pstride = b * RO_SPLITS * n;
    float *imp = part + 2 * pstride;
    for (int s = 0; s < layers; ++s) {
        const int l = layers - 1 - s;
        hipLaunchKernelGGL(k_rollout_chain, dim3((unsigned)((n + 63) / 64), RO_SPLITS, (unsigned)b), dim3(RO_THREADS), 0, st,
                           workspace + (int64_t)l * b * n * n, part + (s & 1) * pstride, part + ((s + 1) & 1) * pstride, (int)n,
                           s == 0 ? 1 : 0);
        MIRX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rollout_importance, dim3((unsigned)((n + 3) / 4), (unsigned)b), dim3(RO_THREADS), 0, st,
                       part + (layers & 1) * pstride, patches, query, e, (int)n, imp);
    MIRX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rollout_upsample, dim3((unsigned)((H + RO_MAP_ROWS - 1) / RO_MAP_ROWS), (unsigned)b), dim3(RO_THREADS), 0, st, imp,
                       h, w, H, W, out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}
