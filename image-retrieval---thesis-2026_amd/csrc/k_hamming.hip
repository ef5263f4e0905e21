// k_hamming.hip -- exact Hamming top-k over bit-packed binary codes (mirx_hamming_* of include/mirx.h).
//
// Codes are packed into WP 32-bit words per row (WP = 1, 2, 4, ..., 32, the padding words zero in queries and rows alike, so they
// add nothing to a distance).  The ranking is (distance ascending, row ascending); one id per query may be excluded.  Passes:
//
//   sample   a workgroup per query: an LDS histogram of the distances of a strided sample of ns rows (ns >= min(N, 4096, 4 k));
//            tau[q] = the k-th smallest sampled distance (bits when the sample holds fewer than k rows).  The sample is a subset of
//            the gallery, so tau >= d*, the true k-th distance.  Also zeroes the query's global histogram and its k-slot row.
//   count    each wave owns a slice of L consecutive rows (a lane per row, the row's words in registers) and QT queries of a
//            tile (their words wave-uniform in LDS): d = sum popcount(g ^ q), and only rows with d <= tau bump a per-(query, bin)
//            LDS count; the workgroup then adds its nonzero bins to hist[q][d].  Integer adds commute: the histogram is exact
//            whatever the order of the atomics.
//   select   a wave per query: d* = the smallest d with sum_{e <= d} hist[q][e] >= k, below = that sum before d*, m = k - below
//            (the rows taken at d*).  (With an exclusion, k = N can leave fewer than k rows: then every row is "below".)
//   slices   per (query, slice): below_s = #(d < d*), at_s = #(d == d*) from wave ballots; no atomics.
//   scan     a wave per query: exclusive prefix sums of below_s and at_s over the slices (in slice = row order).
//   emit     per (query, slice), skipped when the slice holds nothing to emit: rows with d < d* go to slot off_below + their in-slice
//            rank; rows at d* have global in-order rank r = off_at + in-slice rank and go to slot below + r when r < m.  Every slot
//            is decided by row order alone, so the k slots hold exactly the rows of the exact ranking.
//   sort     a workgroup per query: bitonic sort of the k keys (d << 32 | row) in LDS.
//
// Workspace: Q * (bits + 1) + Q * 2 (S + 1) + 4 Q ints and Q * kp keys (kp = next power of two >= k), S = ceil(N / L): bounded by Q,
// N, k and bits, never by how the distances are spread (a gallery at distance 0 from every query costs what any other does).
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int HM_THREADS = 256;
constexpr int HM_TARGET_WAVES = 16384;     // count / slices / emit grid: about 64 waves per CU
constexpr unsigned long long HM_SENTINEL = ~0ull;

__device__ inline int lanemask_rank(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

__device__ inline int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

template <int WP>
__device__ inline void load_row(const uint32_t *__restrict__ p, uint32_t (&g)[WP]) {
    if constexpr (WP >= 4) {
        const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int i = 0; i < WP / 4; ++i) {
            const uint4 v = p4[i];
            g[4 * i] = v.x;
            g[4 * i + 1] = v.y;
            g[4 * i + 2] = v.z;
            g[4 * i + 3] = v.w;
        }
    } else if constexpr (WP == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        g[0] = v.x;
        g[1] = v.y;
    } else {
        g[0] = p[0];
    }
}

template <int WP>
__device__ inline int hdist(const uint32_t (&g)[WP], const uint32_t *q) {
    int d = 0;
#pragma unroll
    for (int w = 0; w < WP; ++w) d += __popc(g[w] ^ q[w]);
    return d;
}

// ---- pack: src [rows, bits] (float32 or bytes) -> dst [rows, wp] words; bad <- 1 on any value other than 0 / 1 ----
template <typename T>
__global__ __launch_bounds__(HM_THREADS) void k_ham_pack(const T *__restrict__ src, int64_t rows, int bits, int wp,
                                                         uint32_t *__restrict__ dst, int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * HM_THREADS + threadIdx.x;
    if (i >= rows * wp) return;
    const int64_t r = i / wp;
    const int w = (int)(i - r * wp);
    const T *s = src + r * bits;
    uint32_t word = 0;
    bool ok = true;
    for (int j = 0; j < 32; ++j) {
        const int b = 32 * w + j;
        if (b >= bits) break;
        const T v = s[b];
        if (v == T(1)) word |= 1u << j;
        else if (!(v == T(0))) ok = false;            // NaN lands here as well
    }
    dst[i] = word;
    if (!ok) *bad = 1;                                // every writer stores the same value
}

// ---- sample: tau[q]; also zeroes hist[q] and fills keys[q] with the sentinel ----
template <int WP>
__global__ __launch_bounds__(HM_THREADS) void k_ham_sample(const uint32_t *__restrict__ qp, const uint32_t *__restrict__ gp, int64_t N,
                                                           int bits, int k, const int64_t *__restrict__ ex, int64_t ns,
                                                           int *__restrict__ tau, int *__restrict__ hist,
                                                           unsigned long long *__restrict__ keys, int kp) {
    __shared__ int lh[MIRX_HAMMING_MAX_BITS + 1];
    __shared__ uint32_t sq[WP];
    const int q = blockIdx.x, tid = threadIdx.x;
    for (int d = tid; d <= bits; d += HM_THREADS) {
        lh[d] = 0;
        hist[(int64_t)q * (bits + 1) + d] = 0;
    }
    for (int j = tid; j < kp; j += HM_THREADS) keys[(int64_t)q * kp + j] = HM_SENTINEL;
    if (tid < WP) sq[tid] = qp[(int64_t)q * WP + tid];
    __syncthreads();
    const int64_t exq = ex ? ex[q] : -1;
    for (int64_t j = tid; j < ns; j += HM_THREADS) {
        const int64_t r = j * N / ns;
        if (r == exq) continue;
        uint32_t g[WP];
        load_row<WP>(gp + r * WP, g);
        atomicAdd(&lh[hdist<WP>(g, sq)], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int c = 0, t = bits;
        for (int d = 0; d <= bits; ++d) {
            c += lh[d];
            if (c >= k) {
                t = d;
                break;
            }
        }
        tau[q] = t;
    }
}

// a workgroup = 4 waves = 4 slices of L rows, one tile of QT queries.  Block b: tile b / sg, slices 4 (b % sg) .. + 3.
template <int WP, int QT>
struct TileCtx {
    int tile, s, q0, nq;
};

template <int WP, int QT>
__device__ inline TileCtx<WP, QT> tile_ctx(int64_t Q, int64_t sg) {
    TileCtx<WP, QT> c;
    c.tile = (int)(blockIdx.x / sg);
    c.s = (int)(blockIdx.x % sg) * 4 + (threadIdx.x >> 6);
    c.q0 = c.tile * QT;
    c.nq = (int)((Q - c.q0) < QT ? (Q - c.q0) : QT);
    return c;
}

// ---- count: hist[q][d] += #rows of the slices with d <= tau[q] ----
template <int WP, int QT>
__global__ __launch_bounds__(HM_THREADS) void k_ham_count(const uint32_t *__restrict__ qp, const uint32_t *__restrict__ gp, int64_t Q,
                                                          int64_t N, int bits, const int64_t *__restrict__ ex, const int *__restrict__ tau,
                                                          int64_t L, int64_t S, int64_t sg, int *__restrict__ hist) {
    extern __shared__ int lh[];                   // [QT][bits + 1]
    __shared__ uint32_t sq[QT][WP];
    __shared__ int st[QT];
    __shared__ int64_t sx[QT];
    const auto c = tile_ctx<WP, QT>(Q, sg);
    const int tid = threadIdx.x, lane = tid & 63, nb = bits + 1;
    for (int i = tid; i < QT * nb; i += HM_THREADS) lh[i] = 0;
    for (int i = tid; i < QT * WP; i += HM_THREADS) {
        const int qi = i / WP;
        sq[qi][i % WP] = qi < c.nq ? qp[(int64_t)(c.q0 + qi) * WP + i % WP] : 0u;
    }
    if (tid < QT) {
        st[tid] = tid < c.nq ? tau[c.q0 + tid] : -1;            // -1: no row passes
        sx[tid] = tid < c.nq && ex ? ex[c.q0 + tid] : -1;
    }
    __syncthreads();
    if (c.s < S) {
        const int64_t r0 = c.s * L, r1 = (r0 + L < N) ? r0 + L : N;
        for (int64_t base = r0; base < r1; base += 64) {
            const int64_t r = base + lane;
            if (r >= r1) break;
            uint32_t g[WP];
            load_row<WP>(gp + r * WP, g);
#pragma unroll 4
            for (int qi = 0; qi < QT; ++qi) {
                const int d = hdist<WP>(g, sq[qi]);
                if (d <= st[qi] && r != sx[qi]) atomicAdd(&lh[qi * nb + d], 1);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < QT * nb; i += HM_THREADS) {
        const int v = lh[i];
        const int qi = i / nb;
        if (v && qi < c.nq) atomicAdd(&hist[(int64_t)(c.q0 + qi) * nb + (i - qi * nb)], v);
    }
}

// ---- select: a wave per query -> sel[q] = {d*, below, m} ----
__global__ __launch_bounds__(HM_THREADS) void k_ham_select(const int *__restrict__ hist, int64_t Q, int bits, int k,
                                                           const int *__restrict__ tau, int *__restrict__ sel) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int lane = threadIdx.x & 63, nb = bits + 1, t = tau[q];
    const int *h = hist + q * nb;
    int run = 0;                                  // rows with d below the current chunk
    for (int d0 = 0; d0 <= t; d0 += 64) {
        const int d = d0 + lane;
        const int v = d <= t ? h[d] : 0;
        const int inc = wave_incl_scan(v) + run;
        const unsigned long long hit = __ballot(inc >= k);
        if (hit) {
            const int first = __builtin_ctzll(hit);
            const int ds = __shfl(d, first, 64), incl = __shfl(inc, first, 64), here = __shfl(v, first, 64);
            if (lane == 0) {
                sel[q * 3] = ds;
                sel[q * 3 + 1] = incl - here;
                sel[q * 3 + 2] = k - (incl - here);
            }
            return;
        }
        run = __shfl(inc, 63, 64);
    }
    if (lane == 0) {                              // fewer than k rows exist (an excluded row and k = N): every row is "below"
        sel[q * 3] = bits + 1;
        sel[q * 3 + 1] = run;
        sel[q * 3 + 2] = 0;
    }
}

// ---- slices: cnt[q][s] = {#(d < d*), #(d == d*)} ----
template <int WP, int QT>
__global__ __launch_bounds__(HM_THREADS) void k_ham_slices(const uint32_t *__restrict__ qp, const uint32_t *__restrict__ gp, int64_t Q,
                                                           int64_t N, const int64_t *__restrict__ ex, const int *__restrict__ sel,
                                                           int64_t L, int64_t S, int64_t sg, int *__restrict__ cnt) {
    __shared__ uint32_t sq[QT][WP];
    __shared__ int sd[QT];
    __shared__ int64_t sx[QT];
    const auto c = tile_ctx<WP, QT>(Q, sg);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < QT * WP; i += HM_THREADS) {
        const int qi = i / WP;
        sq[qi][i % WP] = qi < c.nq ? qp[(int64_t)(c.q0 + qi) * WP + i % WP] : 0u;
    }
    if (tid < QT) {
        sd[tid] = tid < c.nq ? sel[(int64_t)(c.q0 + tid) * 3] : -1;
        sx[tid] = tid < c.nq && ex ? ex[c.q0 + tid] : -1;
    }
    __syncthreads();
    if (c.s >= S) return;
    int nbelow[QT], nat[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) nbelow[qi] = nat[qi] = 0;
    const int64_t r0 = c.s * L, r1 = (r0 + L < N) ? r0 + L : N;
    for (int64_t base = r0; base < r1; base += 64) {
        const int64_t r = base + lane;
        const bool valid = r < r1;
        uint32_t g[WP];
        if (valid) load_row<WP>(gp + r * WP, g);
        else {
#pragma unroll
            for (int w = 0; w < WP; ++w) g[w] = 0;
        }
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            const int d = hdist<WP>(g, sq[qi]);
            const bool ok = valid && r != sx[qi];
            nbelow[qi] += __popcll(__ballot(ok && d < sd[qi]));
            nat[qi] += __popcll(__ballot(ok && d == sd[qi]));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            if (qi < c.nq) {
                int *o = cnt + ((int64_t)(c.q0 + qi) * (S + 1) + c.s) * 2;
                o[0] = nbelow[qi];
                o[1] = nat[qi];
            }
        }
    }
}

// ---- scan: a wave per query, exclusive prefix sums over the S slices in place; entry S holds the totals ----
__global__ __launch_bounds__(HM_THREADS) void k_ham_scan(int *__restrict__ cnt, int64_t Q, int64_t S) {
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    const int lane = threadIdx.x & 63;
    int *c = cnt + q * (S + 1) * 2;
    int rb = 0, ra = 0;
    for (int64_t s0 = 0; s0 < S; s0 += 64) {
        const int64_t s = s0 + lane;
        const int b = s < S ? c[2 * s] : 0, a = s < S ? c[2 * s + 1] : 0;
        const int ib = wave_incl_scan(b), ia = wave_incl_scan(a);
        if (s < S) {
            c[2 * s] = rb + ib - b;
            c[2 * s + 1] = ra + ia - a;
        }
        rb += __shfl(ib, 63, 64);
        ra += __shfl(ia, 63, 64);
    }
    if (lane == 0) {
        c[2 * S] = rb;
        c[2 * S + 1] = ra;
    }
}

// ---- emit: the k rows into their slots ----
template <int WP, int QT>
__global__ __launch_bounds__(HM_THREADS) void k_ham_emit(const uint32_t *__restrict__ qp, const uint32_t *__restrict__ gp, int64_t Q,
                                                         int64_t N, const int64_t *__restrict__ ex, const int *__restrict__ sel,
                                                         const int *__restrict__ cnt, int64_t L, int64_t S, int64_t sg,
                                                         unsigned long long *__restrict__ keys, int kp) {
    __shared__ uint32_t sq[QT][WP];
    __shared__ int64_t sx[QT];
    const auto c = tile_ctx<WP, QT>(Q, sg);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < QT * WP; i += HM_THREADS) {
        const int qi = i / WP;
        sq[qi][i % WP] = qi < c.nq ? qp[(int64_t)(c.q0 + qi) * WP + i % WP] : 0u;
    }
    if (tid < QT) sx[tid] = tid < c.nq && ex ? ex[c.q0 + tid] : -1;
    __syncthreads();
    if (c.s >= S) return;
    const int64_t r0 = c.s * L, r1 = (r0 + L < N) ? r0 + L : N;
    for (int qi = 0; qi < c.nq; ++qi) {
        const int64_t q = c.q0 + qi;
        const int ds = sel[q * 3], below = sel[q * 3 + 1], m = sel[q * 3 + 2];
        const int *cs = cnt + (q * (S + 1) + c.s) * 2;
        int ob = cs[0], oa = cs[1];
        const int nb = cs[2] - ob, na = cs[3] - oa;
        if (nb == 0 && (na == 0 || oa >= m)) continue;                      // nothing of this query in this slice
        unsigned long long *kq = keys + q * kp;
        for (int64_t base = r0; base < r1; base += 64) {
            const int64_t r = base + lane;
            const bool valid = r < r1 && r != sx[qi];
            uint32_t g[WP];
            if (r < r1) load_row<WP>(gp + r * WP, g);
            else {
#pragma unroll
                for (int w = 0; w < WP; ++w) g[w] = 0;
            }
            const int d = hdist<WP>(g, sq[qi]);
            const bool pb = valid && d < ds, pa = valid && d == ds;
            const unsigned long long bb = __ballot(pb), ba = __ballot(pa);
            const unsigned long long key = ((unsigned long long)(unsigned)d << 32) | (unsigned long long)r;
            if (pb) kq[ob + lanemask_rank(bb)] = key;
            if (pa) {
                const int rank = oa + lanemask_rank(ba);
                if (rank < m) kq[below + rank] = key;
            }
            ob += __popcll(bb);
            oa += __popcll(ba);
        }
    }
}

// ---- sort: a workgroup per query, bitonic over kp <= 1024 keys; the first k out ----
__global__ __launch_bounds__(HM_THREADS) void k_ham_sort(const unsigned long long *__restrict__ keys, int kp, int k,
                                                         int *__restrict__ dist, int64_t *__restrict__ ids) {
    __shared__ unsigned long long sk[MIRX_HAMMING_MAX_K];
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < kp; i += HM_THREADS) sk[i] = keys[q * kp + i];
    __syncthreads();
    for (int size = 2; size <= kp; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < kp; i += HM_THREADS) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool up = (i & size) == 0;
                    const unsigned long long a = sk[i], b = sk[j];
                    if ((a > b) == up) {
                        sk[i] = b;
                        sk[j] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += HM_THREADS) {
        const unsigned long long v = sk[i];
        dist[q * k + i] = v == HM_SENTINEL ? -1 : (int)(v >> 32);
        ids[q * k + i] = v == HM_SENTINEL ? -1 : (int64_t)(v & 0xffffffffull);
    }
}

struct HamPlan {
    int wp, qt, kp;
    int64_t L, S, sg, tiles, ns;
    // workspace layout (bytes from the base)
    int64_t o_tau, o_sel, o_hist, o_cnt, o_keys, bytes;
};

inline int64_t rup(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

HamPlan ham_plan(int64_t Q, int64_t N, int bits, int k) {
    HamPlan p;
    const int w = (bits + 31) / 32;
    p.wp = 1;
    while (p.wp < w) p.wp <<= 1;
    p.qt = bits <= 512 ? 16 : 8;
    p.kp = 1;
    while (p.kp < k) p.kp <<= 1;
    p.tiles = (Q + p.qt - 1) / p.qt;
    const int64_t s_target = (HM_TARGET_WAVES + (p.tiles > 0 ? p.tiles : 1) - 1) / (p.tiles > 0 ? p.tiles : 1);
    p.L = rup((N + s_target - 1) / s_target, 64);
    if (p.L < 256) p.L = 256;
    p.S = (N + p.L - 1) / p.L;
    p.sg = (p.S + 3) / 4;
    p.ns = N < 4096 ? N : 4096;
    if (p.ns < 4 * (int64_t)k) p.ns = N < 4 * (int64_t)k ? N : 4 * (int64_t)k;
    p.o_tau = 0;
    p.o_sel = rup(p.o_tau + 4 * Q, 256);
    p.o_hist = rup(p.o_sel + 12 * Q, 256);
    p.o_cnt = rup(p.o_hist + 4 * Q * (bits + 1), 256);
    p.o_keys = rup(p.o_cnt + 8 * Q * (p.S + 1), 256);
    p.bytes = rup(p.o_keys + 8 * Q * (int64_t)p.kp, 256);
    return p;
}

template <int WP, int QT>
hipError_t launch_ham_passes(const HamPlan &p, const uint32_t *qp, const uint32_t *gp, int64_t Q, int64_t N, int bits, int k,
                             const int64_t *ex, char *ws, int *dist, int64_t *ids, hipStream_t st) {
    int *tau = reinterpret_cast<int *>(ws + p.o_tau);
    int *sel = reinterpret_cast<int *>(ws + p.o_sel);
    int *hist = reinterpret_cast<int *>(ws + p.o_hist);
    int *cnt = reinterpret_cast<int *>(ws + p.o_cnt);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + p.o_keys);
    const dim3 blk(HM_THREADS);
    const unsigned qwaves = (unsigned)((Q + 3) / 4);
    const unsigned tiled = (unsigned)(p.tiles * p.sg);
    hipLaunchKernelGGL((k_ham_sample<WP>), dim3((unsigned)Q), blk, 0, st, qp, gp, N, bits, k, ex, p.ns, tau, hist, keys, p.kp);
    const size_t lds = (size_t)QT * (bits + 1) * sizeof(int);
    hipLaunchKernelGGL((k_ham_count<WP, QT>), dim3(tiled), blk, lds, st, qp, gp, Q, N, bits, ex, tau, p.L, p.S, p.sg, hist);
    hipLaunchKernelGGL(k_ham_select, dim3(qwaves), blk, 0, st, hist, Q, bits, k, tau, sel);
    hipLaunchKernelGGL((k_ham_slices<WP, QT>), dim3(tiled), blk, 0, st, qp, gp, Q, N, ex, sel, p.L, p.S, p.sg, cnt);
    hipLaunchKernelGGL(k_ham_scan, dim3(qwaves), blk, 0, st, cnt, Q, p.S);
    hipLaunchKernelGGL((k_ham_emit<WP, QT>), dim3(tiled), blk, 0, st, qp, gp, Q, N, ex, sel, cnt, p.L, p.S, p.sg, keys, p.kp);
    hipLaunchKernelGGL(k_ham_sort, dim3((unsigned)Q), blk, 0, st, keys, p.kp, k, dist, ids);
    return hipGetLastError();
}

const char *ham_args_error(int64_t Q, int64_t N, int bits, int k) {
    if (bits < 1 || bits > MIRX_HAMMING_MAX_BITS) return "bits must be in [1, 1024]";
    if (k < 1 || k > MIRX_HAMMING_MAX_K) return "k must be in [1, 1024]";
    if (Q < 0 || Q > MIRX_HAMMING_MAX_Q) return "nq must be in [0, 2^24]";
    if (N < 1 || N > 0x7fffffffLL) return "n must be in [1, 2^31 - 1]";
    if (k > N) return "k must not exceed the gallery rows";
    return nullptr;
}

}  // namespace

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

extern "C" int mirx_hamming_words(int bits) {
    if (bits < 1 || bits > MIRX_HAMMING_MAX_BITS) return fail(MIRX_EINVAL, "hamming_words: bits must be in [1, 1024]");
    return ham_plan(1, 1, bits, 1).wp;
}

extern "C" int mirx_hamming_pack(const void *src, int dtype, int64_t rows, int bits, uint32_t *dst, int *bad_flag, void *stream) {
    if (bits < 1 || bits > MIRX_HAMMING_MAX_BITS) return fail(MIRX_EINVAL, "hamming_pack: bits must be in [1, 1024]");
    if (rows < 0 || rows > 0x7fffffffLL) return fail(MIRX_EINVAL, "hamming_pack: rows must be in [0, 2^31 - 1]");
    if (dtype != MIRX_BITS_F32 && dtype != MIRX_BITS_U8) return fail(MIRX_EINVAL, "hamming_pack: dtype must be MIRX_BITS_F32 or MIRX_BITS_U8");
    if (rows == 0) return MIRX_OK;
    if (!src || !dst || !bad_flag) return fail(MIRX_EINVAL, "hamming_pack: null buffer");
    if (dtype == MIRX_BITS_F32 && (uintptr_t)src % 4) return fail(MIRX_EINVAL, "hamming_pack: float32 src must be 4-byte aligned");
    if ((uintptr_t)dst % 16) return fail(MIRX_EINVAL, "hamming_pack: dst must be 16-byte aligned");
    const int wp = ham_plan(1, 1, bits, 1).wp;
    const int64_t total = rows * wp;
    const dim3 grid((unsigned)((total + HM_THREADS - 1) / HM_THREADS)), blk(HM_THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MIRX_BITS_F32)
        hipLaunchKernelGGL(k_ham_pack<float>, grid, blk, 0, st, static_cast<const float *>(src), rows, bits, wp, dst, bad_flag);
    else
        hipLaunchKernelGGL(k_ham_pack<uint8_t>, grid, blk, 0, st, static_cast<const uint8_t *>(src), rows, bits, wp, dst, bad_flag);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int64_t mirx_hamming_workspace_bytes(int64_t nq, int64_t n, int bits, int k) {
    const char *why = ham_args_error(nq, n, bits, k);
    if (why) return fail(MIRX_EINVAL, std::string("hamming_workspace_bytes: ") + why);
    return ham_plan(nq, n, bits, k).bytes;
}

extern "C" int mirx_hamming_topk(const uint32_t *q_packed, int64_t nq, const uint32_t *g_packed, int64_t n, int bits, int k,
                                 const int64_t *exclude_or_null, void *workspace, int64_t workspace_bytes, int *out_dist,
                                 int64_t *out_ids, void *stream) {
    const char *why = ham_args_error(nq, n, bits, k);
    if (why) return fail(MIRX_EINVAL, std::string("hamming_topk: ") + why);
    if (nq == 0) return MIRX_OK;
    const HamPlan p = ham_plan(nq, n, bits, k);
    if (!q_packed || !g_packed || !workspace || !out_dist || !out_ids) return fail(MIRX_EINVAL, "hamming_topk: null buffer");
    if (workspace_bytes < p.bytes) return fail(MIRX_EINVAL, "hamming_topk: workspace smaller than mirx_hamming_workspace_bytes()");
    if (((uintptr_t)q_packed | (uintptr_t)g_packed | (uintptr_t)workspace) % 16)
        return fail(MIRX_EINVAL, "hamming_topk: packed codes and workspace must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
#define MIRX_HAM(WP)                                                                                                                \
    (p.qt == 16 ? launch_ham_passes<WP, 16>(p, q_packed, g_packed, nq, n, bits, k, exclude_or_null, ws, out_dist, out_ids, st)     \
                : launch_ham_passes<WP, 8>(p, q_packed, g_packed, nq, n, bits, k, exclude_or_null, ws, out_dist, out_ids, st))
    hipError_t e;
    switch (p.wp) {
    case 1: e = MIRX_HAM(1); break;
    case 2: e = MIRX_HAM(2); break;
    case 4: e = MIRX_HAM(4); break;
    case 8: e = MIRX_HAM(8); break;
    case 16: e = MIRX_HAM(16); break;
    default: e = launch_ham_passes<32, 8>(p, q_packed, g_packed, nq, n, bits, k, exclude_or_null, ws, out_dist, out_ids, st); break;
    }
#undef MIRX_HAM
    MIRX_HIP(e);
    return MIRX_OK;
}
