// k_anomaly.hip -- anomaly evaluation on the device (gfx950, wave64): class centroids of an embedding set, every row's distance
// to its nearest centroid, and the binary ranking metrics (AUROC, AUPR, FPR at a recall level, the ROC / PR curve points) of
// score segments.  DESIGN 25.
//
// Reference behaviour replaced (paths into the reference's anomaly/):
//   centroids   test_anomaly.py:31-32   embeds[labels == c].mean(axis=0)
//   distances   test_anomaly.py:46-48   cdist(test, centroids).min(axis=1), then / max
//   metrics     anomaly.py:27-81        roc_auc_score, average_precision_score, fpr_and_fdr_at_recall; test_anomaly.py:60-61
//                                       roc_curve, precision_recall_curve
//
// 1. Centroids.  The rows are cut into chunks of an_chunk_rows(n, d) consecutive rows (a function of n and d alone).  A
//    workgroup owns (chunk, 256 columns): each thread adds its column's values, in row order, into one fp64 accumulator per
//    class kept in LDS, and stores them as the chunk's partial sums.  A second launch adds the partials in chunk order and
//    divides by the class count.  No floating atomic anywhere: the bits of a centroid depend on the inputs alone.  The centroid
//    stays fp64 (numpy's mean of an fp32 array rounds it to fp32; this does not).
// 2. Min distance.  A wave per row, lanes stride the row with 16-byte loads (4-byte loads when d % 4 != 0 or the rows are not
//    16-byte aligned), (x - c)^2 accumulated in fp64 for one, two or four centroids at a time (k = 1, k = 2, k >= 3; k <= 4: the row
//    is read once; above, once per four classes, from the cache), a butterfly sum, sqrt, strict < so that the lowest class wins
//    a tie; a NaN distance of any class makes the row's minimum NaN.  Centroids sit in LDS
//    while k * d * 8 <= 64 KiB, else they are read through L2.  The maximum goes through an unsigned 64-bit atomic max on the
//    bit pattern (sign bit cleared): distances are >= 0, whose patterns order like the values, so the result does not depend
//    on arrival order (a NaN has the largest pattern and wins: loud).
// 3. Binary ranking metrics of nseg segments of n (score, positive) pairs:
//      k_bm_build    keys = rank_key(score / norm), payload = position            flags a non-finite score, a bad norm
//      launch_rank_sort (k_ranksort.hip)                                          ascending key = descending score
//      k_bm_count    per RANK_TILE tile: positives (gathered through the payload) and group ends (key != next key)
//      k_bm_scan     per segment: exclusive scan of both over the tiles; P, T      flags a segment without positives / negatives
//      k_bm_compact  per tile: one record (threshold, tps, fps) per distinct score at its place among the segment's T
//      k_bm_reduce   per segment: AUROC (int64 trapezoid sum, one division), AUPR, FPR at the recall level
//    Launch boundaries are the only synchronisation between workgroups, as in the sort.
//    NOTHING DEPENDS ON THE ORDER OF EQUAL SCORES: a record is written at a group's last element, its tps is the count of
//    positives up to there, which is the same for every order inside the groups; every output is a function of the groups.
//    FPR at recall reproduces anomaly.py:59-67: last_ind = the first record with tps == P; among the records 0 .. last_ind the
//    one whose |tps / P - level| is smallest, the LATER record on a tie (the reference searches the reversed slice and takes
//    the first minimum; its appended (recall 1, fps 0) point ties with record last_ind and comes after it, so it never wins).
//    AUPR adds per-thread strided partial sums and combines them in a fixed tree: an order fixed by T alone, so a segment's
//    bits do not depend on how many segments the call carries.
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

#include <algorithm>

namespace mirx {

namespace {

constexpr int AN_THREADS = 256;
constexpr int AN_WAVES = AN_THREADS / WAVE;
constexpr int AN_MD_LDS_BYTES = 64 * 1024;                   // centroids staged in LDS up to here
constexpr int BM_ROWS = RANK_TILE / AN_THREADS;              // 64-element rows per wave of a tile
constexpr int BM_RTHREADS = 1024;
static_assert(RANK_TILE == AN_WAVES * BM_ROWS * WAVE, "a tile is AN_WAVES chunks of BM_ROWS rows of 64 elements");

struct ClassList {
    int64_t v[MIRX_ANOMALY_MAX_K];
};

// ---- 1. centroids -----------------------------------------------------------------------------------------------------------
// class index (or -1) of every row, and the chunk's class counts
__global__ __launch_bounds__(AN_THREADS) void k_an_classify(const int64_t *__restrict__ labels, int64_t n, int64_t chunk_rows,
                                                            ClassList cl, int k, int32_t *__restrict__ cls,
                                                            unsigned *__restrict__ cnt_part) {
    __shared__ unsigned c[MIRX_ANOMALY_MAX_K];
    if (threadIdx.x < MIRX_ANOMALY_MAX_K) c[threadIdx.x] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * chunk_rows;
    const int64_t r1 = std::min<int64_t>(n, r0 + chunk_rows);
    for (int64_t r = r0 + threadIdx.x; r < r1; r += AN_THREADS) {
        const int64_t lab = labels[r];
        int idx = -1;
        for (int j = k - 1; j >= 0; --j) idx = cl.v[j] == lab ? j : idx;        // the first class that matches
        cls[r] = idx;
        if (idx >= 0) atomicAdd(&c[idx], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < k) cnt_part[(int64_t)blockIdx.x * k + threadIdx.x] = c[threadIdx.x];
}

// partial[chunk][class][col] = the sum, in row order, of the chunk's rows of that class; grid (chunks, ceil(d / 256))
__global__ __launch_bounds__(AN_THREADS) void k_an_partial(const float *__restrict__ rows, int64_t n, int d, int64_t chunk_rows,
                                                           const int32_t *__restrict__ cls, int k, double *__restrict__ partial) {
    extern __shared__ double an_acc[];                         // [k][256]; a thread touches its own column only: no barrier
    const int t = threadIdx.x;
    const int col = blockIdx.y * AN_THREADS + t;
    for (int j = 0; j < k; ++j) an_acc[j * AN_THREADS + t] = 0.0;
    if (col >= d) return;
    const int64_t r0 = (int64_t)blockIdx.x * chunk_rows;
    const int64_t r1 = std::min<int64_t>(n, r0 + chunk_rows);
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {                              // four loads in flight, added in row order
        float x[4];
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x[u] = rows[(r + u) * d + col];
            c[u] = cls[r + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if ((unsigned)c[u] < (unsigned)k) an_acc[c[u] * AN_THREADS + t] += (double)x[u];
    }
    for (; r < r1; ++r) {
        const int c = cls[r];
        if ((unsigned)c < (unsigned)k) an_acc[c * AN_THREADS + t] += (double)rows[r * d + col];
    }
    for (int j = 0; j < k; ++j) partial[((int64_t)blockIdx.x * k + j) * d + col] = an_acc[j * AN_THREADS + t];
}

// centroid[class][col] = (partials in chunk order) / count
__global__ __launch_bounds__(AN_THREADS) void k_an_reduce(const double *__restrict__ partial, const unsigned *__restrict__ cnt_part,
                                                          int64_t nchunks, int k, int d, double *__restrict__ centroids,
                                                          int64_t *__restrict__ counts, int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= (int64_t)k * d) return;
    const int j = (int)(i / d), col = (int)(i % d);
    int64_t cnt = 0;
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) {
        cnt += cnt_part[c * k + j];
        s += partial[(c * k + j) * d + col];
    }
    centroids[i] = s / (double)cnt;                            // an empty class: 0 / 0 = NaN, and the flag
    if (col == 0) {
        counts[j] = cnt;
        if (cnt == 0) atomicOr(bad, MIRX_ANOMALY_BAD_EMPTY_CLASS);
    }
}

// ---- 2. min distance --------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) double f64x2;

// NC = classes per pass over the row: 1, 2 or 4 (k = 1, k = 2, k >= 3: no accumulator is computed for nothing at the driver's
// k = 2).  VEC && IN_LDS: the staged copy of centroid j keeps elements 4q, 4q + 1 of every quad q first and 4q + 2, 4q + 3
// after them, so that lane q's two 16-byte LDS reads are 16 bytes from its neighbour's (conflict-free ds_read_b128; in natural
// order they would be 32 bytes apart, two lanes per bank group).
// A NaN distance of ANY class makes the row's minimum NaN (`t != t` below) and with it the maximum: loud, never a finite
// minimum that silently skipped a class.
template <bool VEC, bool IN_LDS, int NC>
__global__ __launch_bounds__(AN_THREADS) void k_an_mindist(const float *__restrict__ rows, int64_t n, int d,
                                                           const double *__restrict__ cent, int k, double *__restrict__ dist,
                                                           int32_t *__restrict__ nearest, unsigned long long *__restrict__ max_bits) {
    extern __shared__ double an_cent[];
    const int nv = d >> 2;
    if (IN_LDS) {
        for (int i = threadIdx.x; i < k * d; i += AN_THREADS) {
            int dst = i;
            if (VEC) {
                const int j = i / d, e = i - j * d;
                dst = j * d + ((e >> 1) & 1) * 2 * nv + 2 * (e >> 2) + (e & 1);
            }
            an_cent[dst] = cent[i];
        }
        __syncthreads();
    }
    const double *C = IN_LDS ? an_cent : cent;
    const int lane = lane_id();
    const int64_t wave = (int64_t)blockIdx.x * AN_WAVES + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * AN_WAVES;
    unsigned long long wmax = 0ull;
    for (int64_t r = wave; r < n; r += nwaves) {
        const float *x = rows + r * d;
        double best = 0.0;
        int arg = 0;
        for (int k0 = 0; k0 < k; k0 += NC) {
            const double *c[NC];                           // classes past k - 1 repeat the last one: computed, never used
            double a[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                c[j] = C + (int64_t)std::min(k0 + j, k - 1) * d;
                a[j] = 0.0;
            }
            if (VEC) {
#pragma unroll 4
                for (int q = lane; q < nv; q += WAVE) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(x + 4 * q);
                    const int lo = IN_LDS ? 2 * q : 4 * q, hi = IN_LDS ? 2 * nv + 2 * q : 4 * q + 2;
#pragma unroll
                    for (int j = 0; j < NC; ++j) {
                        const f64x2 cl = *reinterpret_cast<const f64x2 *>(c[j] + lo), ch = *reinterpret_cast<const f64x2 *>(c[j] + hi);
                        double t;
                        t = (double)v[0] - cl[0]; a[j] = fma(t, t, a[j]);
                        t = (double)v[1] - cl[1]; a[j] = fma(t, t, a[j]);
                        t = (double)v[2] - ch[0]; a[j] = fma(t, t, a[j]);
                        t = (double)v[3] - ch[1]; a[j] = fma(t, t, a[j]);
                    }
                }
            } else {
                for (int q = lane; q < d; q += WAVE) {
                    const double xe = (double)x[q];
#pragma unroll
                    for (int j = 0; j < NC; ++j) {
                        const double t = xe - c[j][q];
                        a[j] = fma(t, t, a[j]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double t = sqrt(wave_butterfly_sum(a[j]));
                if (k0 + j < k && (k0 + j == 0 || t < best || (t != t && best == best))) {
                    best = t;
                    arg = k0 + j;
                }
            }
        }
        if (lane == 0) {
            dist[r] = best;
            nearest[r] = arg;
        }
        const unsigned long long b = (unsigned long long)__double_as_longlong(best) & 0x7fffffffffffffffull;   // a NaN of either sign
        wmax = b > wmax ? b : wmax;
    }
    if (lane == 0 && wmax) atomicMax(max_bits, wmax);
}

// ---- 3. binary ranking metrics ----------------------------------------------------------------------------------------------
// the score whose rank_key is `key` (-0.0 comes back as +0.0, which compares equal)
__device__ inline double score_of_key(uint64_t key) {
    const uint64_t u = (key >> 63) ? key : ~key ^ 0x8000000000000000ull;
    double s;
    __builtin_memcpy(&s, &u, 8);
    return s;
}

__global__ __launch_bounds__(AN_THREADS) void k_bm_build(const double *__restrict__ scores, int64_t n, const double *__restrict__ norm,
                                                         uint64_t *__restrict__ keys, int32_t *__restrict__ pay, int *__restrict__ bad) {
    const int64_t seg = blockIdx.y;
    const double nm = norm ? norm[seg] : 1.0;
    int flags = 0;
    if (norm && !(nm > 0.0 && nm < INFINITY)) flags |= MIRX_ANOMALY_BAD_NORM;
    for (int64_t j = (int64_t)blockIdx.x * AN_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * AN_THREADS) {
        const double s = scores[seg * n + j];
        if (!(fabs(s) < INFINITY)) flags |= MIRX_ANOMALY_BAD_SCORE;
        keys[seg * n + j] = rank_key(norm ? s / nm : s);
        pay[seg * n + j] = (int32_t)j;
    }
    if (flags) atomicOr(bad, flags);
}

// row `row` (64 consecutive sorted elements) of this wave's part of the tile: the lane's key and the wave's masks of positives
// and of group ends
struct BmRow {
    uint64_t key;
    unsigned long long pos, end;
    int64_t i;                  // the lane's position in the segment
};
__device__ inline BmRow bm_row(const uint64_t *__restrict__ keys, const int32_t *__restrict__ pay, const uint8_t *__restrict__ positive,
                               int64_t n, int64_t t0, int wave, int row, int lane) {
    BmRow o;
    o.i = t0 + (wave * BM_ROWS + row) * WAVE + lane;
    const bool valid = o.i < n;
    o.key = valid ? keys[o.i] : 0ull;
    const bool last = o.i + 1 >= n;
    const uint64_t next = (valid && !last) ? keys[o.i + 1] : 0ull;
    const int32_t p = valid ? pay[o.i] : 0;
    const bool is_pos = valid && (uint32_t)p < (uint64_t)n && positive[p] != 0;    // always in range for a sorted payload
    o.pos = __ballot(is_pos);
    o.end = __ballot(valid && (last || o.key != next));
    return o;
}

// grid (tiles, segments): the tile's positives and group ends
__global__ __launch_bounds__(AN_THREADS) void k_bm_count(const uint64_t *__restrict__ keys, const int32_t *__restrict__ pay,
                                                         const uint8_t *__restrict__ positive, int64_t n, int ntiles,
                                                         unsigned *__restrict__ tile_pos, unsigned *__restrict__ tile_end) {
    __shared__ unsigned wp[AN_WAVES], we[AN_WAVES];
    const int64_t seg = blockIdx.y;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * RANK_TILE;
    unsigned np = 0, ne = 0;
    for (int r = 0; r < BM_ROWS; ++r) {
        const BmRow o = bm_row(keys + seg * n, pay + seg * n, positive + seg * n, n, t0, wave, r, lane);
        np += (unsigned)__popcll(o.pos);
        ne += (unsigned)__popcll(o.end);
    }
    if (lane == 0) {
        wp[wave] = np;
        we[wave] = ne;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a = 0, b = 0;
        for (int w = 0; w < AN_WAVES; ++w) {
            a += wp[w];
            b += we[w];
        }
        tile_pos[seg * ntiles + blockIdx.x] = a;
        tile_end[seg * ntiles + blockIdx.x] = b;
    }
}

// inclusive sum over the lanes at or below this one
__device__ inline unsigned bm_wave_inclusive(unsigned v, int lane) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)v, off, WAVE);
        if (lane >= off) v += o;
    }
    return v;
}

// grid (segments): both tile arrays become exclusive prefixes; P and T of the segment
__global__ __launch_bounds__(AN_THREADS) void k_bm_scan(unsigned *__restrict__ tile_pos, unsigned *__restrict__ tile_end, int ntiles,
                                                        int64_t n, int64_t *__restrict__ seg_p, int64_t *__restrict__ out_t,
                                                        int *__restrict__ bad) {
    __shared__ unsigned wp[AN_WAVES], we[AN_WAVES];
    const int64_t seg = blockIdx.x;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    unsigned *tp = tile_pos + seg * ntiles, *te = tile_end + seg * ntiles;
    unsigned run_p = 0, run_e = 0;
    for (int base = 0; base < ntiles; base += AN_THREADS) {
        const int i = base + threadIdx.x;
        const unsigned vp = i < ntiles ? tp[i] : 0u, ve = i < ntiles ? te[i] : 0u;
        const unsigned ip = bm_wave_inclusive(vp, lane), ie = bm_wave_inclusive(ve, lane);
        if (lane == WAVE - 1) {
            wp[wave] = ip;
            we[wave] = ie;
        }
        __syncthreads();
        unsigned bp = 0, be = 0, ap = 0, ae = 0;
#pragma unroll
        for (int w = 0; w < AN_WAVES; ++w) {
            bp += w < wave ? wp[w] : 0u;
            be += w < wave ? we[w] : 0u;
            ap += wp[w];
            ae += we[w];
        }
        __syncthreads();
        if (i < ntiles) {
            tp[i] = run_p + bp + ip - vp;
            te[i] = run_e + be + ie - ve;
        }
        run_p += ap;
        run_e += ae;
    }
    if (threadIdx.x == 0) {
        seg_p[seg] = run_p;
        out_t[seg] = run_e;
        if (run_p == 0 || (int64_t)run_p == n) atomicOr(bad, MIRX_ANOMALY_BAD_ONE_CLASS);
    }
}

// grid (tiles, segments): the records of the tile's group ends
__global__ __launch_bounds__(AN_THREADS) void k_bm_compact(const uint64_t *__restrict__ keys, const int32_t *__restrict__ pay,
                                                           const uint8_t *__restrict__ positive, int64_t n, int ntiles,
                                                           const unsigned *__restrict__ tile_pos, const unsigned *__restrict__ tile_end,
                                                           double *__restrict__ thresholds, int64_t *__restrict__ tps,
                                                           int64_t *__restrict__ fps) {
    __shared__ unsigned wp[AN_WAVES], we[AN_WAVES];
    const int64_t seg = blockIdx.y;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * RANK_TILE;
    const uint64_t *kk = keys + seg * n;
    const int32_t *pp = pay + seg * n;
    const uint8_t *ps = positive + seg * n;
    unsigned np = 0, ne = 0;
    for (int r = 0; r < BM_ROWS; ++r) {
        const BmRow o = bm_row(kk, pp, ps, n, t0, wave, r, lane);
        np += (unsigned)__popcll(o.pos);
        ne += (unsigned)__popcll(o.end);
    }
    if (lane == 0) {
        wp[wave] = np;
        we[wave] = ne;
    }
    __syncthreads();
    int64_t cp = tile_pos[seg * ntiles + blockIdx.x], ce = tile_end[seg * ntiles + blockIdx.x];   // before this wave's first row
    for (int w = 0; w < wave; ++w) {
        cp += wp[w];
        ce += we[w];
    }
    const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
    for (int r = 0; r < BM_ROWS; ++r) {
        const BmRow o = bm_row(kk, pp, ps, n, t0, wave, r, lane);
        if (o.end >> lane & 1ull) {
            const int64_t rec = ce + __popcll(o.end & below);
            const int64_t tp = cp + __popcll(o.pos & upto);
            if (rec < n) {                                     // always, for consistent counts: keeps a bug in bounds
                thresholds[seg * n + rec] = score_of_key(o.key);
                tps[seg * n + rec] = tp;
                fps[seg * n + rec] = o.i + 1 - tp;
            }
        }
        cp += __popcll(o.pos);
        ce += __popcll(o.end);
    }
}

// grid (segments), 1024 threads: the three measures from the segment's T records
__global__ __launch_bounds__(BM_RTHREADS) void k_bm_reduce(const int64_t *__restrict__ tps, const int64_t *__restrict__ fps, int64_t n,
                                                           const int64_t *__restrict__ seg_p, const int64_t *__restrict__ seg_t,
                                                           double level, double *__restrict__ out_auroc, double *__restrict__ out_aupr,
                                                           double *__restrict__ out_fpr) {
    constexpr int NW = BM_RTHREADS / WAVE;
    __shared__ long long s_area[NW], s_idx[NW], s_fp[NW];
    __shared__ double s_ap[NW], s_dev[NW];
    const int64_t seg = blockIdx.x;
    const int64_t T = seg_t[seg], P = seg_p[seg], N = n - P;
    const int64_t *tp_ = tps + seg * n, *fp_ = fps + seg * n;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const double dp = (double)P;
    long long area = 0, bidx = -1, bfp = 0;
    double ap = 0.0, bdev = INFINITY;
    for (int64_t i = threadIdx.x; i < T; i += BM_RTHREADS) {
        const int64_t tp = tp_[i], fp = fp_[i];
        const int64_t tp0 = i ? tp_[i - 1] : 0, fp0 = i ? fp_[i - 1] : 0;
        area += (fp - fp0) * (tp + tp0);
        ap += ((double)(tp - tp0) / dp) * ((double)tp / (double)(tp + fp));
        if (tp0 < P) {                                          // records 0 .. last_ind
            const double dev = fabs((double)tp / dp - level);
            if (dev < bdev || (dev == bdev && i > bidx)) {
                bdev = dev;
                bidx = i;
                bfp = fp;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        area += __shfl_xor(area, off, 64);
        ap = ap + __shfl_xor(ap, off, 64);
        const double odev = __shfl_xor(bdev, off, 64);
        const long long oidx = __shfl_xor(bidx, off, 64), ofp = __shfl_xor(bfp, off, 64);
        if (oidx >= 0 && (bidx < 0 || odev < bdev || (odev == bdev && oidx > bidx))) {
            bdev = odev;
            bidx = oidx;
            bfp = ofp;
        }
    }
    if (lane == 0) {
        s_area[wave] = area;
        s_ap[wave] = ap;
        s_dev[wave] = bdev;
        s_idx[wave] = bidx;
        s_fp[wave] = bfp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; ++w) {
            area += s_area[w];
            ap = ap + s_ap[w];
            if (s_idx[w] >= 0 && (bidx < 0 || s_dev[w] < bdev || (s_dev[w] == bdev && s_idx[w] > bidx))) {
                bdev = s_dev[w];
                bidx = s_idx[w];
                bfp = s_fp[w];
            }
        }
        const bool ok = P > 0 && N > 0;
        out_auroc[seg] = ok ? (double)area / (2.0 * dp * (double)N) : NAN;
        out_aupr[seg] = ok ? ap : NAN;
        out_fpr[seg] = ok ? (double)bfp / (double)N : NAN;
    }
}

unsigned an_grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + AN_THREADS - 1) / AN_THREADS, 4096); }

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

// ---- host side --------------------------------------------------------------------------------------------------------------
int64_t an_chunk_rows(int64_t n, int d) {
    const int64_t cap = std::min<int64_t>(512, std::max<int64_t>(8, 524288 / d));
    const int64_t nch = std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, cap));
    return (n + nch - 1) / nch;
}

static int64_t an_chunks(int64_t n, int d) {
    const int64_t cr = an_chunk_rows(n, d);
    return (n + cr - 1) / cr;
}

int64_t class_centroids_workspace_bytes(int64_t n, int d, int k) {
    const int64_t nch = an_chunks(n, d);
    return (int64_t)(align256((size_t)n * 4) + align256((size_t)nch * k * 4) + align256((size_t)nch * k * d * 8));
}

hipError_t launch_class_centroids(const float *rows, int64_t n, int d, const int64_t *labels, const int64_t *classes_host, int k,
                                  void *workspace, double *centroids, int64_t *counts, int *bad, hipStream_t st) {
    const int64_t cr = an_chunk_rows(n, d), nch = an_chunks(n, d);
    char *ws = static_cast<char *>(workspace);
    int32_t *cls = reinterpret_cast<int32_t *>(ws);
    unsigned *cnt_part = reinterpret_cast<unsigned *>(ws + align256((size_t)n * 4));
    double *partial = reinterpret_cast<double *>(ws + align256((size_t)n * 4) + align256((size_t)nch * k * 4));
    ClassList cl{};
    for (int j = 0; j < k; ++j) cl.v[j] = classes_host[j];
    hipLaunchKernelGGL(k_an_classify, dim3((unsigned)nch), dim3(AN_THREADS), 0, st, labels, n, cr, cl, k, cls, cnt_part);
    const size_t lds = (size_t)k * AN_THREADS * sizeof(double);
    if (lds > 64 * 1024) {
        const hipError_t e = set_dynamic_lds(k_an_partial, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_an_partial, dim3((unsigned)nch, (unsigned)((d + AN_THREADS - 1) / AN_THREADS)), dim3(AN_THREADS), lds, st,
                       rows, n, d, cr, cls, k, partial);
    hipLaunchKernelGGL(k_an_reduce, dim3((unsigned)(((int64_t)k * d + AN_THREADS - 1) / AN_THREADS)), dim3(AN_THREADS), 0, st,
                       partial, cnt_part, nch, k, d, centroids, counts, bad);
    return hipGetLastError();
}

hipError_t launch_centroid_min_dist(const float *rows, int64_t n, int d, const double *centroids, int k, double *dist,
                                    int32_t *nearest, double *max_out, hipStream_t st) {
    hipError_t e = hipMemsetAsync(max_out, 0, sizeof(double), st);
    if (e != hipSuccess) return e;
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0 && (reinterpret_cast<uintptr_t>(centroids) & 15) == 0;
    const size_t bytes = (size_t)k * d * sizeof(double);
    const bool in_lds = bytes <= (size_t)AN_MD_LDS_BYTES;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + AN_WAVES - 1) / AN_WAVES, (int64_t)current_device_cus() * 8));
    unsigned long long *mb = reinterpret_cast<unsigned long long *>(max_out);
    const size_t lds = in_lds ? bytes : 0;
#define MIRX_AN_MD(V, L, NC) hipLaunchKernelGGL((k_an_mindist<V, L, NC>), dim3(grid), dim3(AN_THREADS), lds, st, rows, n, d, centroids, k, dist, nearest, mb)
#define MIRX_AN_MD_NC(V, L) \
    do {                    \
        if (k == 1) MIRX_AN_MD(V, L, 1); \
        else if (k == 2) MIRX_AN_MD(V, L, 2); \
        else MIRX_AN_MD(V, L, 4); \
    } while (0)
    if (vec && in_lds) MIRX_AN_MD_NC(true, true);
    else if (vec) MIRX_AN_MD_NC(true, false);
    else if (in_lds) MIRX_AN_MD_NC(false, true);
    else MIRX_AN_MD_NC(false, false);
#undef MIRX_AN_MD_NC
#undef MIRX_AN_MD
    return hipGetLastError();
}

int64_t binary_rank_metrics_workspace_bytes(int64_t nseg, int64_t n) {
    const size_t tot = (size_t)nseg * n, tiles = (size_t)nseg * rank_sort_tiles(n);
    return (int64_t)(2 * align256(tot * 8) + 2 * align256(tot * 4) + align256(tiles * 256 * 4) + 2 * align256(tiles * 4) +
                     align256((size_t)nseg * 8));
}

hipError_t launch_binary_rank_metrics(const double *scores, const uint8_t *positive, int64_t nseg, int64_t n, const double *norm,
                                      double level, void *workspace, double *thresholds, int64_t *tps, int64_t *fps, int64_t *out_t,
                                      double *out_auroc, double *out_aupr, double *out_fpr, int *bad, hipStream_t st) {
    const size_t tot = (size_t)nseg * n;
    const int ntiles = (int)rank_sort_tiles(n);
    const size_t tiles = (size_t)nseg * ntiles;
    char *ws = static_cast<char *>(workspace);
    uint64_t *keys_a = reinterpret_cast<uint64_t *>(ws);
    ws += align256(tot * 8);
    uint64_t *keys_b = reinterpret_cast<uint64_t *>(ws);
    ws += align256(tot * 8);
    int32_t *pay_a = reinterpret_cast<int32_t *>(ws);
    ws += align256(tot * 4);
    int32_t *pay_b = reinterpret_cast<int32_t *>(ws);
    ws += align256(tot * 4);
    unsigned *hist = reinterpret_cast<unsigned *>(ws);
    ws += align256(tiles * 256 * 4);
    unsigned *tile_pos = reinterpret_cast<unsigned *>(ws);
    ws += align256(tiles * 4);
    unsigned *tile_end = reinterpret_cast<unsigned *>(ws);
    ws += align256(tiles * 4);
    int64_t *seg_p = reinterpret_cast<int64_t *>(ws);
    const dim3 tgrid((unsigned)ntiles, (unsigned)nseg);
    hipLaunchKernelGGL(k_bm_build, dim3(an_grid_for(n), (unsigned)nseg), dim3(AN_THREADS), 0, st, scores, n, norm, keys_a, pay_a, bad);
    const hipError_t e = launch_rank_sort(keys_a, pay_a, keys_b, pay_b, hist, n, (int)nseg, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bm_count, tgrid, dim3(AN_THREADS), 0, st, keys_a, pay_a, positive, n, ntiles, tile_pos, tile_end);
    hipLaunchKernelGGL(k_bm_scan, dim3((unsigned)nseg), dim3(AN_THREADS), 0, st, tile_pos, tile_end, ntiles, n, seg_p, out_t, bad);
    hipLaunchKernelGGL(k_bm_compact, tgrid, dim3(AN_THREADS), 0, st, keys_a, pay_a, positive, n, ntiles, tile_pos, tile_end, thresholds,
                       tps, fps);
    hipLaunchKernelGGL(k_bm_reduce, dim3((unsigned)nseg), dim3(BM_RTHREADS), 0, st, tps, fps, n, seg_p, out_t, level, out_auroc,
                       out_aupr, out_fpr);
    return hipGetLastError();
}

}  // namespace mirx
