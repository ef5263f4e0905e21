// k_range.hip -- range search (mirx_index_range_search): every row whose fp64 ranking score s lies in (lo, hi], per query, best
// first.  pymilvus' radius / range_filter search parameters; the near-duplicate self-join over a gallery.
//
// Filter route: the filter GEMM (k_gemm.hip, unchanged) stores EVERY row whose approximate score s~ exceeds tau[q].  k_range_tau
// puts tau[q] below lo'[q] - eps[q], where lo' is the bound in the GEMM's units and |s~ - s'| <= eps (DESIGN 33 states the
// inequality), so every row with s > lo is a candidate.  k_range_finalize re-scores ALL candidates of a query in fp64 (the
// lane-tree order of k_finalize) and keeps those with lo < s <= hi, allow[row] != 0 and id != the excluded id: membership of a
// row does not depend on other rows, so mask and exclusion are plain tests.  A query whose candidate lists overflowed is not
// answered here: it goes to the exact route.
//
// Exact route: fp64 scores of all rows and the radix ranking (k_ranksort.hip) with masked and excluded rows behind every score;
// the hits of a query are then the span [first s <= hi, first s <= lo) of its sorted keys, found by two binary searches.
//
// CSR assembly: an exclusive scan of the per-query counts gives lims; one kernel moves the 16-byte (score, id) records of the
// staging rows and of the exact route's segments to their places.  Positions come from counts and scans alone.
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

namespace mirx {

namespace {

constexpr int RANGE_SORT = 2048;                 // power of two >= RANGE_CAP

// One wave per query.  The GEMM scores s' = q.g (metric 0) or q.g - ||g||^2 / 2 (metric 1), for which s = s' resp.
// s = 2 s' - ||q||^2: s > lo  <=>  s' > lo' with lo' = lo resp. (lo + ||q||^2) / 2.  ||q||^2 is summed here in fp64 (lane tree).
// eps is k_finalize's bound of |s~ - s'| (filter_eps); e64 covers what fp64 rounding can move lo' and the lane-tree s
// against the real numbers; then fp32 round-down and the nudge k_finalize applies to its own bound.
template <int METRIC>
__global__ __launch_bounds__(256) void k_range_tau(const float *__restrict__ q32p, const float *__restrict__ qnorm,
                                                   const unsigned *__restrict__ gnorm_max_bits, double lo, int dimp, int64_t nq,
                                                   int64_t nq_pad, float *__restrict__ tau) {
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq_pad) return;
    if (qi >= nq) {
        if (lane_id() == 0) tau[qi] = INFINITY;
        return;
    }
    const float *qrow = q32p + qi * dimp;
    const double qq = lane_tree_score<0>(qrow, qrow, dimp);
    if (lane_id() != 0) return;
    const float gmax = __uint_as_float(*gnorm_max_bits);
    const float qn = qnorm[qi];
    const float eps = filter_eps<METRIC>(qn, gmax, dimp);
    const double span = METRIC == 0 ? (double)qn * (double)gmax : ((double)qn + (double)gmax) * ((double)qn + (double)gmax);
    const double e64 = (span + fabs(lo)) * (double)(dimp + 8) * 2.220446049250313e-16;
    const double lop = METRIC == 0 ? lo : 0.5 * (lo + qq);
    const double below = lop - (double)eps - e64;
    float t = (float)below;
    if ((double)t > below) t = nextafterf(t, -INFINITY);           // fp32 round-down
    t -= fabsf(t) * 2.4e-7f + 1e-37f;                              // and k_finalize's nudge on top
    tau[qi] = t;
}

template <int METRIC>
__global__ __launch_bounds__(256) void k_range_finalize(RangeFinalizeArgs A) {
    __shared__ int32_t rows[RANGE_CAP];
    __shared__ Hit hits[RANGE_SORT];
    static_assert((DEEP_MAX_REGIONS + 1) * sizeof(int) <= sizeof(hits), "the region offsets live in the hits' storage");
    __shared__ int sh_hits;
    const int qi = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = lane_id();
    if (threadIdx.x == 0) sh_hits = 0;
    // the query's candidate rows; where a row lands does not matter, the hits are sorted by (score, id)
    const Gathered got = gather_cands<256>(A.lists, qi, RANGE_CAP, reinterpret_cast<int *>(hits),
                                           [&](int p, const Cand cd) { rows[p] = cd.row; });
    if (got.lost) {                                                // some candidate was lost: the exact route answers
        if (threadIdx.x == 0) {
            const int p = atomicAdd(A.fail_count, 1);
            A.fail_list[p] = qi;
            A.count[qi] = 0;
        }
        return;
    }
    const int c = got.taken;
    const bool has_ex = A.exclude != nullptr;
    const int64_t ex = has_ex ? A.exclude[qi] : 0;
    const float *qrow = A.q32p + (int64_t)qi * A.dimp;
    for (int i = wave; i < c; i += 4) {
        const uint32_t row = (uint32_t)rows[i];
        Hit h;
        h.s = -INFINITY;
        h.id = ID_LAST;
        if ((int64_t)row < A.n_rows) {                             // always, for a row the GEMM stored: keeps a bug in bounds
            const double s = lane_tree_score<METRIC>(qrow, A.g32 + (int64_t)row * A.dimp, A.dimp);
            if (lane == 0) {
                const int64_t id = A.ids[row];
                const bool keep = s > A.lo && s <= A.hi && (!A.allow || A.allow[row] != 0) && !(has_ex && id == ex);
                if (keep) {
                    h.s = s;
                    h.id = id;
                    atomicAdd(&sh_hits, 1);
                }
            }
        }
        if (lane == 0) hits[i] = h;
    }
    const int mp = pow2_ceil(c > 1 ? c : 1);
    for (int i = c + threadIdx.x; i < mp; i += 256) { hits[i].s = -INFINITY; hits[i].id = ID_LAST; }
    bitonic_lds(hits, mp, [](const Hit &x, const Hit &y) { return hit_before(x.s, x.id, y.s, y.id); });
    const int m = sh_hits;                                         // every hit has s > lo >= -inf: they are hits[0 .. m)
    Hit *dst = A.stage + (int64_t)qi * RANGE_CAP;
    for (int r = threadIdx.x; r < m; r += 256) dst[r] = hits[r];
    if (threadIdx.x == 0) {
        A.count[qi] = m;
        atomicAdd(A.stats + 0, 1ull);
        atomicAdd(A.stats + 1, (unsigned long long)got.raw);
    }
}

__global__ __launch_bounds__(256) void k_range_gather_exclude(const int64_t *__restrict__ exclude, const int32_t *__restrict__ list,
                                                              int n, int64_t *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = exclude[list[i]];
}

// first position of the ascending keys[0 .. n) that is >= k
__device__ inline int64_t key_lower_bound(const uint64_t *keys, int64_t n, uint64_t k) {
    int64_t a = 0, b = n;
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (keys[mid] < k) a = mid + 1;
        else b = mid;
    }
    return a;
}

// rank_key descends with the score: s <= hi <=> key(s) >= key(hi), s > lo <=> key(s) < key(lo).  Masked and excluded rows carry
// RANK_KEY_LAST, which no key(lo) reaches (key(-inf) is below it).
__global__ __launch_bounds__(256) void k_range_cut(const uint64_t *__restrict__ keys, int64_t n, int nq, uint64_t key_hi,
                                                   uint64_t key_lo, const int32_t *__restrict__ list, int64_t q_first,
                                                   int32_t *__restrict__ first, int32_t *__restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const uint64_t *k = keys + (int64_t)i * n;
    const int64_t a = key_lower_bound(k, n, key_hi);
    const int64_t b = key_lower_bound(k, n, key_lo);
    const int64_t qx = list ? list[i] : q_first + i;
    first[i] = (int32_t)a;
    count[qx] = (int32_t)(b > a ? b - a : 0);
}

// One workgroup: thread t sums a contiguous run of counts, the runs' sums are scanned in LDS, then each thread writes its run.
__global__ __launch_bounds__(256) void k_range_scan(const int32_t *__restrict__ count, const int32_t *__restrict__ list,
                                                    int64_t q_first, int m, int64_t base, int64_t *__restrict__ off,
                                                    int64_t *__restrict__ tail, int64_t *__restrict__ total_out) {
    __shared__ int64_t part[256];
    const int per = (m + 255) / 256;
    const int i0 = threadIdx.x * per;
    const int i1 = i0 + per < m ? i0 + per : m;
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) sum += count[list ? list[i] : q_first + i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 256; ++t) {
            const int64_t v = part[t];
            part[t] = run;
            run += v;
        }
        if (tail) tail[0] = base + run;
        total_out[0] = base + run;
    }
    __syncthreads();
    int64_t at = base + part[threadIdx.x];
    for (int i = i0; i < i1; ++i) {
        const int64_t qx = list ? list[i] : q_first + i;
        off[qx] = at;
        at += count[qx];
    }
}

__global__ __launch_bounds__(256) void k_range_emit(const int32_t *__restrict__ pay, int64_t n, const double *__restrict__ scores,
                                                    int64_t ld, const int64_t *__restrict__ ids, const int32_t *__restrict__ list,
                                                    int64_t q_first, const int32_t *__restrict__ first,
                                                    const int32_t *__restrict__ count, const int64_t *__restrict__ off,
                                                    Hit *__restrict__ seg) {
    const int64_t i = blockIdx.y;
    const int64_t qx = list ? list[i] : q_first + i;
    const int64_t c = count[qx], a = first[i];
    Hit *dst = seg + off[qx];
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < c; p += (int64_t)gridDim.x * 256) {
        const int64_t at = a + p;
        if (at >= n) break;                                        // never: a + c <= n by the cut
        uint32_t r = (uint32_t)pay[i * n + at];
        if ((int64_t)r >= n) r = 0;                                // never for a permutation: keeps a bug in bounds
        Hit h;
        h.s = scores[i * ld + r];
        h.id = ids[r];
        dst[p] = h;
    }
}

__global__ __launch_bounds__(256) void k_range_compact(const Hit *__restrict__ stage, const Hit *__restrict__ seg,
                                                       const int64_t *__restrict__ xoff, const int32_t *__restrict__ count,
                                                       const int64_t *__restrict__ lims, Hit *__restrict__ out) {
    const int64_t qi = blockIdx.x;
    const int64_t c = count[qi];
    const int64_t xo = xoff[qi];
    // 16-byte records on both sides (hipMalloc'ed arrays of Hit): each move is one 16-byte load and store
    const double2 *src = reinterpret_cast<const double2 *>(xo >= 0 ? seg + xo : stage + qi * RANGE_CAP);
    double2 *dst = reinterpret_cast<double2 *>(out + lims[qi]);
    for (int64_t p = threadIdx.x; p < c; p += 256) dst[p] = src[p];
}

__global__ __launch_bounds__(256) void k_range_fetch(const Hit *__restrict__ res, int64_t total, int metric,
                                                     float *__restrict__ out_val, double *__restrict__ out_f64,
                                                     int64_t *__restrict__ out_ids) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
        const Hit h = res[p];
        if (out_val) out_val[p] = reported_value(h.s, metric);
        if (out_f64) out_f64[p] = h.s;
        out_ids[p] = h.id;
    }
}

inline unsigned grid_for(int64_t n, int64_t cap) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

hipError_t launch_range_tau(const float *q32p, const float *qnorm, const unsigned *gnorm_max_bits, double lo, int dimp, int metric,
                            int64_t nq, int64_t nq_pad, float *tau, hipStream_t st) {
    if (nq_pad <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nq_pad + 3) / 4));
    if (metric == MIRX_METRIC_IP)
        hipLaunchKernelGGL(k_range_tau<0>, grid, dim3(256), 0, st, q32p, qnorm, gnorm_max_bits, lo, dimp, nq, nq_pad, tau);
    else
        hipLaunchKernelGGL(k_range_tau<1>, grid, dim3(256), 0, st, q32p, qnorm, gnorm_max_bits, lo, dimp, nq, nq_pad, tau);
    return hipGetLastError();
}

hipError_t launch_range_finalize(const RangeFinalizeArgs &a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (a.lists.regions < 1 || a.lists.regions > DEEP_MAX_REGIONS || a.lists.slots < 1) return hipErrorInvalidValue;
    if (a.metric == MIRX_METRIC_IP)
        hipLaunchKernelGGL(k_range_finalize<0>, dim3(a.nq), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_range_finalize<1>, dim3(a.nq), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_range_gather_exclude(const int64_t *exclude, const int32_t *list, int n, int64_t *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_range_gather_exclude, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, exclude, list, n, out);
    return hipGetLastError();
}

hipError_t launch_range_cut(const uint64_t *keys, int64_t n, int nq, double lo, double hi, const int32_t *list, int64_t q_first,
                            int32_t *first, int32_t *count, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_range_cut, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, keys, n, nq, rank_key(hi), rank_key(lo),
                       list, q_first, first, count);
    return hipGetLastError();
}

hipError_t launch_range_scan(const int32_t *count, const int32_t *list, int64_t q_first, int m, int64_t base, int64_t *off,
                             int64_t *tail_or_null, int64_t *total_out, hipStream_t st) {
    hipLaunchKernelGGL(k_range_scan, dim3(1), dim3(256), 0, st, count, list, q_first, m, base, off, tail_or_null, total_out);
    return hipGetLastError();
}

hipError_t launch_range_emit(const int32_t *pay, int64_t n, const double *scores, int64_t ld, const int64_t *ids, int nq,
                             const int32_t *list, int64_t q_first, const int32_t *first, const int32_t *count, const int64_t *off,
                             Hit *seg, hipStream_t st) {
    if (nq <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_range_emit, dim3(grid_for(n, 64), (unsigned)nq), dim3(256), 0, st, pay, n, scores, ld, ids, list, q_first,
                       first, count, off, seg);
    return hipGetLastError();
}

hipError_t launch_range_compact(const Hit *stage, const Hit *seg, const int64_t *xoff, const int32_t *count, const int64_t *lims,
                                int nq, Hit *out, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_range_compact, dim3((unsigned)nq), dim3(256), 0, st, stage, seg, xoff, count, lims, out);
    return hipGetLastError();
}

hipError_t launch_range_fetch(const Hit *res, int64_t total, int metric, float *out_val, double *out_f64, int64_t *out_ids,
                              hipStream_t st) {
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_range_fetch, dim3(grid_for(total, 4096)), dim3(256), 0, st, res, total, metric, out_val, out_f64, out_ids);
    return hipGetLastError();
}

}  // namespace mirx
