// k_finalize.hip -- the filter routes' tail: threshold selection from sampled group maxima, and the per-query finalize (gather
// and sort the candidates, completeness guard, fp64 re-rank, final top-k), one kernel source at two capacities: CAND_CAP
// candidates on 256 threads (mirx_index_search) and DEEP_CAP on 1024 (mirx_index_search_deep).
//
// Why the result is exact (DESIGN.md "Exactness"), whatever the capacity: the GEMM stores EVERY row whose approximate score s~
// exceeds tau.  With |s~ - s| <= eps for every row (filter_eps), the true top-k_eff rows all have s~ >= kth(s~) - 2 eps.  So if
// (a) the list did not overflow -- at most CAP candidates, no region's surplus lost to a full overflow list --, (b) it holds at
// least k_eff rows and (c) tau < lo = kth(s~) - 2 eps (rounded down), then re-scoring exactly the rows with s~ >= lo in fp64, in
// the oracle's summation order (lane_tree_score), and sorting them (score desc, id asc) gives the oracle's answer.  A query that
// fails (c) alone is filtered once more with tau2 just below lo (retry list); every other failure, and a failure of the second
// pass, goes to the exact scan (fail list).  Nothing is answered from approximate scores.
//
// Leave-group-out (CODES, mirx_index_search_leave_out): the same argument restricted to the eligible set E = the rows
// whose code is not the query's.  A candidate outside E is dropped as it is gathered, before the sort: it never counts toward
// c >= k_eff, never becomes the k_eff-th key and is never re-scored.  With no overflow the survivors are exactly E n {s~ > tau}
// (overflow is still decided on the raw count: a lost candidate may have been eligible).  With at least k_eff survivors and
// tau < lo = kth_surv(s~) - 2 eps, every eligible row with s~ >= lo is a survivor, and the true top k_eff of E all have
// s~ >= kth_surv(s~) - 2 eps: they are among the re-scored rows.  The retry threshold tau2 is derived from kth_surv, so the second
// pass is complete for E by construction.  The instantiations without CODES read neither code pointer.
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

namespace mirx {

namespace {

// tau[q] = rank_j-th largest sampled group maximum of query q; +inf for padding queries.
__global__ __launch_bounds__(256) void k_select_tau(const float *__restrict__ groupmax, int ngroups,
                                                    int64_t nq, int rank_j, float *__restrict__ tau) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *a = reinterpret_cast<float *>(smem);
    const int64_t qi = blockIdx.x;
    if (qi >= nq) {
        if (threadIdx.x == 0) tau[qi] = INFINITY;
        return;
    }
    const int m = pow2_ceil(ngroups);
    for (int i = threadIdx.x; i < m; i += 256) a[i] = i < ngroups ? groupmax[qi * ngroups + i] : -INFINITY;
    bitonic_lds(a, m, [](float x, float y) { return x > y; });
    if (threadIdx.x == 0) {
        const int j = rank_j < ngroups ? rank_j : ngroups;
        tau[qi] = a[j - 1];
    }
}

// One workgroup of THREADS threads per query.  Dynamic LDS: CAP keys (8 B) and CAP hits (16 B) -- 24 KiB at CAND_CAP, six
// workgroups per CU; 96 KiB at DEEP_CAP, one workgroup of 16 waves per CU (160 KiB).  The hits' storage doubles as the region
// offsets during the gather.  At run = CAP tied rows every candidate is re-scored, so the hits cannot be bounded below CAP.
// Counters are integer atomics; no floating-point atomic is used.
template <int METRIC, int CAP, int THREADS, bool CODES>
__global__ __launch_bounds__(THREADS) void k_finalize(FinalizeArgs A) {
    static_assert((DEEP_MAX_REGIONS + 1) * sizeof(int) <= CAP * sizeof(Hit), "the region offsets live in the hits' storage");
    constexpr int WAVES = THREADS / WAVE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);                 // [CAP]
    Hit *hits = reinterpret_cast<Hit *>(smem + (size_t)CAP * sizeof(unsigned long long));    // [CAP]
    __shared__ int sh_ok, sh_m, sh_drop;
    __shared__ float sh_lo;
    const int slot_q = blockIdx.x;                                  // index into tau / candidate buffers
    const int qi = A.qmap ? A.qmap[slot_q] : slot_q;                // original query number
    const int wave = threadIdx.x >> 6, lane = lane_id();

    // ---- gather and sort.  Where a candidate lands does not matter: the keys are distinct and sorted next.
    // CODES: a candidate that carries the query's code gets the padding key 0, below every real key (a real key's high word is
    // 0 only for a NaN score, which passes no threshold), so the sort leaves the survivors in keys[0 .. c)
    int32_t qcode = -1;
    int dropped = 0;
    if constexpr (CODES) {
        qcode = A.query_codes[qi];
        if (threadIdx.x == 0) sh_drop = 0;                          // (gather_cands' first barrier orders this before the adds)
    }
    const Gathered got = gather_cands<THREADS>(A.lists, slot_q, CAP, reinterpret_cast<int *>(hits), [&](int p, const Cand cd) {
        if constexpr (CODES) {
            const bool out = qcode >= 0 && A.row_codes[cd.row] == qcode;
            dropped += out ? 1 : 0;
            keys[p] = out ? 0ull : cand_key(cd);
        } else {
            keys[p] = cand_key(cd);
        }
    });
    const bool overflow = got.lost;
    const int taken = overflow ? 0 : got.taken;
    int c = taken;                                                  // the candidates that can rank
    if constexpr (CODES) {
        dropped = wave_isum(dropped);
        if (lane == 0 && dropped) atomicAdd(&sh_drop, dropped);
        __syncthreads();
        dropped = sh_drop;
        c = taken - dropped;
    }
    const int m2 = pow2_ceil(taken > 1 ? taken : 1);
    for (int i = taken + threadIdx.x; i < m2; i += THREADS) keys[i] = 0ull;
    const int64_t ex = A.exclude ? A.exclude[qi] : -1;
    const int k_eff = A.k + (ex >= 0 ? 1 : 0);
    if (!overflow) bitonic_lds(keys, m2, [](unsigned long long x, unsigned long long y) { return x > y; });

    // ---- guard
    if (threadIdx.x == 0) {
        int ok = (!overflow && c >= k_eff) ? 1 : 0, retry = 0;
        float lo = 0.0f;
        if (ok) {
            const float kth = f32_from_orderable((uint32_t)(keys[k_eff - 1] >> 32));
            const float gmax = __uint_as_float(*A.gnorm_max_bits);
            const float qn = A.qnorm[qi];
            const float eps = filter_eps<METRIC>(qn, gmax, A.dimp);        // |s~ - s| <= eps
            lo = kth - 2.0f * eps;
            lo -= fabsf(lo) * 2.4e-7f + 1e-37f;            // round toward -inf with margin
            ok = (A.tau[slot_q] < lo) ? 1 : 0;
            if (!ok) {
                atomicAdd((unsigned long long *)&A.stats->incomplete, 1ull);
                if (A.retry_list) {
                    // the k-th best s~ is final (every row above tau was seen), so tau2 just below
                    // `lo` makes the next filter pass complete by construction
                    const int p = atomicAdd(A.fail_count + 1, 1);
                    A.retry_list[p] = qi;
                    A.tau2[qi] = lo - (fabsf(lo) * 2.4e-7f + 1e-37f);
                    retry = 1;
                }
            }
        } else {
            if (overflow) atomicAdd((unsigned long long *)&A.stats->overflowed, 1ull);
            else atomicAdd((unsigned long long *)&A.stats->incomplete, 1ull);
        }
        if (!ok && !retry) {
            const int p = atomicAdd(A.fail_count, 1);
            A.fail_list[p] = qi;
        }
        sh_ok = ok;
        sh_lo = lo;
        sh_m = 0;
    }
    __syncthreads();
    if (!sh_ok) return;
    const float lo = sh_lo;
    {
        int n = 0;
        for (int i = threadIdx.x; i < c; i += THREADS) n += cand_key_score(keys[i]) >= lo ? 1 : 0;
        n = wave_isum(n);
        if (lane == 0 && n) atomicAdd(&sh_m, n);
    }
    __syncthreads();
    const int m = sh_m;                                   // sorted, so these are keys[0..m)

    // ---- re-score in fp64, one row per wave and trip (the region offsets are dead: the hits take their storage)
    const float *qrow = A.q32p + (int64_t)qi * A.dimp;
    for (int i = wave; i < m; i += WAVES) {
        const uint32_t row = cand_key_row(keys[i]);
        const double s = lane_tree_score<METRIC>(qrow, A.g32 + (int64_t)row * A.dimp, A.dimp);
        if (lane == 0) {
            const int64_t id = A.ids[row];
            Hit h;
            h.s = (id == ex) ? -INFINITY : s;
            h.id = (id == ex) ? ID_LAST : id;
            hits[i] = h;
        }
    }
    const int mp = pow2_ceil(m > 1 ? m : 1);
    for (int i = m + threadIdx.x; i < mp; i += THREADS) { hits[i].s = -INFINITY; hits[i].id = ID_LAST; }
    bitonic_lds(hits, mp, [](const Hit &x, const Hit &y) { return hit_before(x.s, x.id, y.s, y.id); });
    for (int r = threadIdx.x; r < A.k; r += THREADS) {
        Hit h;
        h.s = -INFINITY;
        h.id = ID_LAST;
        if (r < mp) h = hits[r];
        const bool empty = h.id == ID_LAST;                // an empty slot's score is -inf, which reported_value keeps
        const int64_t o = (int64_t)qi * A.k + r;
        if (A.out_f64) A.out_f64[o] = empty ? -INFINITY : h.s;
        A.out_ids[o] = empty ? -1 : h.id;
        if (A.out_val) A.out_val[o] = reported_value(h.s, A.metric);
    }
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long *)&A.stats->tier1_answered, 1ull);
        atomicAdd((unsigned long long *)&A.stats->candidates, (unsigned long long)got.raw);
        atomicAdd((unsigned long long *)&A.stats->reranked, (unsigned long long)m);
        if constexpr (CODES) atomicAdd((unsigned long long *)&A.stats->left_out, (unsigned long long)dropped);
    }
}

__global__ __launch_bounds__(256) void k_gather_queries(const uint16_t *__restrict__ q16,
                                                        const float *__restrict__ tau2,
                                                        const int32_t *__restrict__ list, int n, int dimp,
                                                        uint16_t *__restrict__ q16r, float *__restrict__ taur) {
    const int64_t i = blockIdx.x;
    const int chunks = dimp / 8;                                    // 16-byte pieces per row
    uint4 *dst = reinterpret_cast<uint4 *>(q16r + i * dimp);
    if (i < n) {
        const int32_t qi = list[i];
        const uint4 *src = reinterpret_cast<const uint4 *>(q16 + (int64_t)qi * dimp);
        for (int c = threadIdx.x; c < chunks; c += 256) dst[c] = src[c];
        if (threadIdx.x == 0) taur[i] = tau2[qi];
    } else {
        for (int c = threadIdx.x; c < chunks; c += 256) dst[c] = make_uint4(0, 0, 0, 0);
        if (threadIdx.x == 0) taur[i] = INFINITY;
    }
}

template <int METRIC, int CAP, int THREADS, bool CODES>
hipError_t launch_finalize_as(const FinalizeArgs &a, hipStream_t st) {
    constexpr size_t LDS_BYTES = (size_t)CAP * (sizeof(unsigned long long) + sizeof(Hit));
    if constexpr (LDS_BYTES > 64 * 1024) {
        static std::atomic<unsigned long long> attr_devs{0};
        const hipError_t e = set_dynamic_lds(k_finalize<METRIC, CAP, THREADS, CODES>, LDS_BYTES, &attr_devs);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_finalize<METRIC, CAP, THREADS, CODES>), dim3(a.nq), dim3(THREADS), LDS_BYTES, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gather_queries(const uint16_t *q16, const float *tau2, const int32_t *list, int n,
                                 int64_t n_pad, int dimp, uint16_t *q16r, float *taur, hipStream_t st) {
    if (n_pad <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_queries, dim3((unsigned)n_pad), dim3(256), 0, st, q16, tau2, list, n, dimp, q16r,
                       taur);
    return hipGetLastError();
}

hipError_t launch_select_tau(const float *groupmax, int ngroups, int64_t nq, int64_t nq_pad, int rank_j,
                             float *tau, hipStream_t st) {
    if (nq_pad <= 0) return hipSuccess;
    int m = 1;
    while (m < ngroups) m <<= 1;
    if (m > 16384) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_devs{0};
    hipError_t e = set_dynamic_lds(k_select_tau, 16384 * (int)sizeof(float), &attr_devs);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_select_tau, dim3((unsigned)nq_pad), dim3(256), (size_t)m * sizeof(float), st,
                       groupmax, ngroups, nq, rank_j, tau);
    return hipGetLastError();
}

hipError_t launch_finalize(const FinalizeArgs &a, bool deep, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (a.lists.regions < 1 || a.lists.regions > DEEP_MAX_REGIONS || a.lists.slots < 1 || a.k < 1 || a.k > MAX_K)
        return hipErrorInvalidValue;
    const bool ip = a.metric == MIRX_METRIC_IP;
    if (a.row_codes) {                                              // leave-group-out: the CODES twins
        if (!a.query_codes) return hipErrorInvalidValue;
        if (deep) return ip ? launch_finalize_as<0, DEEP_CAP, 1024, true>(a, st) : launch_finalize_as<1, DEEP_CAP, 1024, true>(a, st);
        return ip ? launch_finalize_as<0, CAND_CAP, 256, true>(a, st) : launch_finalize_as<1, CAND_CAP, 256, true>(a, st);
    }
    if (deep) return ip ? launch_finalize_as<0, DEEP_CAP, 1024, false>(a, st) : launch_finalize_as<1, DEEP_CAP, 1024, false>(a, st);
    return ip ? launch_finalize_as<0, CAND_CAP, 256, false>(a, st) : launch_finalize_as<1, CAND_CAP, 256, false>(a, st);
}

}  // namespace mirx
