// k_finalize_deep.hip -- the per-query tail of the deep route (mirx_index_search_deep): k_finalize's job for candidate
// lists of up to DEEP_CAP = 4096 rows, k_eff up to 1025.
//
// Why the result is exact -- k_finalize's argument, unchanged by the capacity: the GEMM stores EVERY row whose approximate score
// s~ exceeds tau.  With |s~ - s| <= eps for every row (filter_eps), the true top-k_eff rows all have s~ >= kth(s~) - 2 eps.  So
// if (a) the list did not overflow -- at most DEEP_CAP candidates, no region's surplus lost to a full overflow list --, (b) it
// holds at least k_eff rows and (c) tau < lo = kth(s~) - 2 eps (rounded down), then re-scoring exactly the rows with s~ >= lo in
// fp64, in the oracle's summation order (lane_tree_score), and sorting them (score desc, id asc) gives the oracle's answer.  A
// query that fails (c) alone is filtered once more with tau2 just below lo (retry list); every other failure, and a failure of
// the second pass, goes to the exact scan (fail list).  Nothing is answered from approximate scores.
//
// Shape: one workgroup of 1024 threads (16 waves) per query.
//   gather    the region counts are scanned (a workgroup prefix sum over up to DEEP_MAX_REGIONS regions), then all threads copy
//             the flattened candidate positions, each finding its region by a binary search of the offsets; the overflow list
//             follows.  Where a candidate lands does not matter: the keys are distinct (one per row) and sorted next.
//   sort      bitonic network over the keys (orderable s~, ~row) in LDS
//   guard     thread 0, as in k_finalize
//   re-score  16 waves, one candidate row per wave and trip; the sort of the hits; k outputs
// LDS: keys 4096 x 8 B = 32 KiB and hits 4096 x 16 B = 64 KiB, 96 KiB of dynamic LDS (set_dynamic_lds) plus 144 bytes static: one
// workgroup per CU (160 KiB), 16 waves, four per SIMD.  The hits' storage doubles as the region offsets during the gather.  At
// run = DEEP_CAP tied rows every candidate is re-scored, so the hits cannot be bounded below DEEP_CAP, and 8192 keys with 8192
// hits would not fit.  Counters are integer atomics; no floating-point atomic and no scalar-memory store is used.
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

namespace mirx {

namespace {

constexpr int64_t ID_LAST = INT64_MAX;
constexpr int DEEP_THREADS = 1024;
constexpr int DEEP_WAVES = DEEP_THREADS / WAVE;
constexpr size_t DEEP_LDS_BYTES = (size_t)DEEP_CAP * (sizeof(unsigned long long) + sizeof(Hit));
static_assert((DEEP_MAX_REGIONS + 1) * sizeof(int) <= DEEP_CAP * sizeof(Hit), "the region offsets live in the hits' storage");

template <int METRIC>
__global__ __launch_bounds__(DEEP_THREADS) void k_finalize_deep(FinalizeArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);                 // [DEEP_CAP]
    Hit *hits = reinterpret_cast<Hit *>(smem + (size_t)DEEP_CAP * sizeof(unsigned long long));   // [DEEP_CAP]
    int *roff = reinterpret_cast<int *>(hits);                     // [regions + 1] during the gather
    __shared__ int sh_wsum[DEEP_WAVES], sh_wraw[DEEP_WAVES];
    __shared__ int sh_ok, sh_m;
    __shared__ float sh_lo;
    const int slot_q = blockIdx.x;                                  // index into tau / candidate buffers
    const int qi = A.qmap ? A.qmap[slot_q] : slot_q;                // original query number
    const int wave = threadIdx.x >> 6, lane = lane_id();

    // ---- gather: prefix sum of the regions' takes; thread t owns the regions [t * per, (t + 1) * per)
    const int per = (A.regions + DEEP_THREADS - 1) / DEEP_THREADS;
    const int *rcnt = A.region_cnt + (int64_t)slot_q * A.regions;
    int mine = 0, raw = 0;
    for (int j = 0; j < per; ++j) {
        const int rg = threadIdx.x * per + j;
        if (rg < A.regions) {
            const int cr = rcnt[rg];
            raw += cr;
            mine += cr < A.slots ? cr : A.slots;
        }
    }
    int incl = mine;                                                // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int v = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += v;
    }
    raw = wave_isum(raw);
    if (lane == WAVE - 1) sh_wsum[wave] = incl;
    if (lane == 0) sh_wraw[wave] = raw;
    __syncthreads();
    int base = 0, c_reg = 0, c_raw = 0;
#pragma unroll
    for (int w = 0; w < DEEP_WAVES; ++w) {
        if (w < wave) base += sh_wsum[w];
        c_reg += sh_wsum[w];
        c_raw += sh_wraw[w];
    }
    {
        int at = base + incl - mine;                                // exclusive offset of this thread's first region
        for (int j = 0; j < per; ++j) {
            const int rg = threadIdx.x * per + j;
            if (rg < A.regions) {
                roff[rg] = at;
                const int cr = rcnt[rg];
                at += cr < A.slots ? cr : A.slots;
            }
        }
        if (threadIdx.x == 0) roff[A.regions] = c_reg;
    }
    const int oc = A.ovf_cnt[slot_q];
    const int otake = oc < CAND_OVF ? oc : CAND_OVF;
    // (a full overflow list has lost rows; the candidates of the regions and of the list share the one capacity)
    const bool overflow = oc > CAND_OVF || c_reg + otake > DEEP_CAP;
    const int c = overflow ? 0 : c_reg + otake;
    const int m2 = pow2_ceil(c > 1 ? c : 1);
    __syncthreads();
    auto key_of = [](const Cand cd) {
        return ((unsigned long long)f32_orderable(cd.s) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)cd.row);
    };
    if (!overflow) {
        const Cand *qcand = A.cand + (int64_t)slot_q * A.regions * A.slots;
        for (int i = threadIdx.x; i < c_reg; i += DEEP_THREADS) {
            int lo_r = 0, hi_r = A.regions;                         // the last region with roff[rg] <= i (empty regions share offsets)
            while (hi_r - lo_r > 1) {
                const int mid = (lo_r + hi_r) >> 1;
                if (roff[mid] <= i) lo_r = mid; else hi_r = mid;
            }
            keys[i] = key_of(qcand[(int64_t)lo_r * A.slots + (i - roff[lo_r])]);
        }
        for (int i = threadIdx.x; i < otake; i += DEEP_THREADS) keys[c_reg + i] = key_of(A.ovf[(int64_t)slot_q * CAND_OVF + i]);
        for (int i = c + threadIdx.x; i < m2; i += DEEP_THREADS) keys[i] = 0ull;
    }
    const int64_t ex = A.exclude ? A.exclude[qi] : -1;
    const int k_eff = A.k + (ex >= 0 ? 1 : 0);
    if (!overflow) bitonic_lds(keys, m2, [](unsigned long long x, unsigned long long y) { return x > y; });

    // ---- guard (k_finalize's, word for word)
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
                    // the k-th best s~ is final (every row above tau was seen), so tau2 just below `lo` makes the next filter
                    // pass complete by construction
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
        for (int i = threadIdx.x; i < c; i += DEEP_THREADS) n += f32_from_orderable((uint32_t)(keys[i] >> 32)) >= lo ? 1 : 0;
        n = wave_isum(n);
        if (lane == 0 && n) atomicAdd(&sh_m, n);
    }
    __syncthreads();
    const int m = sh_m;                                   // sorted, so these are keys[0..m)

    // ---- re-score in fp64, one row per wave and trip (the region offsets are dead: the hits take their storage)
    const float *qrow = A.q32p + (int64_t)qi * A.dimp;
    for (int i = wave; i < m; i += DEEP_WAVES) {
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)(keys[i] & 0xFFFFFFFFull);
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
    for (int i = m + threadIdx.x; i < mp; i += DEEP_THREADS) { hits[i].s = -INFINITY; hits[i].id = ID_LAST; }
    bitonic_lds(hits, mp, [](const Hit &x, const Hit &y) { return hit_before(x.s, x.id, y.s, y.id); });
    for (int r = threadIdx.x; r < A.k; r += DEEP_THREADS) {
        Hit h;
        h.s = -INFINITY;
        h.id = ID_LAST;
        if (r < mp) h = hits[r];
        const bool empty = h.id == ID_LAST;
        const int64_t o = (int64_t)qi * A.k + r;
        if (A.out_f64) A.out_f64[o] = empty ? -INFINITY : h.s;
        A.out_ids[o] = empty ? -1 : h.id;
        if (A.out_val) {
            float v = -INFINITY;
            if (!empty) v = METRIC == 0 ? (float)h.s : (float)(-sqrt(fmax(-h.s, 0.0)));
            A.out_val[o] = v;
        }
    }
    if (threadIdx.x == 0) {
        atomicAdd((unsigned long long *)&A.stats->tier1_answered, 1ull);
        atomicAdd((unsigned long long *)&A.stats->candidates, (unsigned long long)c_raw);
        atomicAdd((unsigned long long *)&A.stats->reranked, (unsigned long long)m);
    }
}

}  // namespace

hipError_t launch_finalize_deep(const FinalizeArgs &a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (a.regions < 1 || a.regions > DEEP_MAX_REGIONS || a.slots < 1 || a.k < 1 || a.k > MAX_K) return hipErrorInvalidValue;
    hipError_t e;
    if (a.metric == MIRX_METRIC_IP) {
        static std::atomic<unsigned long long> attr_devs{0};
        if ((e = set_dynamic_lds(k_finalize_deep<0>, DEEP_LDS_BYTES, &attr_devs)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_finalize_deep<0>, dim3(a.nq), dim3(DEEP_THREADS), DEEP_LDS_BYTES, st, a);
    } else {
        static std::atomic<unsigned long long> attr_devs{0};
        if ((e = set_dynamic_lds(k_finalize_deep<1>, DEEP_LDS_BYTES, &attr_devs)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_finalize_deep<1>, dim3(a.nq), dim3(DEEP_THREADS), DEEP_LDS_BYTES, st, a);
    }
    return hipGetLastError();
}

}  // namespace mirx
