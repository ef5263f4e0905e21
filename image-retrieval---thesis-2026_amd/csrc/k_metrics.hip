// k_metrics.hip -- the ranked-list metric tail on the device.
//
// One wavefront walks one query's ranking (best first) 64 ids at a time and produces, in one pass:
//   * AP, trapezoidal (compute_ap test.py:58-92 as summed by compute_map test.py:95-146) or
//     standard (sum of precision at each relevant rank / relevant count: compute_map_multilabel
//     test.py:941-985, fusion_eval/metrics.py:41-94),
//   * the number of relevant items within the first kappa ranks for up to 8 kappas
//     (retrieval_accuracy test.py:38-54; the precision@kappa of test.py:137-142 and the mP@k / R@k
//     of fusion_eval/metrics.py are ratios of these),
//   * the relevant count of the list and the largest 1-based relevant rank (the reference's
//     kq = min(max(pos), kappa) quirk needs it).
// Relevance is label equality (int64) or Jaccard(multi-hot bit masks) > threshold, evaluated as
// inter / (union + 1e-8) > thr in fp64 like test.py:958-961; an optional per-query id is never relevant
// (self-exclusion).  Sums are fp64, per-lane partials combined by a fixed butterfly: deterministic.
// An entry can be taken out of its list -- the query's own (drop_self), or with CODES every entry that carries the query's
// group code (leave-group-out, mirx_rank_metrics_grouped): it has no position, later ranks move up.
// The second half of the file is the same walk cut into segments, for the few long lists of one radix-ranking batch
// (mirx_index_rank_metrics): it reads the sort's row payload and never sees a ranking in memory.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

// Relevance of a gallery label for the query's: equality, or Jaccard of the bit masks above the threshold (qbits = |qlab|).
template <int REL_KIND>
__device__ inline bool label_relevant(int64_t glab, int64_t qlab, double qbits, double thr) {
    if (REL_KIND == 0) return glab == qlab;
    const double inter = (double)__popcll((unsigned long long)(glab & qlab));
    const double uni = qbits + (double)__popcll((unsigned long long)glab) - inter;
    return inter / (uni + 1e-8) > thr;
}

// One relevant entry's share of the AP: 0-based position reff in the list (after removals), j positives before it.
template <int AP_KIND>
__device__ inline double ap_term(int64_t reff, double j) {
    const double rr = (double)reff;
    const double p1 = (j + 1.0) / (rr + 1.0);
    if (AP_KIND == 1) return p1;
    const double p0 = reff == 0 ? 1.0 : j / rr;
    return (p0 + p1) * 0.5;
}

// CODES (mirx_rank_metrics_grouped): an entry whose id carries the query's code leaves the list exactly like a dropped self entry.
template <int REL_KIND, int AP_KIND, bool CODES>
__global__ __launch_bounds__(256) void k_rank_metrics(RankMetricsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.nq) return;
    const int64_t *row = a.ranks + q * a.row_stride;
    const int64_t qlab = a.query_labels[q];
    const int64_t self = a.query_ids ? a.query_ids[q] : -1;
    const int32_t qcode = CODES ? a.query_codes[q] : -1;
    const double qbits = REL_KIND == 1 ? (double)__popcll((unsigned long long)qlab) : 0.0;
    double acc = 0.0;
    int64_t running = 0, maxpos = 0;
    int64_t cnt[MIRX_MAX_KAPPAS];
#pragma unroll
    for (int j = 0; j < MIRX_MAX_KAPPAS; ++j) cnt[j] = 0;

    int64_t dropped = 0;                                     // entries already passed that left the list (drop_self, CODES)
    for (int64_t i = 0; i < a.n; i += 64) {
        const int64_t r = i + lane;
        bool rel = false, out = false;
        if (r < a.n) {
            const int64_t id = row[r];
            const bool is_self = id == self;
            const bool known = id >= 0 && id < a.n_labels;
            const bool in_group = CODES && known && qcode >= 0 && a.gallery_codes[id] == qcode;
            out = (a.drop_self && is_self) || in_group;
            if (known && !is_self && !in_group) rel = label_relevant<REL_KIND>(a.gallery_labels[id], qlab, qbits, a.jaccard_threshold);
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long smask = (CODES || a.drop_self) ? __ballot(out) : 0ull;
        const unsigned long long mask = __ballot(rel);
        // 0-based position in the list with the query's own entry taken out (fusion_eval/metrics.py:58-60)
        const int64_t reff = r - dropped - __popcll(smask & below);
        if (mask != 0) {
            if (rel) acc += ap_term<AP_KIND>(reff, (double)(running + __popcll(mask & below)));   // positives before
#pragma unroll
            for (int j = 0; j < MIRX_MAX_KAPPAS; ++j)
                if (j < a.nk) cnt[j] += __popcll(__ballot(rel && reff < (int64_t)a.kappas[j]));
            running += __popcll(mask);
            maxpos = __shfl(reff, 63 - __clzll((long long)mask), 64) + 1;
        }
        dropped += __popcll(smask);
    }
    acc = wave_butterfly_sum(acc);
    if (lane == 0) {
        a.out_ap[q] = running > 0 ? acc / (double)running : __longlong_as_double(0x7ff8000000000000ll);
        a.out_nrel[q] = running;
        a.out_maxpos[q] = maxpos;
        for (int j = 0; j < a.nk; ++j) a.out_cnt[q * a.nk + j] = cnt[j];
    }
}

// ---- the same walk, parallel along the list (mirx_index_rank_metrics) -------------------------------------------------------
// A block of 256 threads owns one segment of one query's list and passes over it 256 entries at a time, in list order.

// Entry r of query q's list: is it taken out of the list, is it relevant?
template <int REL_KIND>
__device__ inline void walk_classify(const RankWalkArgs &a, int q, int64_t r, int64_t qlab, double qbits, int64_t ex, bool has_ex,
                                     int32_t qcode, bool &rel, bool &out) {
    const int32_t row = a.pay[(int64_t)q * a.n + r];
    const bool is_ex = has_ex && a.ids[row] == ex;
    out = (a.self_kind == 2 && is_ex) || (qcode >= 0 && a.row_codes[row] == qcode);
    rel = !out && !is_ex && label_relevant<REL_KIND>(a.row_labels[row], qlab, qbits, a.jaccard_threshold);
}

struct WalkQuery {
    int64_t qlab, ex;
    double qbits;
    int32_t qcode;
    bool has_ex;
};
template <int REL_KIND>
__device__ inline WalkQuery walk_query(const RankWalkArgs &a, int q) {
    WalkQuery w;
    w.qlab = a.query_labels[q];
    w.qbits = REL_KIND == 1 ? (double)__popcll((unsigned long long)w.qlab) : 0.0;
    w.has_ex = a.exclude != nullptr && a.self_kind != 0;       // self_kind 0: the excluded row is an entry like any other
    w.ex = w.has_ex ? a.exclude[q] : 0;
    w.qcode = a.query_codes ? a.query_codes[q] : -1;
    return w;
}

template <int REL_KIND>
__global__ __launch_bounds__(256) void k_rank_walk_count(RankWalkArgs a) {
    __shared__ int sh[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = blockIdx.x, q = blockIdx.y;
    const WalkQuery w = walk_query<REL_KIND>(a, q);
    const int64_t s0 = (int64_t)seg * a.seg_len, s1 = min(s0 + a.seg_len, a.n);
    int n_out = 0, n_rel = 0;                                  // of this wave's entries
    for (int64_t base = s0; base < s1; base += 256) {
        const int64_t r = base + threadIdx.x;
        bool rel = false, out = false;
        if (r < s1) walk_classify<REL_KIND>(a, q, r, w.qlab, w.qbits, w.ex, w.has_ex, w.qcode, rel, out);
        n_out += __popcll(__ballot(out));
        n_rel += __popcll(__ballot(rel));
    }
    if (lane == 0) { sh[wave][0] = n_out; sh[wave][1] = n_rel; }
    __syncthreads();
    if (threadIdx.x < 2)
        a.seg_cnt[((int64_t)q * a.nseg + seg) * 2 + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

template <int REL_KIND, int AP_KIND>
__global__ __launch_bounds__(256) void k_rank_walk_terms(RankWalkArgs a) {
    __shared__ long long sh_pre[4][2];
    __shared__ int sh_step[2][4][2];
    __shared__ double sh_acc[4];
    __shared__ long long sh_max[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = blockIdx.x, q = blockIdx.y;
    const WalkQuery w = walk_query<REL_KIND>(a, q);
    const int64_t s0 = (int64_t)seg * a.seg_len, s1 = min(s0 + a.seg_len, a.n);

    // entries taken out and relevant entries of the segments before this one (integer sums: any order gives the same value)
    long long p_out = 0, p_rel = 0;
    const int32_t *sc = a.seg_cnt + (int64_t)q * a.nseg * 2;
    for (int s = threadIdx.x; s < seg; s += 256) { p_out += sc[2 * s]; p_rel += sc[2 * s + 1]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { p_out += __shfl_xor(p_out, off, 64); p_rel += __shfl_xor(p_rel, off, 64); }
    if (lane == 0) { sh_pre[wave][0] = p_out; sh_pre[wave][1] = p_rel; }
    __syncthreads();
    int64_t out_before = sh_pre[0][0] + sh_pre[1][0] + sh_pre[2][0] + sh_pre[3][0];
    int64_t rel_before = sh_pre[0][1] + sh_pre[1][1] + sh_pre[2][1] + sh_pre[3][1];

    int max_kappa = 0;
    for (int j = 0; j < a.nk; ++j) max_kappa = max(max_kappa, a.kappas[j]);
    double acc = 0.0;
    int64_t last = 0;                                          // this thread's largest 1-based relevant position
    int cnt[MIRX_MAX_KAPPAS];                                  // this wave's hits below each kappa
#pragma unroll
    for (int j = 0; j < MIRX_MAX_KAPPAS; ++j) cnt[j] = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    int par = 0;
    for (int64_t base = s0; base < s1; base += 256, par ^= 1) {
        const int64_t r = base + threadIdx.x;
        bool rel = false, out = false;
        if (r < s1) walk_classify<REL_KIND>(a, q, r, w.qlab, w.qbits, w.ex, w.has_ex, w.qcode, rel, out);
        const unsigned long long omask = __ballot(out), rmask = __ballot(rel);
        if (lane == 0) { sh_step[par][wave][0] = __popcll(omask); sh_step[par][wave][1] = __popcll(rmask); }
        __syncthreads();   // the step after the next one reuses this buffer, and no wave gets there before all have read it here
        int o_lo = 0, r_lo = 0, o_all = 0, r_all = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int o = sh_step[par][v][0], p = sh_step[par][v][1];
            if (v < wave) { o_lo += o; r_lo += p; }
            o_all += o; r_all += p;
        }
        const int64_t reff = r - out_before - o_lo - __popcll(omask & below);   // 0-based position after removals
        if (rel) {
            acc += ap_term<AP_KIND>(reff, (double)(rel_before + r_lo + __popcll(rmask & below)));
            last = reff + 1;
        }
        if (base - out_before < max_kappa) {                   // positions only grow: later steps of a list are past every kappa
#pragma unroll
            for (int j = 0; j < MIRX_MAX_KAPPAS; ++j)
                if (j < a.nk) cnt[j] += __popcll(__ballot(rel && reff < (int64_t)a.kappas[j]));
        }
        out_before += o_all;
        rel_before += r_all;
    }
    acc = wave_butterfly_sum(acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) last = max(last, (int64_t)__shfl_xor((long long)last, off, 64));
    if (lane == 0) {
        sh_acc[wave] = acc;
        sh_max[wave] = last;
        for (int j = 0; j < a.nk; ++j)
            if (cnt[j]) atomicAdd(a.out_cnt + (int64_t)q * a.nk + j, (unsigned long long)cnt[j]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.seg_ap[(int64_t)q * a.nseg + seg] = ((sh_acc[0] + sh_acc[1]) + sh_acc[2]) + sh_acc[3];
        a.seg_max[(int64_t)q * a.nseg + seg] = max(max(sh_max[0], sh_max[1]), max(sh_max[2], sh_max[3]));
    }
}

// One wavefront per query: lane l adds segments l, l + 64, .. in that order, then the butterfly.
__global__ __launch_bounds__(64) void k_rank_walk_finish(RankWalkArgs a) {
    const int lane = threadIdx.x, q = blockIdx.x;
    double acc = 0.0;
    long long nrel = 0, maxpos = 0;
    for (int s = lane; s < a.nseg; s += 64) {
        const int64_t i = (int64_t)q * a.nseg + s;
        acc += a.seg_ap[i];
        nrel += a.seg_cnt[2 * i + 1];
        maxpos = max(maxpos, (long long)a.seg_max[i]);
    }
    acc = wave_butterfly_sum(acc);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        nrel += __shfl_xor(nrel, off, 64);
        maxpos = max(maxpos, __shfl_xor(maxpos, off, 64));
    }
    if (lane == 0) {
        a.out_ap[q] = nrel > 0 ? acc / (double)nrel : __longlong_as_double(0x7ff8000000000000ll);
        a.out_nrel[q] = nrel;
        a.out_maxpos[q] = maxpos;
    }
}

}  // namespace

hipError_t launch_rank_metrics(const RankMetricsArgs &a, int rel_kind, int ap_kind, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.nq + 3) / 4));
#define MIRX_RM(R, P)                                                                                      \
    do {                                                                                                   \
        if (a.gallery_codes) hipLaunchKernelGGL((k_rank_metrics<R, P, true>), grid, dim3(256), 0, st, a);  \
        else hipLaunchKernelGGL((k_rank_metrics<R, P, false>), grid, dim3(256), 0, st, a);                 \
    } while (0)
    if (rel_kind == 0) { if (ap_kind == 0) MIRX_RM(0, 0); else MIRX_RM(0, 1); }
    else               { if (ap_kind == 0) MIRX_RM(1, 0); else MIRX_RM(1, 1); }
#undef MIRX_RM
    return hipGetLastError();
}

int64_t rank_walk_segment(int64_t n) {
    const int64_t unit = 4096;
    return unit * std::max<int64_t>(1, (n + unit * 1024 - 1) / (unit * 1024));
}

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

size_t rank_walk_workspace_bytes(int64_t per, int64_t n) {
    const int64_t seg = rank_walk_segment(n);
    const size_t cells = (size_t)per * (size_t)((n + seg - 1) / seg);
    return align256(cells * 2 * sizeof(int32_t)) + 2 * align256(cells * 8);
}

void rank_walk_carve(RankWalkArgs &a, void *workspace, int64_t per) {
    a.seg_len = rank_walk_segment(a.n);
    a.nseg = (int)((a.n + a.seg_len - 1) / a.seg_len);
    const size_t cells = (size_t)per * (size_t)a.nseg;
    char *p = static_cast<char *>(workspace);
    a.seg_cnt = reinterpret_cast<int32_t *>(p);
    p += align256(cells * 2 * sizeof(int32_t));
    a.seg_ap = reinterpret_cast<double *>(p);
    p += align256(cells * 8);
    a.seg_max = reinterpret_cast<int64_t *>(p);
}

hipError_t launch_rank_walk(const RankWalkArgs &a, int rel_kind, int ap_kind, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (a.nk > 0) {
        hipError_t e = hipMemsetAsync(a.out_cnt, 0, (size_t)a.nq * a.nk * sizeof(unsigned long long), st);
        if (e != hipSuccess) return e;
    }
    if (a.nseg > 0) {
        const dim3 grid((unsigned)a.nseg, (unsigned)a.nq);
        if (rel_kind == 0) hipLaunchKernelGGL((k_rank_walk_count<0>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_rank_walk_count<1>), grid, dim3(256), 0, st, a);
#define MIRX_RW(R, P) hipLaunchKernelGGL((k_rank_walk_terms<R, P>), grid, dim3(256), 0, st, a)
        if (rel_kind == 0) { if (ap_kind == 0) MIRX_RW(0, 0); else MIRX_RW(0, 1); }
        else               { if (ap_kind == 0) MIRX_RW(1, 0); else MIRX_RW(1, 1); }
#undef MIRX_RW
    }
    hipLaunchKernelGGL(k_rank_walk_finish, dim3((unsigned)a.nq), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace mirx
