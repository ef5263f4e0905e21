// k_rerank.hip -- lesion-aware re-ranking of a full base ranking (the reference's ChestMIR/chestmir_eval.py
// rerank_with_specific_lesion / rerank_with_adaptive_lesion), all stages of a dataset in one launch.
//
//   k_lesion_rerank   one workgroup of 4 waves per (query, stage).  The query's region vector is staged in LDS.  Wave w takes
//                     the candidates c = w, w + 4, ... of the query's first `topk` base positions: the base score (given, or the
//                     fp64 dot of the two global vectors), then the candidate's CSR segment, regions of other lesions skipped on
//                     the lesion id alone, the fp64 dot of every region of the chosen lesion, their maximum (-1.0 when there is
//                     none), combined = w * base + (1 - w) * region.  The workgroup counts the candidates with region >= 0.
//                     No query vector or no counted candidate: the base row is copied.  Otherwise a bitonic sort of the
//                     candidate positions in LDS on (combined desc, base desc, base position asc), the sorted ids written in
//                     front and the base tail copied behind them.
//
// Every dot product is summed in one fixed order: lane l adds the products of elements l, l + 64, ... in ascending order
// (each product exact: two floats widened to double), then a butterfly over lane distances 32, 16, 8, 4, 2, 1.  The order
// depends on the vector length alone, so a (query, stage) result does not depend on the number of stages, on the launch
// shape or on any other query.  No atomics; nothing is accumulated across workgroups.
#include <cmath>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_WAVES = RR_THREADS / 64;

// fp64 dot of two float vectors of length d by one wave (every lane returns the sum)
__device__ inline double rr_dot(const float *a, const float *b, int d, int lane) {
    double p = 0.0;
    for (int t = lane; t < d; t += 64) p = p + (double)a[t] * (double)b[t];
    return wave_butterfly_sum(p);
}

struct RerankArgs {
    const int64_t *base_ids;      // [n, n] row = query
    const double *base_sim;       // [n, n] row = query, column = gallery id; or null: recompute from gvec
    const float *gvec;            // [n, d]
    const int64_t *row_ptr;       // [n + 1]
    const int32_t *region_lesion; // [n_regions]
    const float *region_vec;      // [n_regions, dr]
    const int32_t *q_lesion;      // [stages, n]
    const int64_t *q_region;      // [stages, n]
    int64_t *out_ids;             // [stages, n, n]
    int32_t *out_matched;         // [stages, n]
    int32_t *out_reranked;        // [stages, n]
    int64_t n, n_regions;
    int d, dr, topk, p2;
    double gw;
};

__global__ __launch_bounds__(RR_THREADS) void k_lesion_rerank(const RerankArgs a) {
    __shared__ float s_q[MIRX_RERANK_MAX_DR];
    __shared__ double s_comb[MIRX_RERANK_MAX_TOPK];
    __shared__ double s_base[MIRX_RERANK_MAX_TOPK];
    __shared__ int64_t s_id[MIRX_RERANK_MAX_TOPK];
    __shared__ int s_perm[MIRX_RERANK_MAX_TOPK];
    __shared__ unsigned char s_hit[MIRX_RERANK_MAX_TOPK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x, s = blockIdx.y;
    const int64_t n = a.n;
    const int topk = a.topk;
    const int64_t *base_row = a.base_ids + q * n;
    int64_t *out_row = a.out_ids + (s * n + q) * n;

    const int lesion = a.q_lesion[s * n + q];
    int64_t qr = a.q_region[s * n + q];
    if (qr >= a.n_regions) qr = -1;                        // an index outside the store counts as "no vector"
    int matched = 0;
    if (qr >= 0) {                                         // uniform over the workgroup
        for (int t = tid; t < a.dr; t += RR_THREADS) s_q[t] = a.region_vec[qr * a.dr + t];
        __syncthreads();
        const double gr = 1.0 - a.gw;
        for (int c = wave; c < topk; c += RR_WAVES) {
            const int64_t j = base_row[c];
            const bool ok = j >= 0 && j < n;               // ids outside the gallery have no vectors: base 0, no region
            double base = 0.0;
            if (ok) base = a.base_sim ? a.base_sim[q * n + j] : rr_dot(a.gvec + q * a.d, a.gvec + j * a.d, a.d, lane);
            int64_t lo = 0, hi = 0;
            if (ok) {
                lo = a.row_ptr[j];
                hi = a.row_ptr[j + 1];
                if (lo < 0) lo = 0;
                if (hi > a.n_regions) hi = a.n_regions;
            }
            bool has = false;
            double best = -1.0;
            for (int64_t r = lo; r < hi; ++r) {
                if (a.region_lesion[r] != lesion) continue;
                const double v = rr_dot(s_q, a.region_vec + r * a.dr, a.dr, lane);
                if (!has || v > best) best = v;            // Python's max(): the first value, then strictly larger ones
                has = true;
            }
            if (lane == 0) {
                s_comb[c] = a.gw * base + gr * best;
                s_base[c] = base;
                s_id[c] = j;
                s_hit[c] = best >= 0.0 ? 1 : 0;
            }
        }
        __syncthreads();
        for (int c0 = 0; c0 < topk; c0 += RR_THREADS) {
            const int c = c0 + tid;
            matched += __syncthreads_count(c < topk && s_hit[c]);
        }
    }
    const bool rerank = matched > 0;
    if (tid == 0) {
        a.out_matched[s * n + q] = matched;
        a.out_reranked[s * n + q] = rerank ? 1 : 0;
    }
    if (!rerank) {
        for (int64_t t = tid; t < n; t += RR_THREADS) out_row[t] = base_row[t];
        return;
    }
    // bitonic sort of the positions 0 .. p2 (positions >= topk are padding and sort last)
    const int p2 = a.p2;
    for (int t = tid; t < p2; t += RR_THREADS) s_perm[t] = t;
    __syncthreads();
    auto before = [&](int x, int y) -> bool {
        if (x >= topk || y >= topk) return x < y;
        const double cx = s_comb[x], cy = s_comb[y];
        if (cx != cy) return cx > cy;
        const double bx = s_base[x], by = s_base[y];
        if (bx != by) return bx > by;
        return x < y;
    };
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (p2 >> 1); t += RR_THREADS) {
                const int i = 2 * t - (t & (j - 1));       // bit j clear
                const int l = i | j;
                const int x = s_perm[i], y = s_perm[l];
                const bool up = (i & k) == 0;
                if (up ? before(y, x) : before(x, y)) {
                    s_perm[i] = y;
                    s_perm[l] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < topk; t += RR_THREADS) out_row[t] = s_id[s_perm[t]];
    for (int64_t t = topk + tid; t < n; t += RR_THREADS) out_row[t] = base_row[t];
}

inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

}  // namespace mirx

using namespace mirx;

extern "C" int mirx_lesion_rerank(const int64_t *base_ids, int64_t n, const double *base_sim_or_null, const float *gvec_or_null, int d,
                                  const int64_t *row_ptr, const int32_t *region_lesion, const float *region_vec, int64_t n_regions, int dr,
                                  const int32_t *q_lesion, const int64_t *q_region, int n_stages, int topk, double global_weight,
                                  int64_t *out_ids, int32_t *out_matched, int32_t *out_reranked, void *stream) {
    if (n < 2 || n > MIRX_RERANK_MAX_N) return fail(MIRX_EINVAL, "lesion_rerank: n must be in [2, 65536]");
    if (dr < 1 || dr > MIRX_RERANK_MAX_DR) return fail(MIRX_EINVAL, "lesion_rerank: dr must be in [1, 4096]");
    if (topk < 1 || topk > MIRX_RERANK_MAX_TOPK || topk > n - 1)
        return fail(MIRX_EINVAL, "lesion_rerank: topk must be in [1, min(1024, n - 1)]");
    if (n_stages < 0 || n_stages > MIRX_RERANK_MAX_STAGES) return fail(MIRX_EINVAL, "lesion_rerank: n_stages must be in [0, 65535]");
    if (!(global_weight >= 0.0 && global_weight <= 1.0)) return fail(MIRX_EINVAL, "lesion_rerank: global_weight must be in [0, 1]");
    if (n_regions < 0 || n_regions > MIRX_RERANK_MAX_REGIONS) return fail(MIRX_EINVAL, "lesion_rerank: n_regions must be in [0, 2^31 - 1]");
    if (!base_sim_or_null && (!gvec_or_null || d < 1 || d > MIRX_RERANK_MAX_D))
        return fail(MIRX_EINVAL, "lesion_rerank: without base_sim the global vectors are needed, d in [1, 65536]");
    if (!base_ids || !row_ptr || !q_lesion || !q_region || !out_ids || !out_matched || !out_reranked)
        return fail(MIRX_EINVAL, "lesion_rerank: null buffer");
    if (n_regions > 0 && (!region_lesion || !region_vec)) return fail(MIRX_EINVAL, "lesion_rerank: null region store");
    if (!aligned8(base_ids) || !aligned8(base_sim_or_null) || !aligned8(row_ptr) || !aligned8(q_region) || !aligned8(out_ids) ||
        !aligned4(gvec_or_null) || !aligned4(region_lesion) || !aligned4(region_vec) || !aligned4(q_lesion) || !aligned4(out_matched) ||
        !aligned4(out_reranked))
        return fail(MIRX_EINVAL, "lesion_rerank: misaligned buffer");
    if (n_stages == 0) return MIRX_OK;
    RerankArgs a;
    a.base_ids = base_ids;
    a.base_sim = base_sim_or_null;
    a.gvec = gvec_or_null;
    a.row_ptr = row_ptr;
    a.region_lesion = region_lesion;
    a.region_vec = region_vec;
    a.q_lesion = q_lesion;
    a.q_region = q_region;
    a.out_ids = out_ids;
    a.out_matched = out_matched;
    a.out_reranked = out_reranked;
    a.n = n;
    a.n_regions = n_regions;
    a.d = d;
    a.dr = dr;
    a.topk = topk;
    a.p2 = 2;
    while (a.p2 < topk) a.p2 <<= 1;
    a.gw = global_weight;
    hipLaunchKernelGGL(k_lesion_rerank, dim3((unsigned)n, (unsigned)n_stages), dim3(RR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}
