// mirx_api.hip -- the C ABI (include/mirx.h): index object, search orchestration.
//
// A search is a fixed sequence of launches on the caller's stream:
//   prep queries -> [group-max GEMM on a strided row sample -> thresholds] -> filter GEMM
//   -> finalize (sort candidates, completeness guard, fp64 re-rank, top-k)
//   -> exact scan (fp64 score tiles + row top-k) for the queries the guard rejected.
// The only host<->device synchronisation is one read of the rejected-query count.
// A masked search (mirx_index_search_masked) runs the same sequence over a SearchRows that stands for the allowed rows.
// A range search (mirx_index_range_search) runs prep -> threshold from the radius -> filter GEMM -> its own finalize, the radix
// ranking for what that cannot answer, and a CSR assembly (k_range.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <mutex>
#include <vector>

#include "mirx_kernels.h"

namespace mirx {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

static inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            bytes = 0;
            if (e != hipSuccess) return e;
        }
        size_t want = need + need / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, need);
            want = need;
        }
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

}  // namespace mirx

using namespace mirx;

// What a search scans.  The index itself for the plain calls; a masked call passes a stand-in for its allowed rows:
//   tier 1    the index's rows with `bias` (-inf on masked rows) in the sample and filter GEMMs, and for the queries the guard
//             rejects the exact scan over all rows with the masked ones neutralised (mpos, ids = the masked ids)
//   exact     either that neutralised scan, or g32 / ids = the allowed rows gathered into scratch, n of them
struct SearchRows {
    const float *g32 = nullptr;           // rows the exact scan scores
    const int64_t *ids = nullptr;         // their ids (INT64_MAX on a masked row when mpos is set)
    int64_t n = 0;
    const int32_t *mpos = nullptr;        // scanned keep positions (n + 1): row r is masked iff mpos[r + 1] == mpos[r]
    const float *bias = nullptr;          // tier 1: the per-row bias of both GEMMs instead of the index's
    bool tier1 = false;
};

struct mirx_index {
    int dim = 0, dimp = 0, metric = 0, device = 0;
    int64_t size = 0, cap = 0;
    float *g32 = nullptr;
    uint16_t *g16 = nullptr;
    int64_t *ids = nullptr;
    float *gbias = nullptr;
    unsigned *gnorm_max_bits = nullptr;   // device scalar
    // options
    int tiers = MIRX_TIER_AUTO;
    int sample_rank = 8;
    uint32_t force_tau_bits = 0x7fc00000u;
    int profile = 0;
    int rank_sort = MIRX_RANK_SORT_AUTO;
    // the radix ranking starts from the rows in (id, row) order: the identity while ids ascend with the row (always, for auto ids),
    // else a permutation built on first use and dropped by every add
    bool ids_ascend = true;
    int64_t last_id = INT64_MIN;
    bool idperm_valid = false;
    int64_t next_auto = 0;                // auto ids go on from here: past the rows removed since (never below `size`)
    int64_t compact_chunk = 0;            // MIRX_OPT_COMPACT_CHUNK_ROWS; 0 = as many rows as COMPACT_SCRATCH_BYTES hold
    int64_t mask_gather_bytes = -1;       // MIRX_OPT_MASK_GATHER_BYTES; -1 = EXACT_WS_BYTES
    int64_t range_max_hits = 0;           // MIRX_OPT_RANGE_MAX_HITS; 0 = RANGE_MAX_HITS
    // the last range search: its hits stay in rres until mirx_index_range_fetch; any other use of the index drops them
    bool range_valid = false;
    int64_t range_total = 0;
    mirx_range_stats range_stats{};
    unsigned long long *range_stats_dev = nullptr;   // [2] filter-answered queries, candidates
    int64_t *range_total_dev = nullptr;              // [1] what the scan leaves
    int64_t *range_total_host = nullptr;             // pinned
    std::vector<hipEvent_t> ev_pool;      // lazily created, reused
    struct Span { int stage; hipEvent_t a, b; };
    std::vector<Span> spans;              // of the last search
    size_t ev_used = 0;
    // workspace
    DevBuf q32p, q16, qnorm, tau, cnt, cand, ovf_cnt, ovf, groupmax, fail_list, retry_list, tau2, q16r, taur,
        scores, stage, rankwork, spill, rkeys, rpay, rhist, idperm, creq, cpos, cpart, mallow, mbias, mids, mrows,
        rstage, rcount, rxoff, rfirst, rexcl, rseg, rres;
    int *fail_count = nullptr;            // device
    mirx_search_stats *stats_dev = nullptr;
    int *fail_count_host = nullptr;       // pinned
    mirx_search_stats stats_host{};
    // a search whose first pass is enqueued and whose counters have not been read yet (search_begin / search_end)
    struct Pending {
        bool active = false;
        int64_t nb = 0;
        int k = 0;
        const int64_t *exb = nullptr;
        double *ofb = nullptr;
        int64_t *oib = nullptr;
        float *ovb = nullptr;
        hipStream_t st = nullptr;
        mirx::GemmArgs ga{};
        mirx::FinalizeArgs fa{};
        SearchRows rows{};
    } pend;
    hipEvent_t pend_ev = nullptr;
    bool begun = false;                   // between mirx_index_search_begin and _end, whether or not a pass is pending
};

namespace {

constexpr int64_t QUERY_BATCH = 8192;          // queries per internal pass
constexpr int64_t TIER1_MIN_ROWS = 32768;      // below this the exact scan answers directly
constexpr int TIER1_MAX_K = 64;
constexpr size_t EXACT_WS_BYTES = (size_t)1 << 30;   // fp64 score tile workspace per pass
constexpr size_t COMPACT_SCRATCH_BYTES = (size_t)256 << 20;   // most a removal's chunk scratch takes by default

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int is_device_pointer(const void *p, bool *dev) {
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // unregistered host memory reports an error: treat as host
        *dev = false;
        return MIRX_OK;
    }
    *dev = (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
    return MIRX_OK;
}

int grow(mirx_index *ix, int64_t want_rows) {
    if (want_rows <= ix->cap) return MIRX_OK;
    int64_t ncap = std::max<int64_t>(ix->cap * 2, want_rows);
    ncap = round_up(std::max<int64_t>(ncap, ROW_ALIGN), ROW_ALIGN);
    float *n32 = nullptr;
    uint16_t *n16 = nullptr;
    int64_t *nid = nullptr;
    float *nb = nullptr;
    const size_t b32 = (size_t)ncap * ix->dimp * sizeof(float);
    const size_t b16 = (size_t)ncap * ix->dimp * sizeof(uint16_t);
    hipError_t e;
    if ((e = hipMalloc(&n32, b32)) != hipSuccess || (e = hipMalloc(&n16, b16)) != hipSuccess ||
        (e = hipMalloc(&nid, (size_t)ncap * sizeof(int64_t))) != hipSuccess ||
        (e = hipMalloc(&nb, (size_t)ncap * sizeof(float))) != hipSuccess) {
        if (n32) (void)hipFree(n32);
        if (n16) (void)hipFree(n16);
        if (nid) (void)hipFree(nid);
        if (nb) (void)hipFree(nb);
        return fail(MIRX_ENOMEM, std::string("index grow: ") + hipGetErrorString(e));
    }
    // rows past `size` must read as zeros (tiles run over the padded tail)
    MIRX_HIP(hipMemset(n32, 0, b32));
    MIRX_HIP(hipMemset(n16, 0, b16));
    MIRX_HIP(hipMemset(nid, 0xFF, (size_t)ncap * sizeof(int64_t)));
    MIRX_HIP(hipMemset(nb, 0, (size_t)ncap * sizeof(float)));
    if (ix->size > 0) {
        MIRX_HIP(hipMemcpy(n32, ix->g32, (size_t)ix->size * ix->dimp * sizeof(float), hipMemcpyDeviceToDevice));
        MIRX_HIP(hipMemcpy(n16, ix->g16, (size_t)ix->size * ix->dimp * sizeof(uint16_t), hipMemcpyDeviceToDevice));
        MIRX_HIP(hipMemcpy(nid, ix->ids, (size_t)ix->size * sizeof(int64_t), hipMemcpyDeviceToDevice));
        MIRX_HIP(hipMemcpy(nb, ix->gbias, (size_t)ix->size * sizeof(float), hipMemcpyDeviceToDevice));
    }
    if (ix->g32) (void)hipFree(ix->g32);
    if (ix->g16) (void)hipFree(ix->g16);
    if (ix->ids) (void)hipFree(ix->ids);
    if (ix->gbias) (void)hipFree(ix->gbias);
    ix->g32 = n32;
    ix->g16 = n16;
    ix->ids = nid;
    ix->gbias = nb;
    ix->cap = ncap;
    return MIRX_OK;
}

struct StageTimer {
    mirx_index *ix;
    hipStream_t st;
    int stage;
    hipEvent_t a = nullptr, b = nullptr;
    StageTimer(mirx_index *ix_, hipStream_t st_, int stage_) : ix(ix_), st(st_), stage(stage_) {
        if (!ix->profile) return;
        a = next();
        b = next();
        if (a && b) (void)hipEventRecord(a, st);
    }
    hipEvent_t next() {
        if (ix->ev_used == ix->ev_pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            ix->ev_pool.push_back(e);
        }
        return ix->ev_pool[ix->ev_used++];
    }
    ~StageTimer() {
        if (a && b) {
            (void)hipEventRecord(b, st);
            ix->spans.push_back({stage, a, b});
        }
    }
};

// Exact scan for `nlist` queries given by a device list (or 0..nlist-1 when list == null).
int exact_pass(mirx_index *ix, const SearchRows &sr, const float *q32p, const int32_t *list_dev, int64_t nlist, int k,
               const int64_t *exclude, double *out_f64, int64_t *out_ids, float *out_val,
               hipStream_t st) {
    if (nlist <= 0) return MIRX_OK;
    const int64_t ld = round_up(std::max<int64_t>(sr.n, 1), 64);
    int64_t per = (int64_t)(EXACT_WS_BYTES / ((size_t)ld * sizeof(double)));
    per = std::max<int64_t>(4, std::min<int64_t>(per, 4096)) / 4 * 4;
    per = std::min<int64_t>(per, round_up(nlist, 4));
    MIRX_HIP(ix->scores.ensure((size_t)per * ld * sizeof(double)));
    for (int64_t b = 0; b < nlist; b += per) {
        const int cnt = (int)std::min<int64_t>(per, nlist - b);
        const int32_t *lst = list_dev ? list_dev + b : nullptr;
        // without a list the query index is the position: shift the base pointers instead
        const float *qb = list_dev ? q32p : q32p + b * ix->dimp;
        const int64_t *exb = exclude ? (list_dev ? exclude : exclude + b) : nullptr;
        double *of = list_dev ? out_f64 : out_f64 + b * k;
        int64_t *oi = list_dev ? out_ids : out_ids + b * k;
        float *ov = out_val ? (list_dev ? out_val : out_val + b * k) : nullptr;
        MIRX_HIP(launch_scores_f64(qb, lst, cnt, sr.g32, sr.n, ix->dimp, ix->metric,
                                   ix->scores.as<double>(), ld, st));
        if (sr.mpos) MIRX_HIP(launch_mask_scores(ix->scores.as<double>(), ld, sr.n, sr.mpos, cnt, st));
        MIRX_HIP(launch_row_topk(ix->scores.as<double>(), ld, sr.n, sr.ids, lst, cnt, exb, k,
                                 ix->metric, of, oi, ov, st));
    }
    return MIRX_OK;
}

// The filter GEMM's workspace for a batch of nb_pad queries and the arguments every filter launch over the whole gallery shares
// (thresholds in ix->tau, which the caller fills; the counters are the caller's to zero).
int filter_args(mirx_index *ix, int64_t nb_pad, int bn, const float *bias_or_null, GemmArgs *out) {
    int regions = 0, slots = 0;
    gemm_plan(ix->size, nb_pad, bn, &regions, &slots);
    MIRX_HIP(ix->tau.ensure((size_t)nb_pad * sizeof(float)));
    MIRX_HIP(ix->cnt.ensure((size_t)nb_pad * regions * sizeof(int)));
    MIRX_HIP(ix->cand.ensure((size_t)nb_pad * regions * slots * sizeof(Cand)));
    MIRX_HIP(ix->ovf_cnt.ensure((size_t)nb_pad * sizeof(int)));
    MIRX_HIP(ix->ovf.ensure((size_t)nb_pad * CAND_OVF * sizeof(Cand)));
    MIRX_HIP(ix->spill.ensure(gemm_spill_bytes()));
    MIRX_HIP(ix->fail_list.ensure((size_t)nb_pad * sizeof(int32_t)));
    GemmArgs ga{};
    ga.g16 = ix->g16;
    ga.q16 = ix->q16.as<uint16_t>();
    ga.gbias = bias_or_null ? bias_or_null : (ix->metric == MIRX_METRIC_NEG_L2 ? ix->gbias : nullptr);
    ga.nq_pad = nb_pad;
    ga.dimp = ix->dimp;
    ga.tau = ix->tau.as<float>();
    ga.regions = regions;
    ga.slots = slots;
    ga.region_cnt = ix->cnt.as<int>();
    ga.cand = ix->cand.as<Cand>();
    ga.ovf_cnt = ix->ovf_cnt.as<int>();
    ga.ovf = ix->ovf.as<Cand>();
    ga.spill = ix->spill.p;
    *out = ga;
    return MIRX_OK;
}

// One internal batch (<= QUERY_BATCH queries), first half: everything that needs no host decision -- prepare the queries,
// sample the thresholds, filter GEMM, finalize -- then the two counters (queries to retry / to scan exactly) start their
// way to pinned host memory and an event marks that point.  Nothing here blocks the host.
int batch_front(mirx_index *ix, const float *qb, int64_t nb, int k, const int64_t *exb, float *ovb, double *ofb,
                int64_t *oib, const SearchRows &sr, hipStream_t st) {
    const int bn = gemm_query_tile(nb);
    const int64_t nb_pad = round_up(nb, bn);
    ix->pend.active = false;
    MIRX_HIP(ix->q32p.ensure((size_t)nb_pad * ix->dimp * sizeof(float)));
    MIRX_HIP(ix->q16.ensure((size_t)nb_pad * ix->dimp * sizeof(uint16_t)));
    MIRX_HIP(ix->qnorm.ensure((size_t)nb_pad * sizeof(float)));
    {
        StageTimer t(ix, st, MIRX_STAGE_PREP);
        MIRX_HIP(launch_prep_queries(qb, nb, nb_pad, ix->dim, ix->dimp, ix->q32p.as<float>(),
                                     ix->q16.as<uint16_t>(), ix->qnorm.as<float>(), st));
    }
    if (!sr.tier1) {
        // (an empty gallery lands here too: every slot becomes (-1, -inf))
        StageTimer t(ix, st, MIRX_STAGE_EXACT);
        int rc = exact_pass(ix, sr, ix->q32p.as<float>(), nullptr, nb, k, exb, ofb, oib, ovb, st);
        if (rc) return rc;
        ix->stats_host.exact_answered += nb;
        return MIRX_OK;
    }

    // ---- tier 1 ---------------------------------------------------------------------
    GemmArgs ga{};
    {
        int rc = filter_args(ix, nb_pad, bn, sr.bias, &ga);
        if (rc) return rc;
    }
    const int regions = ga.regions, slots = ga.slots;
    MIRX_HIP(ix->retry_list.ensure((size_t)nb_pad * sizeof(int32_t)));
    MIRX_HIP(ix->tau2.ensure((size_t)nb_pad * sizeof(float)));
    if (ix->force_tau_bits != 0x7fc00000u) {
        // test hook: one fixed threshold for every query
        std::vector<float> t((size_t)nb_pad, INFINITY);
        float v;
        std::memcpy(&v, &ix->force_tau_bits, 4);
        std::fill(t.begin(), t.begin() + nb, v);
        MIRX_HIP(hipMemcpyAsync(ix->tau.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, st));
        MIRX_HIP(hipStreamSynchronize(st));
    } else {
        // sample = every `stride`-th row, about size/32 rows, a multiple of the 256-row tile; at most
        // 16384 group maxima per query (the selection sorts them in LDS).  The threshold is the j-th
        // largest sampled group maximum with j ~ 256 / stride, i.e. about 256 expected candidates per
        // query whatever the gallery size (j = sample_rank = 8 at the usual stride of 32).
        const int gpt = gemm_groups_per_tile(bn);
        int64_t ms = round_up(std::max<int64_t>(ix->size / 32, 4096), ROW_ALIGN);
        ms = std::min<int64_t>(ms, (int64_t)(16384 / gpt) * ROW_ALIGN);
        const int64_t stride = std::max<int64_t>(ix->size / ms, 1);
        const int ngroups = (int)(ms / ROW_ALIGN) * gpt;
        int rank_j = (int)std::max<int64_t>(1, std::min<int64_t>(ix->sample_rank, (32 * (int64_t)ix->sample_rank) / stride));
        // j * stride candidates are expected, and a query left with fewer than k_eff of them has no k-th score to retry
        // from: it goes to the exact scan.  At the smallest galleries (stride 8) j = 8 gives ~64, so from k_eff = 17 on
        // ask for 4 k_eff of them -- at most half the groups deep, where the j-th maximum still tracks the j-th score.
        // k_eff <= 16 keeps j at any stride, and so does every k at stride >= 32 (k_eff <= TIER1_MAX_K = 64).
        const int64_t k_eff = (int64_t)k + (exb ? 1 : 0);
        const int64_t rank_k = std::min<int64_t>((4 * k_eff + stride - 1) / stride, ngroups / 2);
        rank_j = (int)std::max<int64_t>(rank_j, rank_k);
        MIRX_HIP(ix->groupmax.ensure((size_t)nb_pad * ngroups * sizeof(float)));
        GemmArgs gs = ga;
        gs.n_rows = ms;
        gs.row_stride = stride;
        gs.groupmax = ix->groupmax.as<float>();
        gs.ngroups = ngroups;
        StageTimer t(ix, st, MIRX_STAGE_SAMPLE);
        MIRX_HIP(launch_gemm_groupmax(gs, bn, st));
        MIRX_HIP(launch_select_tau(ix->groupmax.as<float>(), ngroups, nb, nb_pad, rank_j, ix->tau.as<float>(), st));
    }
    MIRX_HIP(hipMemsetAsync(ix->cnt.p, 0, (size_t)nb_pad * regions * sizeof(int), st));
    MIRX_HIP(hipMemsetAsync(ix->ovf_cnt.p, 0, (size_t)nb_pad * sizeof(int), st));
    MIRX_HIP(hipMemsetAsync(ix->fail_count, 0, 2 * sizeof(int), st));
    ga.n_rows = ix->size;
    ga.row_stride = 1;
    {
        StageTimer t(ix, st, MIRX_STAGE_GEMM);
        MIRX_HIP(launch_gemm_filter(ga, bn, st));
    }

    FinalizeArgs fa{};
    fa.q32p = ix->q32p.as<float>();
    fa.qnorm = ix->qnorm.as<float>();
    fa.g32 = ix->g32;
    fa.ids = ix->ids;
    fa.gnorm_max_bits = ix->gnorm_max_bits;
    fa.tau = ix->tau.as<float>();
    fa.regions = regions;
    fa.slots = slots;
    fa.region_cnt = ix->cnt.as<int>();
    fa.cand = ix->cand.as<Cand>();
    fa.ovf_cnt = ix->ovf_cnt.as<int>();
    fa.ovf = ix->ovf.as<Cand>();
    fa.exclude = exb;
    fa.n_rows = ix->size;
    fa.dimp = ix->dimp;
    fa.k = k;
    fa.metric = ix->metric;
    fa.nq = (int)nb;
    fa.out_f64 = ofb;
    fa.out_ids = oib;
    fa.out_val = ovb;
    fa.fail_list = ix->fail_list.as<int32_t>();
    fa.fail_count = ix->fail_count;
    fa.retry_list = ix->retry_list.as<int32_t>();
    fa.tau2 = ix->tau2.as<float>();
    fa.qmap = nullptr;
    fa.stats = ix->stats_dev;
    {
        StageTimer t(ix, st, MIRX_STAGE_FINALIZE);
        MIRX_HIP(launch_finalize(fa, st));
    }
    MIRX_HIP(hipMemcpyAsync(ix->fail_count_host, ix->fail_count, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (!ix->pend_ev) MIRX_HIP(hipEventCreateWithFlags(&ix->pend_ev, hipEventDisableTiming));
    MIRX_HIP(hipEventRecord(ix->pend_ev, st));
    ix->pend.active = true;
    ix->pend.nb = nb;
    ix->pend.k = k;
    ix->pend.exb = exb;
    ix->pend.ofb = ofb;
    ix->pend.oib = oib;
    ix->pend.ovb = ovb;
    ix->pend.st = st;
    ix->pend.ga = ga;
    ix->pend.fa = fa;
    ix->pend.rows = sr;
    return MIRX_OK;
}

// Second half: wait (host only, on the event -- the stream is not drained) for the two counters and run what they ask for:
// the second-chance filter for queries whose threshold was too high, the exact scan for what is still unanswered.  On the
// bench workload both counters are zero and this returns after the event.
int batch_back(mirx_index *ix) {
    if (!ix->pend.active) return MIRX_OK;
    ix->pend.active = false;
    hipStream_t st = ix->pend.st;
    const GemmArgs &ga = ix->pend.ga;
    const FinalizeArgs &fa = ix->pend.fa;
    const int k = ix->pend.k;
    MIRX_HIP(hipEventSynchronize(ix->pend_ev));
    const int nretry = ix->fail_count_host[1];
    if (nretry > 0) {
        // second chance: same filter GEMM over the gathered queries with tau2 = kth(s~) - 2*eps
        const int bn2 = gemm_query_tile(nretry);
        const int64_t nr_pad = round_up(nretry, bn2);
        int regions2 = 0, slots2 = 0;
        gemm_plan(ix->size, nr_pad, bn2, &regions2, &slots2);
        MIRX_HIP(ix->q16r.ensure((size_t)nr_pad * ix->dimp * sizeof(uint16_t)));
        MIRX_HIP(ix->taur.ensure((size_t)nr_pad * sizeof(float)));
        MIRX_HIP(ix->cnt.ensure((size_t)nr_pad * regions2 * sizeof(int)));
        MIRX_HIP(ix->cand.ensure((size_t)nr_pad * regions2 * slots2 * sizeof(Cand)));
        MIRX_HIP(launch_gather_queries(ix->q16.as<uint16_t>(), ix->tau2.as<float>(), ix->retry_list.as<int32_t>(),
                                       nretry, nr_pad, ix->dimp, ix->q16r.as<uint16_t>(), ix->taur.as<float>(),
                                       st));
        MIRX_HIP(hipMemsetAsync(ix->cnt.p, 0, (size_t)nr_pad * regions2 * sizeof(int), st));
        MIRX_HIP(hipMemsetAsync(ix->ovf_cnt.p, 0, (size_t)nr_pad * sizeof(int), st));
        GemmArgs g2 = ga;
        g2.q16 = ix->q16r.as<uint16_t>();
        g2.nq_pad = nr_pad;
        g2.tau = ix->taur.as<float>();
        g2.regions = regions2;
        g2.slots = slots2;
        g2.region_cnt = ix->cnt.as<int>();
        g2.cand = ix->cand.as<Cand>();
        {
            StageTimer t(ix, st, MIRX_STAGE_GEMM);
            MIRX_HIP(launch_gemm_filter(g2, bn2, st));
        }
        FinalizeArgs f2 = fa;
        f2.tau = ix->taur.as<float>();
        f2.regions = regions2;
        f2.slots = slots2;
        f2.region_cnt = ix->cnt.as<int>();
        f2.cand = ix->cand.as<Cand>();
        f2.nq = nretry;
        f2.retry_list = nullptr;          // no third chance: what fails now goes to the exact scan
        f2.tau2 = nullptr;
        f2.qmap = ix->retry_list.as<int32_t>();
        {
            StageTimer t(ix, st, MIRX_STAGE_FINALIZE);
            MIRX_HIP(launch_finalize(f2, st));
        }
        MIRX_HIP(hipMemcpyAsync(ix->fail_count_host, ix->fail_count, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        MIRX_HIP(hipEventRecord(ix->pend_ev, st));
        MIRX_HIP(hipEventSynchronize(ix->pend_ev));
    }
    const int nfail = ix->fail_count_host[0];
    if (nfail > 0) {
        StageTimer t(ix, st, MIRX_STAGE_EXACT);
        int rc = exact_pass(ix, ix->pend.rows, ix->q32p.as<float>(), ix->fail_list.as<int32_t>(), nfail, k, ix->pend.exb, ix->pend.ofb,
                            ix->pend.oib, ix->pend.ovb, st);
        if (rc) return rc;
        ix->stats_host.exact_answered += nfail;
    }
    return MIRX_OK;
}

// The tier-1 sequence answers when the tiers are on auto, `rows` rows can rank (the gallery, or a masked call's allowed rows)
// and the candidate lists hold k plus the excluded id; else the exact scan answers directly.
bool tier1_route(const mirx_index *ix, int64_t rows, int k, const int64_t *exclude) {
    return ix->tiers == MIRX_TIER_AUTO && rows >= TIER1_MIN_ROWS && k + (exclude ? 1 : 0) <= TIER1_MAX_K;
}

// wait_last = false: the last internal batch is left pending (mirx_index_search_begin); batch_back completes it.
int search_impl(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude,
                float *out_val, double *out_f64_user, int64_t *out_ids, hipStream_t st, bool wait_last = true,
                const SearchRows *masked = nullptr) {
    MIRX_CHECK(ix, "search: null index");
    MIRX_CHECK(!ix->pend.active, "search: a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    MIRX_CHECK(k >= 1 && k <= MAX_K, "search: k must be in [1, 1024]");
    MIRX_CHECK(nq >= 0, "search: nq < 0");
    MIRX_CHECK(nq == 0 || (q && out_ids && (out_val || out_f64_user)), "search: null buffer");
    ix->range_valid = false;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "search: cannot select the index device");
    MIRX_HIP(hipMemsetAsync(ix->stats_dev, 0, sizeof(mirx_search_stats), st));
    ix->stats_host = mirx_search_stats{};
    ix->stats_host.nq = nq;
    ix->spans.clear();
    ix->ev_used = 0;
    if (nq == 0) return MIRX_OK;

    SearchRows sr;
    if (masked) {
        sr = *masked;
    } else {
        sr.g32 = ix->g32;
        sr.ids = ix->ids;
        sr.n = ix->size;
        sr.tier1 = tier1_route(ix, ix->size, k, exclude);
    }
    for (int64_t q0 = 0; q0 < nq; q0 += QUERY_BATCH) {
        const int64_t nb = std::min<int64_t>(QUERY_BATCH, nq - q0);
        const float *qb = q + q0 * ix->dim;
        const int64_t *exb = exclude ? exclude + q0 : nullptr;
        float *ovb = out_val ? out_val + q0 * k : nullptr;
        int64_t *oib = out_ids + q0 * k;
        // fp64 ranking scores are always produced (user buffer or workspace)
        double *ofb;
        if (out_f64_user) {
            ofb = out_f64_user + q0 * k;
        } else {
            MIRX_HIP(ix->stage.ensure((size_t)nb * k * sizeof(double)));
            ofb = ix->stage.as<double>();
        }
        int rc = batch_front(ix, qb, nb, k, exb, ovb, ofb, oib, sr, st);
        if (rc) return rc;
        if (wait_last || q0 + QUERY_BATCH < nq) {
            rc = batch_back(ix);
            if (rc) return rc;
        }
    }
    return MIRX_OK;
}

// ---- the radix ranking (k_ranksort.hip) ---------------------------------------------------------------------------------
constexpr int64_t RANK_BITONIC_MAX_ROWS = 65536;     // the bitonic network's reach (launch_rank_rows)
constexpr size_t RANK_WS_BYTES = (size_t)1 << 29;    // workspace budget of a ranking batch, either sort

// ix->idperm = the rows in (id, row) order: one segment sorted by id ^ sign bit, stably, from the identity.
int build_id_permutation(mirx_index *ix, hipStream_t st) {
    const int64_t n = ix->size;
    MIRX_HIP(ix->rkeys.ensure((size_t)2 * n * sizeof(uint64_t)));
    MIRX_HIP(ix->rpay.ensure((size_t)2 * n * sizeof(int32_t)));
    MIRX_HIP(ix->rhist.ensure((size_t)256 * rank_sort_tiles(n) * sizeof(unsigned)));
    MIRX_HIP(ix->idperm.ensure((size_t)n * sizeof(int32_t)));
    uint64_t *ka = ix->rkeys.as<uint64_t>();
    int32_t *pa = ix->rpay.as<int32_t>();
    MIRX_HIP(launch_rank_sort_build_ids(ix->ids, n, ka, pa, st));
    MIRX_HIP(launch_rank_sort(ka, pa, ka + n, pa + n, ix->rhist.as<unsigned>(), n, 1, st));
    MIRX_HIP(hipMemcpyAsync(ix->idperm.p, pa, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    ix->idperm_valid = true;
    return MIRX_OK;
}

// Ranks 0 .. kout-1 of every query by the radix sort.  Per query of a batch: n fp64 scores, two key and two payload buffers =
// 32 bytes per row, batches sized to RANK_WS_BYTES (16 queries at 2^20 rows); a gallery whose single query does not fit is
// bounded by the allocation alone.
// mpos (rank_top under a mask): the scanned keep positions; masked rows sort behind every score and their slots read (-1, -inf).
int rank_radix(mirx_index *ix, const float *q, int64_t nq, int64_t kout, const int64_t *exclude, bool drop_excluded,
               int64_t *out_ids, float *out_val, double *out_f64, hipStream_t st, const int32_t *mpos = nullptr) {
    const int64_t n = ix->size;
    ix->range_valid = false;
    if (!ix->ids_ascend && !ix->idperm_valid) {
        int rc = build_id_permutation(ix, st);
        if (rc) return rc;
    }
    const int32_t *perm = ix->ids_ascend ? nullptr : ix->idperm.as<int32_t>();
    const int64_t ld = round_up(n, 64);
    int64_t per = (int64_t)RANK_WS_BYTES / (ld * 32);
    per = std::max<int64_t>(1, std::min<int64_t>(per, std::min<int64_t>(1024, nq)));
    if (ix->scores.ensure((size_t)per * ld * sizeof(double)) != hipSuccess ||
        ix->rkeys.ensure((size_t)2 * per * n * sizeof(uint64_t)) != hipSuccess ||
        ix->rpay.ensure((size_t)2 * per * n * sizeof(int32_t)) != hipSuccess ||
        ix->rhist.ensure((size_t)per * 256 * rank_sort_tiles(n) * sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, "rank: the sort workspace (32 bytes per gallery row) does not fit the device");
    }
    MIRX_HIP(ix->q32p.ensure((size_t)per * ix->dimp * sizeof(float)));
    MIRX_HIP(ix->q16.ensure((size_t)per * ix->dimp * sizeof(uint16_t)));
    MIRX_HIP(ix->qnorm.ensure((size_t)per * sizeof(float)));
    uint64_t *ka = ix->rkeys.as<uint64_t>(), *kb = ka + per * n;
    int32_t *pa = ix->rpay.as<int32_t>(), *pb = pa + per * n;
    for (int64_t b = 0; b < nq; b += per) {
        const int cnt = (int)std::min<int64_t>(per, nq - b);
        const int64_t *exb = exclude ? exclude + b : nullptr;
        MIRX_HIP(launch_prep_queries(q + b * ix->dim, cnt, cnt, ix->dim, ix->dimp, ix->q32p.as<float>(),
                                     ix->q16.as<uint16_t>(), ix->qnorm.as<float>(), st));
        MIRX_HIP(launch_scores_f64(ix->q32p.as<float>(), nullptr, cnt, ix->g32, n, ix->dimp, ix->metric,
                                   ix->scores.as<double>(), ld, st));
        MIRX_HIP(launch_rank_sort_build(ix->scores.as<double>(), ld, n, ix->ids, perm, exb, drop_excluded ? 1 : 0, cnt, ka, pa,
                                        st));
        if (mpos) MIRX_HIP(launch_mask_rank_keys(ka, pa, n, mpos, cnt, st));
        MIRX_HIP(launch_rank_sort(ka, pa, kb, pb, ix->rhist.as<unsigned>(), n, cnt, st));
        MIRX_HIP(launch_rank_sort_write(pa, n, kout, ix->scores.as<double>(), ld, ix->ids, exb, drop_excluded ? 1 : 0,
                                        ix->metric, cnt, out_ids + b * kout, out_val ? out_val + b * kout : nullptr,
                                        out_f64 ? out_f64 + b * kout : nullptr, st));
        if (mpos)
            MIRX_HIP(launch_mask_rank_tail(pa, n, kout, mpos, cnt, out_ids + b * kout, out_val ? out_val + b * kout : nullptr,
                                           out_f64 ? out_f64 + b * kout : nullptr, st));
    }
    return MIRX_OK;
}

// The one pass over a masked call's allow bytes (k_mask.hip) and the scan of its keep flags (k_compact.hip): leaves the bias
// vector in ix->mbias (capacity floats), the masked ids in ix->mids, the scanned positions in ix->cpos (size + 1) and the number
// of allowed rows in *n_allowed.  Every buffer, with `gather_bytes` of ix->mrows for the caller's gather of the allowed rows, is
// allocated before the first launch; one host wait, for the count.
int mask_prepare(mirx_index *ix, const uint8_t *allow, size_t gather_bytes, hipStream_t st, int64_t *n_allowed, const char *who) {
    const int64_t size = ix->size;
    bool allow_dev = false;
    is_device_pointer(allow, &allow_dev);
    hipError_t e;
    if ((e = ix->mallow.ensure(allow_dev ? 0 : (size_t)size)) != hipSuccess ||
        (e = ix->mbias.ensure((size_t)ix->cap * sizeof(float))) != hipSuccess ||
        (e = ix->mids.ensure((size_t)size * sizeof(int64_t))) != hipSuccess ||
        (e = ix->mrows.ensure(gather_bytes)) != hipSuccess ||
        (e = ix->cpos.ensure((size_t)(size + 1) * sizeof(int32_t))) != hipSuccess ||
        (e = ix->cpart.ensure((size_t)compact_tiles(size) * sizeof(int32_t))) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, std::string(who) + ": " + hipGetErrorString(e));
    }
    const uint8_t *am = allow;
    if (!allow_dev) {
        MIRX_HIP(hipMemcpyAsync(ix->mallow.p, allow, (size_t)size, hipMemcpyHostToDevice, st));
        am = ix->mallow.as<uint8_t>();
    }
    int32_t *pos = ix->cpos.as<int32_t>();
    MIRX_HIP(launch_mask_pass(am, size, ix->cap, ix->metric == MIRX_METRIC_NEG_L2 ? ix->gbias : nullptr, ix->ids,
                              ix->mbias.as<float>(), ix->mids.as<int64_t>(), pos, ix->cpart.as<int32_t>(), st));
    MIRX_HIP(launch_compact_scan_flags(pos, size, ix->cpart.as<int32_t>(), st));
    int32_t total = 0;
    MIRX_HIP(hipMemcpyAsync(&total, pos + size, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MIRX_HIP(hipStreamSynchronize(st));
    if (total < 0 || total > size) return fail(MIRX_EHIP, std::string(who) + ": the scan returned an impossible count");
    *n_allowed = total;
    return MIRX_OK;
}

// ---- range search (k_range.hip) -----------------------------------------------------------------------------------------
constexpr int64_t RANGE_MAX_HITS = (int64_t)1 << 28;   // most hits of one call by default (16 bytes each in ix->rres)

int64_t range_limit(const mirx_index *ix) { return ix->range_max_hits > 0 ? ix->range_max_hits : RANGE_MAX_HITS; }

// At least `need` bytes in `b` with its first `used` bytes kept (DevBuf::ensure drops the contents).  Waits for the stream.
int grow_keep(DevBuf &b, size_t used, size_t need, hipStream_t st, const char *who) {
    if (need <= b.bytes) return MIRX_OK;
    size_t want = std::max(need, 2 * b.bytes);
    void *np = nullptr;
    if (hipMalloc(&np, want) != hipSuccess) {
        (void)hipGetLastError();
        want = need;
        if (hipMalloc(&np, want) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIRX_ENOMEM, std::string(who) + ": the hits do not fit the device");
        }
    }
    if (used > 0 && b.p) MIRX_HIP(hipMemcpyAsync(np, b.p, used, hipMemcpyDeviceToDevice, st));
    MIRX_HIP(hipStreamSynchronize(st));
    if (b.p) (void)hipFree(b.p);
    b.p = np;
    b.bytes = want;
    return MIRX_OK;
}

struct RangeCall {
    double lo, hi;
    const int64_t *exclude;      // of the current batch, or null
    const uint8_t *allow;        // device, or null
    int64_t res_total;           // hits of the batches in front of the current one
    int64_t seg_total;           // records the exact route has written for the current batch
};

// Exact route for `m` queries of the current batch, given by a device list of their numbers in the batch (or 0 .. m-1 when
// list == null); ix->q32p holds the batch's prepared queries.  Leaves count[qx], xoff[qx] and the records in ix->rseg.
int range_exact(mirx_index *ix, RangeCall &rc, const int32_t *list_dev, int64_t m, hipStream_t st) {
    if (m <= 0) return MIRX_OK;
    const int64_t n = ix->size;
    if (!ix->ids_ascend && !ix->idperm_valid) {
        int r = build_id_permutation(ix, st);
        if (r) return r;
    }
    const int32_t *perm = ix->ids_ascend ? nullptr : ix->idperm.as<int32_t>();
    const int64_t ld = round_up(n, 64);
    int64_t per = (int64_t)RANK_WS_BYTES / (ld * 32);
    per = std::max<int64_t>(1, std::min<int64_t>(per, std::min<int64_t>(1024, m)));
    if (ix->scores.ensure((size_t)per * ld * sizeof(double)) != hipSuccess ||
        ix->rkeys.ensure((size_t)2 * per * n * sizeof(uint64_t)) != hipSuccess ||
        ix->rpay.ensure((size_t)2 * per * n * sizeof(int32_t)) != hipSuccess ||
        ix->rhist.ensure((size_t)per * 256 * rank_sort_tiles(n) * sizeof(unsigned)) != hipSuccess ||
        ix->rfirst.ensure((size_t)per * sizeof(int32_t)) != hipSuccess ||
        ix->rexcl.ensure((size_t)per * sizeof(int64_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, "range_search: the sort workspace (32 bytes per gallery row) does not fit the device");
    }
    uint64_t *ka = ix->rkeys.as<uint64_t>(), *kb = ka + per * n;
    int32_t *pa = ix->rpay.as<int32_t>(), *pb = pa + per * n;
    int32_t *count = ix->rcount.as<int32_t>();
    int64_t *xoff = ix->rxoff.as<int64_t>();
    for (int64_t b = 0; b < m; b += per) {
        const int cnt = (int)std::min<int64_t>(per, m - b);
        const int32_t *lst = list_dev ? list_dev + b : nullptr;
        const float *qb = list_dev ? ix->q32p.as<float>() : ix->q32p.as<float>() + b * ix->dimp;
        const int64_t *exb = nullptr;
        if (rc.exclude && list_dev) {
            MIRX_HIP(launch_range_gather_exclude(rc.exclude, lst, cnt, ix->rexcl.as<int64_t>(), st));
            exb = ix->rexcl.as<int64_t>();
        } else if (rc.exclude) {
            exb = rc.exclude + b;
        }
        MIRX_HIP(launch_scores_f64(qb, lst, cnt, ix->g32, n, ix->dimp, ix->metric, ix->scores.as<double>(), ld, st));
        MIRX_HIP(launch_rank_sort_build(ix->scores.as<double>(), ld, n, ix->ids, perm, exb, /*drop_excluded=*/1, cnt, ka, pa, st));
        if (rc.allow) MIRX_HIP(launch_range_mask_keys(ka, pa, n, rc.allow, cnt, st));
        MIRX_HIP(launch_rank_sort(ka, pa, kb, pb, ix->rhist.as<unsigned>(), n, cnt, st));
        MIRX_HIP(launch_range_cut(ka, n, cnt, rc.lo, rc.hi, lst, b, ix->rfirst.as<int32_t>(), count, st));
        MIRX_HIP(launch_range_scan(count, lst, b, cnt, rc.seg_total, xoff, nullptr, ix->range_total_dev, st));
        MIRX_HIP(hipMemcpyAsync(ix->range_total_host, ix->range_total_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MIRX_HIP(hipStreamSynchronize(st));
        const int64_t seg_total = ix->range_total_host[0];
        if (seg_total < rc.seg_total) return fail(MIRX_EHIP, "range_search: the scan returned an impossible count");
        if (rc.res_total + seg_total > range_limit(ix))
            return fail(MIRX_ENOMEM, "range_search: more hits than one call may return (MIRX_OPT_RANGE_MAX_HITS; default 2^28)");
        int r = grow_keep(ix->rseg, (size_t)rc.seg_total * sizeof(Hit), (size_t)seg_total * sizeof(Hit), st, "range_search");
        if (r) return r;
        MIRX_HIP(launch_range_emit(pa, n, ix->scores.as<double>(), ld, ix->ids, cnt, lst, b, ix->rfirst.as<int32_t>(), count, xoff,
                                   ix->rseg.as<Hit>(), st));
        rc.seg_total = seg_total;
        ix->range_stats.exact_answered += cnt;
    }
    return MIRX_OK;
}

// One internal batch of a range search: counts, staging rows / exact segments, lims[0 .. nb] of the batch, compaction into
// ix->rres behind the rc.res_total hits of earlier batches.
int range_batch(mirx_index *ix, RangeCall &rc, const float *qb, int64_t nb, bool filter, int64_t *lims, hipStream_t st) {
    const int bn = gemm_query_tile(nb);
    const int64_t nb_pad = round_up(nb, bn);
    MIRX_HIP(ix->q32p.ensure((size_t)nb_pad * ix->dimp * sizeof(float)));
    MIRX_HIP(ix->q16.ensure((size_t)nb_pad * ix->dimp * sizeof(uint16_t)));
    MIRX_HIP(ix->qnorm.ensure((size_t)nb_pad * sizeof(float)));
    MIRX_HIP(ix->rcount.ensure((size_t)nb * sizeof(int32_t)));
    MIRX_HIP(ix->rxoff.ensure((size_t)nb * sizeof(int64_t)));
    MIRX_HIP(launch_prep_queries(qb, nb, nb_pad, ix->dim, ix->dimp, ix->q32p.as<float>(), ix->q16.as<uint16_t>(),
                                 ix->qnorm.as<float>(), st));
    MIRX_HIP(hipMemsetAsync(ix->rcount.p, 0, (size_t)nb * sizeof(int32_t), st));
    MIRX_HIP(hipMemsetAsync(ix->rxoff.p, 0xFF, (size_t)nb * sizeof(int64_t), st));      // -1: the staging row
    rc.seg_total = 0;
    int32_t *count = ix->rcount.as<int32_t>();
    int64_t batch_total = -1;
    if (filter) {
        // the candidate machinery of batch_front (filter_args), unchanged; only tau and the finalize differ
        GemmArgs ga{};
        {
            int r = filter_args(ix, nb_pad, bn, nullptr, &ga);
            if (r) return r;
        }
        const int regions = ga.regions, slots = ga.slots;
        if (ix->rstage.ensure((size_t)nb * RANGE_CAP * sizeof(Hit)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIRX_ENOMEM, "range_search: the staging rows (20 KiB per query of a batch) do not fit the device");
        }
        MIRX_HIP(launch_range_tau(ix->q32p.as<float>(), ix->qnorm.as<float>(), ix->gnorm_max_bits, rc.lo, ix->dimp, ix->metric, nb,
                                  nb_pad, ix->tau.as<float>(), st));
        MIRX_HIP(hipMemsetAsync(ix->cnt.p, 0, (size_t)nb_pad * regions * sizeof(int), st));
        MIRX_HIP(hipMemsetAsync(ix->ovf_cnt.p, 0, (size_t)nb_pad * sizeof(int), st));
        MIRX_HIP(hipMemsetAsync(ix->fail_count, 0, 2 * sizeof(int), st));
        ga.n_rows = ix->size;
        ga.row_stride = 1;
        MIRX_HIP(launch_gemm_filter(ga, bn, st));
        RangeFinalizeArgs fa{};
        fa.q32p = ix->q32p.as<float>();
        fa.g32 = ix->g32;
        fa.ids = ix->ids;
        fa.regions = regions;
        fa.slots = slots;
        fa.region_cnt = ix->cnt.as<int>();
        fa.cand = ix->cand.as<Cand>();
        fa.ovf_cnt = ix->ovf_cnt.as<int>();
        fa.ovf = ix->ovf.as<Cand>();
        fa.exclude = rc.exclude;
        fa.allow = rc.allow;
        fa.n_rows = ix->size;
        fa.dimp = ix->dimp;
        fa.metric = ix->metric;
        fa.nq = (int)nb;
        fa.lo = rc.lo;
        fa.hi = rc.hi;
        fa.stage = ix->rstage.as<Hit>();
        fa.count = count;
        fa.fail_list = ix->fail_list.as<int32_t>();
        fa.fail_count = ix->fail_count;
        fa.stats = ix->range_stats_dev;
        MIRX_HIP(launch_range_finalize(fa, st));
        // the overflow counter and the batch's hit count (right when nothing overflowed) travel together: one host wait
        MIRX_HIP(launch_range_scan(count, nullptr, 0, (int)nb, rc.res_total, lims, lims + nb, ix->range_total_dev, st));
        MIRX_HIP(hipMemcpyAsync(ix->fail_count_host, ix->fail_count, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        MIRX_HIP(hipMemcpyAsync(ix->range_total_host, ix->range_total_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MIRX_HIP(hipStreamSynchronize(st));
        const int nfail = ix->fail_count_host[0];
        if (nfail < 0 || nfail > nb) return fail(MIRX_EHIP, "range_search: impossible overflow count");
        if (nfail == 0) {
            batch_total = ix->range_total_host[0];
        } else {
            int r = range_exact(ix, rc, ix->fail_list.as<int32_t>(), nfail, st);
            if (r) return r;
        }
    } else {
        int r = range_exact(ix, rc, nullptr, nb, st);
        if (r) return r;
    }
    if (batch_total < 0) {
        MIRX_HIP(launch_range_scan(count, nullptr, 0, (int)nb, rc.res_total, lims, lims + nb, ix->range_total_dev, st));
        MIRX_HIP(hipMemcpyAsync(ix->range_total_host, ix->range_total_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MIRX_HIP(hipStreamSynchronize(st));
        batch_total = ix->range_total_host[0];
    }
    if (batch_total < rc.res_total) return fail(MIRX_EHIP, "range_search: the scan returned an impossible count");
    if (batch_total > range_limit(ix))
        return fail(MIRX_ENOMEM, "range_search: more hits than one call may return (MIRX_OPT_RANGE_MAX_HITS; default 2^28)");
    int r = grow_keep(ix->rres, (size_t)rc.res_total * sizeof(Hit), (size_t)batch_total * sizeof(Hit), st, "range_search");
    if (r) return r;
    if (batch_total > rc.res_total)
        MIRX_HIP(launch_range_compact(ix->rstage.as<Hit>(), ix->rseg.as<Hit>(), ix->rxoff.as<int64_t>(), count, lims, (int)nb,
                                      ix->rres.as<Hit>(), st));
    rc.res_total = batch_total;
    return MIRX_OK;
}

}  // namespace

extern "C" {

const char *mirx_last_error(void) { return g_err.c_str(); }
int mirx_version(void) { return MIRX_VERSION; }

int mirx_set_tuning(int key, int64_t value) {
    switch (key) {
        case MIRX_TUNE_CONV1X1_SMALL_MAX_WG:
            MIRX_CHECK(value >= 0 && value <= (1 << 20), "set_tuning: conv1x1 small-launch limit out of range");
            set_conv1x1_small_max_wg((int)value);
            return MIRX_OK;
        case MIRX_TUNE_CONV3X3_SMALL_MAX_WG:
            MIRX_CHECK(value >= 0 && value <= (1 << 20), "set_tuning: conv3x3 small-launch limit out of range");
            set_conv3x3_small_max_wg((int)value);
            return MIRX_OK;
        case MIRX_TUNE_CONV1X1_RING:
            MIRX_CHECK(value == 0 || value == 1, "set_tuning: conv1x1 ring switch must be 0 or 1");
            set_conv1x1_ring((int)value);
            return MIRX_OK;
        default:
            return fail(MIRX_EINVAL, "set_tuning: unknown key");
    }
}

int mirx_index_create(int dim, int metric, int device, mirx_index **out) {
    MIRX_CHECK(out, "index_create: out is null");
    *out = nullptr;
    MIRX_CHECK(dim >= 1 && round_up(dim, DIM_ALIGN) <= MAX_DIMP, "index_create: dim out of range");
    MIRX_CHECK(metric == MIRX_METRIC_IP || metric == MIRX_METRIC_NEG_L2, "index_create: unknown metric");
    int ndev = 0;
    MIRX_HIP(hipGetDeviceCount(&ndev));
    MIRX_CHECK(device >= 0 && device < ndev, "index_create: no such device");
    DeviceGuard dg(device);
    if (!dg.ok) return fail(MIRX_EHIP, "index_create: cannot select device");
    mirx_index *ix = new (std::nothrow) mirx_index();
    if (!ix) return fail(MIRX_ENOMEM, "index_create: host allocation failed");
    ix->dim = dim;
    ix->dimp = (int)round_up(dim, DIM_ALIGN);
    ix->metric = metric;
    ix->device = device;
    hipError_t e;
    if ((e = hipMalloc(&ix->gnorm_max_bits, sizeof(unsigned))) != hipSuccess ||
        (e = hipMemset(ix->gnorm_max_bits, 0, sizeof(unsigned))) != hipSuccess ||
        (e = hipMalloc(&ix->fail_count, 2 * sizeof(int))) != hipSuccess ||
        (e = hipMalloc(&ix->stats_dev, sizeof(mirx_search_stats))) != hipSuccess ||
        (e = hipMemset(ix->stats_dev, 0, sizeof(mirx_search_stats))) != hipSuccess ||
        (e = hipHostMalloc(&ix->fail_count_host, 2 * sizeof(int))) != hipSuccess) {
        mirx_index_destroy(ix);
        return fail(MIRX_ENOMEM, std::string("index_create: ") + hipGetErrorString(e));
    }
    *out = ix;
    return MIRX_OK;
}

void mirx_index_destroy(mirx_index *ix) {
    if (!ix) return;
    DeviceGuard dg(ix->device);
    if (ix->g32) (void)hipFree(ix->g32);
    if (ix->g16) (void)hipFree(ix->g16);
    if (ix->ids) (void)hipFree(ix->ids);
    if (ix->gbias) (void)hipFree(ix->gbias);
    if (ix->gnorm_max_bits) (void)hipFree(ix->gnorm_max_bits);
    if (ix->fail_count) (void)hipFree(ix->fail_count);
    if (ix->stats_dev) (void)hipFree(ix->stats_dev);
    if (ix->fail_count_host) (void)hipHostFree(ix->fail_count_host);
    if (ix->range_stats_dev) (void)hipFree(ix->range_stats_dev);
    if (ix->range_total_dev) (void)hipFree(ix->range_total_dev);
    if (ix->range_total_host) (void)hipHostFree(ix->range_total_host);
    for (hipEvent_t e : ix->ev_pool) (void)hipEventDestroy(e);
    if (ix->pend_ev) (void)hipEventDestroy(ix->pend_ev);
    for (DevBuf *b : {&ix->q32p, &ix->q16, &ix->qnorm, &ix->tau, &ix->cnt, &ix->cand, &ix->ovf_cnt, &ix->ovf, &ix->groupmax,
                      &ix->fail_list, &ix->retry_list, &ix->tau2, &ix->q16r, &ix->taur, &ix->scores, &ix->stage,
                      &ix->rankwork, &ix->spill, &ix->rkeys, &ix->rpay, &ix->rhist, &ix->idperm, &ix->creq, &ix->cpos,
                      &ix->cpart, &ix->mallow, &ix->mbias, &ix->mids, &ix->mrows, &ix->rstage, &ix->rcount, &ix->rxoff,
                      &ix->rfirst, &ix->rexcl, &ix->rseg, &ix->rres})
        b->release();
    delete ix;
}

int mirx_index_reserve(mirx_index *ix, int64_t capacity_rows) {
    MIRX_CHECK(ix && capacity_rows >= 0, "index_reserve: bad argument");
    DeviceGuard dg(ix->device);
    return grow(ix, capacity_rows);
}

int64_t mirx_index_size(const mirx_index *ix) { return ix ? ix->size : -1; }
int mirx_index_dim(const mirx_index *ix) { return ix ? ix->dim : -1; }

int mirx_index_set_option(mirx_index *ix, int option, int64_t value) {
    MIRX_CHECK(ix, "set_option: null index");
    switch (option) {
        case MIRX_OPT_TIERS:
            MIRX_CHECK(value == MIRX_TIER_AUTO || value == MIRX_TIER_EXACT_ONLY, "set_option: bad tier");
            ix->tiers = (int)value;
            return MIRX_OK;
        case MIRX_OPT_SAMPLE_RANK:
            MIRX_CHECK(value >= 1 && value <= 256, "set_option: sample rank out of range");
            ix->sample_rank = (int)value;
            return MIRX_OK;
        case MIRX_OPT_FORCE_TAU:
            ix->force_tau_bits = (uint32_t)value;
            return MIRX_OK;
        case MIRX_OPT_PROFILE:
            ix->profile = value ? 1 : 0;
            return MIRX_OK;
        case MIRX_OPT_RANK_SORT:
            MIRX_CHECK(value == MIRX_RANK_SORT_AUTO || value == MIRX_RANK_SORT_BITONIC || value == MIRX_RANK_SORT_RADIX,
                       "set_option: rank sort must be 0 (auto), 1 (bitonic) or 2 (radix)");
            ix->rank_sort = (int)value;
            return MIRX_OK;
        case MIRX_OPT_MASK_GATHER_BYTES:
            MIRX_CHECK(value >= -1, "set_option: mask gather bytes must be -1 (default) or a byte count");
            ix->mask_gather_bytes = value;
            return MIRX_OK;
        case MIRX_OPT_RANGE_MAX_HITS:
            MIRX_CHECK(value >= 0, "set_option: range max hits must be 0 (default) or a count");
            ix->range_max_hits = value;
            return MIRX_OK;
        case MIRX_OPT_COMPACT_CHUNK_ROWS:
            MIRX_CHECK(value >= 0 && value <= 0x7FFFFF00ll, "set_option: compaction chunk rows out of range (0 = default)");
            ix->compact_chunk = value;
            return MIRX_OK;
        default:
            return fail(MIRX_EINVAL, "set_option: unknown option");
    }
}

int mirx_index_add(mirx_index *ix, const float *rows, int64_t n, const int64_t *ids_or_null) {
    MIRX_CHECK(ix && n >= 0 && (rows || n == 0), "index_add: bad argument");
    if (n == 0) return MIRX_OK;
    ix->range_valid = false;
    MIRX_CHECK(ix->size + n <= 0x7FFFFF00ll, "index_add: more than 2^31 rows per index");
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "index_add: cannot select device");
    int rc = grow(ix, ix->size + n);
    if (rc) return rc;
    bool rows_dev = false, ids_dev = false;
    is_device_pointer(rows, &rows_dev);
    if (ids_or_null) is_device_pointer(ids_or_null, &ids_dev);
    const int64_t chunk = std::max<int64_t>(1, ((int64_t)256 << 20) / ((int64_t)ix->dim * 4));
    for (int64_t b = 0; b < n; b += chunk) {
        const int64_t m = std::min(chunk, n - b);
        const float *src = rows + b * ix->dim;
        if (!rows_dev) {
            MIRX_HIP(ix->stage.ensure((size_t)m * ix->dim * sizeof(float)));
            MIRX_HIP(hipMemcpy(ix->stage.p, src, (size_t)m * ix->dim * sizeof(float), hipMemcpyHostToDevice));
            src = ix->stage.as<float>();
        }
        const int64_t at = ix->size + b;
        MIRX_HIP(launch_ingest(src, m, ix->dim, ix->dimp, ix->g32 + at * ix->dimp, ix->g16 + at * ix->dimp,
                               ix->gbias + at, ix->gnorm_max_bits, ix->metric, nullptr));
        MIRX_HIP(hipStreamSynchronize(nullptr));
    }
    std::vector<int64_t> host_ids;
    const int64_t *idh = ids_or_null;                      // the new ids on the host: do they go on ascending with the row?
    if (ids_or_null) {
        MIRX_HIP(hipMemcpy(ix->ids + ix->size, ids_or_null, (size_t)n * sizeof(int64_t),
                           ids_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        if (ids_dev && ix->ids_ascend) {
            host_ids.resize((size_t)n);
            MIRX_HIP(hipMemcpy(host_ids.data(), ids_or_null, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
            idh = host_ids.data();
        }
    } else {
        host_ids.resize((size_t)n);
        const int64_t first = std::max(ix->next_auto, ix->size);   // == size until a removal shrinks it
        for (int64_t i = 0; i < n; ++i) host_ids[(size_t)i] = first + i;
        ix->next_auto = first + n;
        MIRX_HIP(hipMemcpy(ix->ids + ix->size, host_ids.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        idh = host_ids.data();
    }
    if (ix->ids_ascend) {
        int64_t last = ix->last_id;
        for (int64_t i = 0; i < n && ix->ids_ascend; ++i) {
            ix->ids_ascend = idh[i] >= last;
            last = idh[i];
        }
        ix->last_id = last;
    }
    ix->idperm_valid = false;
    ix->size += n;
    return MIRX_OK;
}

int mirx_index_remove_ids(mirx_index *ix, const int64_t *ids, int64_t n, int64_t *out_removed_or_null, void *stream) {
    MIRX_CHECK(ix && n >= 0 && (ids || n == 0), "remove_ids: bad argument");
    MIRX_CHECK(n <= 0x7FFFFF00ll, "remove_ids: more than 2^31 ids in one request");
    if (ix->pend.active || ix->begun)
        return fail(MIRX_ESTATE, "remove_ids: a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    if (out_removed_or_null) *out_removed_or_null = 0;
    ix->range_valid = false;
    if (n == 0 || ix->size == 0) return MIRX_OK;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "remove_ids: cannot select device");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t size = ix->size;
    bool ids_dev = false;
    is_device_pointer(ids, &ids_dev);
    int64_t chunk = ix->compact_chunk;
    if (chunk == 0)
        chunk = std::max<int64_t>(ROW_ALIGN, (int64_t)(COMPACT_SCRATCH_BYTES / compact_scratch_bytes(1, ix->dimp)) / ROW_ALIGN * ROW_ALIGN);
    chunk = std::min(chunk, size);
    // every allocation before the first row moves: a failure leaves the index as it was
    hipError_t e;
    if ((e = ix->creq.ensure(ids_dev ? 0 : (size_t)n * sizeof(int64_t))) != hipSuccess ||
        (e = ix->rkeys.ensure((size_t)2 * n * sizeof(uint64_t))) != hipSuccess ||
        (e = ix->rpay.ensure((size_t)2 * n * sizeof(int32_t))) != hipSuccess ||
        (e = ix->rhist.ensure((size_t)256 * rank_sort_tiles(n) * sizeof(unsigned))) != hipSuccess ||
        (e = ix->cpos.ensure((size_t)(size + 1) * sizeof(int32_t))) != hipSuccess ||
        (e = ix->cpart.ensure((size_t)compact_tiles(size) * sizeof(int32_t))) != hipSuccess ||
        (e = ix->stage.ensure(compact_scratch_bytes(chunk, ix->dimp))) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, std::string("remove_ids: ") + hipGetErrorString(e));
    }
    // the request as ascending keys (id ^ sign bit, duplicates and all), sorted on the device by the ranking's radix sort: what
    // the membership kernel searches.  A host list is uploaded first; the copy is done with it when the call returns.
    const int64_t *req = ids;
    if (!ids_dev) {
        MIRX_HIP(hipMemcpyAsync(ix->creq.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st));
        req = ix->creq.as<int64_t>();
    }
    uint64_t *keys = ix->rkeys.as<uint64_t>();
    MIRX_HIP(launch_rank_sort_build_ids(req, n, keys, ix->rpay.as<int32_t>(), st));
    MIRX_HIP(launch_rank_sort(keys, ix->rpay.as<int32_t>(), keys + n, ix->rpay.as<int32_t>() + n, ix->rhist.as<unsigned>(), n, 1, st));
    int32_t *pos = ix->cpos.as<int32_t>();
    MIRX_HIP(launch_compact_scan(ix->ids, size, keys, n, pos, ix->cpart.as<int32_t>(), st));
    int32_t kept32 = 0;
    MIRX_HIP(hipMemcpyAsync(&kept32, pos + size, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MIRX_HIP(hipStreamSynchronize(st));
    const int64_t kept = kept32;
    if (kept < 0 || kept > size) return fail(MIRX_EHIP, "remove_ids: the scan returned an impossible count");
    if (kept == size) return MIRX_OK;
    for (int64_t c0 = 0; c0 < size; c0 += chunk)
        MIRX_HIP(launch_compact_chunk(ix->g32, ix->g16, ix->ids, ix->gbias, ix->stage.p, chunk, pos, c0, std::min(size, c0 + chunk),
                                      ix->dimp, st));
    // rows from the new size up to the capacity read as zeros again (ids -1), as grow() left them
    const size_t gone = (size_t)(size - kept);
    MIRX_HIP(hipMemsetAsync(ix->g32 + kept * ix->dimp, 0, gone * ix->dimp * sizeof(float), st));
    MIRX_HIP(hipMemsetAsync(ix->g16 + kept * ix->dimp, 0, gone * ix->dimp * sizeof(uint16_t), st));
    MIRX_HIP(hipMemsetAsync(ix->ids + kept, 0xFF, gone * sizeof(int64_t), st));
    MIRX_HIP(hipMemsetAsync(ix->gbias + kept, 0, gone * sizeof(float), st));
    MIRX_HIP(hipStreamSynchronize(st));
    ix->next_auto = std::max(ix->next_auto, size);                      // auto ids handed out so far are never handed out again
    ix->size = kept;
    ix->idperm_valid = false;
    if (out_removed_or_null) *out_removed_or_null = size - kept;
    return MIRX_OK;
}

int mirx_compact_tile(void) { return COMPACT_TILE; }

int mirx_index_get_rows(const mirx_index *ix, int64_t first, int64_t n, float *out_rows,
                        int64_t *out_ids_or_null) {
    MIRX_CHECK(ix && out_rows && first >= 0 && n >= 0 && first + n <= ix->size, "get_rows: bad range");
    DeviceGuard dg(ix->device);
    MIRX_HIP(hipMemcpy2D(out_rows, (size_t)ix->dim * sizeof(float), ix->g32 + first * ix->dimp,
                         (size_t)ix->dimp * sizeof(float), (size_t)ix->dim * sizeof(float), (size_t)n,
                         hipMemcpyDefault));
    if (out_ids_or_null)
        MIRX_HIP(hipMemcpy(out_ids_or_null, ix->ids + first, (size_t)n * sizeof(int64_t), hipMemcpyDefault));
    return MIRX_OK;
}

int mirx_index_get_ids(const mirx_index *ix, int64_t first, int64_t n, int64_t *out_ids) {
    MIRX_CHECK(ix && first >= 0 && n >= 0 && first + n <= ix->size && (out_ids || n == 0), "get_ids: bad range");
    if (n == 0) return MIRX_OK;
    DeviceGuard dg(ix->device);
    MIRX_HIP(hipMemcpy(out_ids, ix->ids + first, (size_t)n * sizeof(int64_t), hipMemcpyDefault));
    return MIRX_OK;
}

int mirx_index_search(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                      float *out_scores, int64_t *out_ids, void *stream) {
    return search_impl(ix, q, nq, k, exclude_ids_or_null, out_scores, nullptr, out_ids,
                       reinterpret_cast<hipStream_t>(stream));
}

int mirx_index_search_f64(mirx_index *ix, const float *q, int64_t nq, int k,
                          const int64_t *exclude_ids_or_null, double *out_rank_scores, int64_t *out_ids,
                          void *stream) {
    return search_impl(ix, q, nq, k, exclude_ids_or_null, nullptr, out_rank_scores, out_ids,
                       reinterpret_cast<hipStream_t>(stream));
}

int mirx_index_search_begin(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                            float *out_scores_or_null, double *out_rank_scores_or_null, int64_t *out_ids, void *stream) {
    const int rc = search_impl(ix, q, nq, k, exclude_ids_or_null, out_scores_or_null, out_rank_scores_or_null, out_ids,
                               reinterpret_cast<hipStream_t>(stream), /*wait_last=*/false);
    if (rc == MIRX_OK) ix->begun = true;
    return rc;
}

int mirx_index_search_masked(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                             const uint8_t *allow, int64_t n_allow, float *out_scores_or_null, double *out_rank_scores_or_null,
                             int64_t *out_ids, void *stream) {
    MIRX_CHECK(ix, "search_masked: null index");
    if (ix->pend.active || ix->begun)
        return fail(MIRX_ESTATE, "search_masked: a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    MIRX_CHECK(n_allow == ix->size, "search_masked: the mask needs one byte per row of the index (n_allow != size)");
    MIRX_CHECK(allow || n_allow == 0, "search_masked: null mask");
    MIRX_CHECK(k >= 1 && k <= MAX_K, "search_masked: k must be in [1, 1024]");
    MIRX_CHECK(nq >= 0, "search_masked: nq < 0");
    MIRX_CHECK(nq == 0 || (q && out_ids && (out_scores_or_null || out_rank_scores_or_null)), "search_masked: null buffer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (nq == 0 || ix->size == 0)
        return search_impl(ix, q, nq, k, exclude_ids_or_null, out_scores_or_null, out_rank_scores_or_null, out_ids, st);
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "search_masked: cannot select the index device");
    // the gather's scratch is sized before the count is known: with the filter route open only fewer than TIER1_MIN_ROWS
    // allowed rows are ever gathered, else any number whose rows fit the limit
    const size_t row_bytes = (size_t)ix->dimp * sizeof(float) + sizeof(int64_t);
    const size_t gather_max = ix->mask_gather_bytes < 0 ? EXACT_WS_BYTES : (size_t)ix->mask_gather_bytes;
    const int64_t most_rows = tier1_route(ix, TIER1_MIN_ROWS, k, exclude_ids_or_null) ? std::min(ix->size, TIER1_MIN_ROWS - 1) : ix->size;
    int64_t n_allowed = 0;
    int rc = mask_prepare(ix, allow, std::min((size_t)most_rows * row_bytes, gather_max), st, &n_allowed, "search_masked");
    if (rc) return rc;
    if (n_allowed == ix->size)            // nothing masked: the plain search, bit for bit
        return search_impl(ix, q, nq, k, exclude_ids_or_null, out_scores_or_null, out_rank_scores_or_null, out_ids, st);
    SearchRows sr;
    sr.tier1 = tier1_route(ix, n_allowed, k, exclude_ids_or_null);
    const size_t gather_bytes = (size_t)n_allowed * row_bytes;
    if (sr.tier1 || (n_allowed > 0 && gather_bytes > gather_max)) {
        // all rows, the masked ones neutralised: tier 1 by the bias, the exact scan by -inf scores and the masked ids
        sr.g32 = ix->g32;
        sr.ids = ix->mids.as<int64_t>();
        sr.n = ix->size;
        sr.mpos = ix->cpos.as<int32_t>();
        sr.bias = sr.tier1 ? ix->mbias.as<float>() : nullptr;
    } else if (n_allowed > 0) {
        // few allowed rows: gather them (ascending, so ids keep their order) and scan only those
        if (gather_bytes > ix->mrows.bytes) return fail(MIRX_EHIP, "search_masked: the gather scratch is smaller than the count needs");
        float *s32 = ix->mrows.as<float>();
        int64_t *sid = reinterpret_cast<int64_t *>(s32 + n_allowed * ix->dimp);
        MIRX_HIP(launch_compact_gather(ix->g32, ix->ids, ix->cpos.as<int32_t>(), ix->size, ix->dimp, s32, sid, st));
        sr.g32 = s32;
        sr.ids = sid;
        sr.n = n_allowed;
    }                                     // else nothing is allowed: n = 0, every slot reads (-1, -inf) and no row is scored
    return search_impl(ix, q, nq, k, exclude_ids_or_null, out_scores_or_null, out_rank_scores_or_null, out_ids, st,
                       /*wait_last=*/true, &sr);
}

int mirx_index_range_search(mirx_index *ix, const float *q, int64_t nq, double lo, double hi, const int64_t *exclude_ids_or_null,
                            const uint8_t *allow_or_null, int64_t n_allow, int64_t *out_lims, int64_t *out_total, void *stream) {
    MIRX_CHECK(ix, "range_search: null index");
    if (ix->pend.active || ix->begun)
        return fail(MIRX_ESTATE, "range_search: a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    ix->range_valid = false;
    MIRX_CHECK(nq >= 0, "range_search: nq < 0");
    MIRX_CHECK(nq <= 0x7FFFFF00ll, "range_search: more than 2^31 queries in one call");
    MIRX_CHECK(!(lo != lo) && !(hi != hi), "range_search: a bound is NaN");
    MIRX_CHECK(out_lims && out_total, "range_search: null output");
    MIRX_CHECK(q || nq == 0, "range_search: null queries");
    MIRX_CHECK(allow_or_null ? n_allow == ix->size : n_allow == 0,
               "range_search: the mask needs one byte per row of the index (n_allow != size)");
    *out_total = 0;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "range_search: cannot select the index device");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!ix->range_stats_dev) {
        hipError_t e;
        if ((e = hipMalloc(&ix->range_stats_dev, 2 * sizeof(unsigned long long))) != hipSuccess ||
            (e = hipMalloc(&ix->range_total_dev, sizeof(int64_t))) != hipSuccess ||
            (e = hipHostMalloc(&ix->range_total_host, sizeof(int64_t))) != hipSuccess)
            return fail(MIRX_ENOMEM, std::string("range_search: ") + hipGetErrorString(e));
    }
    MIRX_HIP(hipMemsetAsync(ix->range_stats_dev, 0, 2 * sizeof(unsigned long long), st));
    ix->range_stats = mirx_range_stats{};
    ix->range_stats.nq = nq;
    ix->range_total = 0;
    MIRX_HIP(hipMemsetAsync(out_lims, 0, (size_t)(nq + 1) * sizeof(int64_t), st));
    if (nq == 0 || ix->size == 0 || !(hi > lo)) {          // nothing can be a hit: lims of zeros, no launch
        ix->range_valid = true;
        return MIRX_OK;
    }
    const uint8_t *allow = allow_or_null;
    if (allow) {
        bool allow_dev = false;
        is_device_pointer(allow, &allow_dev);
        if (!allow_dev) {
            if (ix->mallow.ensure((size_t)ix->size) != hipSuccess) {
                (void)hipGetLastError();
                return fail(MIRX_ENOMEM, "range_search: the mask does not fit the device");
            }
            MIRX_HIP(hipMemcpyAsync(ix->mallow.p, allow, (size_t)ix->size, hipMemcpyHostToDevice, st));
            allow = ix->mallow.as<uint8_t>();
        }
    }
    const bool filter = ix->tiers == MIRX_TIER_AUTO && ix->size >= TIER1_MIN_ROWS && lo > -INFINITY;
    RangeCall rc{};
    rc.lo = lo;
    rc.hi = hi;
    rc.allow = allow;
    for (int64_t q0 = 0; q0 < nq; q0 += QUERY_BATCH) {
        const int64_t nb = std::min<int64_t>(QUERY_BATCH, nq - q0);
        rc.exclude = exclude_ids_or_null ? exclude_ids_or_null + q0 : nullptr;
        int r = range_batch(ix, rc, q + q0 * ix->dim, nb, filter, out_lims + q0, st);
        if (r) return r;
    }
    ix->range_total = rc.res_total;
    ix->range_stats.hits = rc.res_total;
    ix->range_valid = true;
    *out_total = rc.res_total;
    return MIRX_OK;
}

int mirx_index_range_fetch(mirx_index *ix, float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids, void *stream) {
    MIRX_CHECK(ix, "range_fetch: null index");
    if (!ix->range_valid)
        return fail(MIRX_ESTATE, "range_fetch: no range search precedes this call (or another call on the index has reused its scratch)");
    if (ix->range_total == 0) return MIRX_OK;
    MIRX_CHECK(out_ids && (out_values_or_null || out_f64_or_null), "range_fetch: null output");
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "range_fetch: cannot select the index device");
    MIRX_HIP(launch_range_fetch(ix->rres.as<Hit>(), ix->range_total, ix->metric, out_values_or_null, out_f64_or_null, out_ids,
                                reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_index_range_last_stats(mirx_index *ix, mirx_range_stats *out) {
    MIRX_CHECK(ix && out, "range_last_stats: null argument");
    *out = ix->range_stats;
    if (!ix->range_stats_dev) return MIRX_OK;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "range_last_stats: cannot select the index device");
    unsigned long long d[2] = {0, 0};
    MIRX_HIP(hipDeviceSynchronize());
    MIRX_HIP(hipMemcpy(d, ix->range_stats_dev, sizeof(d), hipMemcpyDeviceToHost));
    out->filter_answered = (int64_t)d[0];
    out->candidates = (int64_t)d[1];
    return MIRX_OK;
}

int mirx_index_search_end(mirx_index *ix) {
    MIRX_CHECK(ix, "search_end: null index");
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "search_end: cannot select the index device");
    ix->begun = false;
    return batch_back(ix);
}

int mirx_index_last_stats(mirx_index *ix, void *stream, mirx_search_stats *out) {
    MIRX_CHECK(ix && out, "last_stats: null argument");
    DeviceGuard dg(ix->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MIRX_HIP(hipStreamSynchronize(st));
    mirx_search_stats d{};
    MIRX_HIP(hipMemcpy(&d, ix->stats_dev, sizeof(d), hipMemcpyDeviceToHost));
    *out = d;
    out->nq = ix->stats_host.nq;
    out->exact_answered = ix->stats_host.exact_answered;
    return MIRX_OK;
}

int mirx_index_last_timings(mirx_index *ix, float *out_ms) {
    MIRX_CHECK(ix && out_ms, "last_timings: null argument");
    DeviceGuard dg(ix->device);
    for (int i = 0; i < MIRX_NUM_STAGES; ++i) out_ms[i] = 0.0f;
    for (const auto &sp : ix->spans) {
        MIRX_HIP(hipEventSynchronize(sp.b));
        float ms = 0.0f;
        MIRX_HIP(hipEventElapsedTime(&ms, sp.a, sp.b));
        out_ms[sp.stage] += ms;
    }
    return MIRX_OK;
}

int mirx_index_rank_all(mirx_index *ix, const float *q, int64_t nq, const int64_t *exclude_ids_or_null,
                        int64_t *out_ids, float *out_scores_or_null, void *stream) {
    MIRX_CHECK(ix && q && out_ids && nq >= 0, "rank_all: bad argument");
    const bool radix = ix->rank_sort == MIRX_RANK_SORT_RADIX ||
                       (ix->rank_sort == MIRX_RANK_SORT_AUTO && ix->size > RANK_BITONIC_MAX_ROWS);
    MIRX_CHECK(radix || ix->size <= RANK_BITONIC_MAX_ROWS,
               "rank_all: the bitonic sort (MIRX_OPT_RANK_SORT = 1) takes at most 65536 rows");
    ix->range_valid = false;
    if (nq == 0 || ix->size == 0) return MIRX_OK;
    DeviceGuard dg(ix->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (radix)
        return rank_radix(ix, q, nq, ix->size, exclude_ids_or_null, /*drop_excluded=*/false, out_ids, out_scores_or_null,
                          nullptr, st);
    const int64_t n = ix->size;
    int64_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    const int64_t ld = round_up(n, 64);
    int64_t per = std::max<int64_t>(4, std::min<int64_t>(1024, (int64_t)RANK_WS_BYTES / (np2 * 16))) / 4 * 4;
    per = std::min<int64_t>(per, round_up(nq, 4));
    MIRX_HIP(ix->scores.ensure((size_t)per * ld * sizeof(double)));
    MIRX_HIP(ix->rankwork.ensure((size_t)per * np2 * sizeof(Hit)));
    MIRX_HIP(ix->q32p.ensure((size_t)per * ix->dimp * sizeof(float)));
    MIRX_HIP(ix->q16.ensure((size_t)per * ix->dimp * sizeof(uint16_t)));
    MIRX_HIP(ix->qnorm.ensure((size_t)per * sizeof(float)));
    for (int64_t b = 0; b < nq; b += per) {
        const int cnt = (int)std::min<int64_t>(per, nq - b);
        MIRX_HIP(launch_prep_queries(q + b * ix->dim, cnt, cnt, ix->dim, ix->dimp, ix->q32p.as<float>(),
                                     ix->q16.as<uint16_t>(), ix->qnorm.as<float>(), st));
        MIRX_HIP(launch_scores_f64(ix->q32p.as<float>(), nullptr, cnt, ix->g32, n, ix->dimp, ix->metric,
                                   ix->scores.as<double>(), ld, st));
        MIRX_HIP(launch_rank_rows(ix->scores.as<double>(), ld, n, ix->ids,
                                  exclude_ids_or_null ? exclude_ids_or_null + b : nullptr, cnt,
                                  ix->rankwork.as<Hit>(), np2, ix->metric, out_ids + b * n,
                                  out_scores_or_null ? out_scores_or_null + b * n : nullptr, st));
    }
    return MIRX_OK;
}

int mirx_index_rank_top(mirx_index *ix, const float *q, int64_t nq, int64_t k, const int64_t *exclude_ids_or_null,
                        float *out_scores_or_null, double *out_rank_scores_or_null, int64_t *out_ids, void *stream) {
    MIRX_CHECK(k >= 1, "rank_top: k must be at least 1");
    MIRX_CHECK(nq >= 0, "rank_top: nq < 0");
    MIRX_CHECK(out_ids, "rank_top: out_ids is null");
    MIRX_CHECK(out_scores_or_null || out_rank_scores_or_null, "rank_top: both score outputs are null");
    MIRX_CHECK(ix, "rank_top: null index");
    MIRX_CHECK(q || nq == 0, "rank_top: null queries");
    MIRX_CHECK(k <= ix->size, "rank_top: k is larger than the index");
    if (nq == 0) return MIRX_OK;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "rank_top: cannot select the index device");
    return rank_radix(ix, q, nq, k, exclude_ids_or_null, /*drop_excluded=*/true, out_ids, out_scores_or_null,
                      out_rank_scores_or_null, reinterpret_cast<hipStream_t>(stream));
}

int mirx_index_rank_top_masked(mirx_index *ix, const float *q, int64_t nq, int64_t k, const int64_t *exclude_ids_or_null,
                               const uint8_t *allow, int64_t n_allow, float *out_scores_or_null,
                               double *out_rank_scores_or_null, int64_t *out_ids, void *stream) {
    MIRX_CHECK(ix, "rank_top_masked: null index");
    if (ix->pend.active || ix->begun)
        return fail(MIRX_ESTATE, "rank_top_masked: a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    MIRX_CHECK(n_allow == ix->size, "rank_top_masked: the mask needs one byte per row of the index (n_allow != size)");
    MIRX_CHECK(allow || n_allow == 0, "rank_top_masked: null mask");
    MIRX_CHECK(k >= 1, "rank_top_masked: k must be at least 1");
    MIRX_CHECK(nq >= 0, "rank_top_masked: nq < 0");
    MIRX_CHECK(out_ids, "rank_top_masked: out_ids is null");
    MIRX_CHECK(out_scores_or_null || out_rank_scores_or_null, "rank_top_masked: both score outputs are null");
    MIRX_CHECK(q || nq == 0, "rank_top_masked: null queries");
    MIRX_CHECK(k <= ix->size, "rank_top_masked: k is larger than the index");
    if (nq == 0) return MIRX_OK;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "rank_top_masked: cannot select the index device");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t n_allowed = 0;
    int rc = mask_prepare(ix, allow, 0, st, &n_allowed, "rank_top_masked");
    if (rc) return rc;
    return rank_radix(ix, q, nq, k, exclude_ids_or_null, /*drop_excluded=*/true, out_ids, out_scores_or_null,
                      out_rank_scores_or_null, st, n_allowed == ix->size ? nullptr : ix->cpos.as<int32_t>());
}

uint64_t mirx_rank_key(double score) { return rank_key(score); }
int mirx_rank_sort_tile(void) { return RANK_TILE; }

int mirx_topk_merge(const double *in_scores, const int64_t *in_ids, int nshard, int64_t nq, int k,
                    int metric, double *out_rank_scores, float *out_scores, int64_t *out_ids, void *stream) {
    MIRX_CHECK(in_scores && in_ids && out_ids && nshard >= 1 && nq >= 0 && k >= 1, "topk_merge: bad argument");
    MIRX_CHECK((int64_t)nshard * k <= 8192, "topk_merge: nshard * k must be <= 8192");
    MIRX_HIP(launch_topk_merge(in_scores, in_ids, nshard, nq, k, metric, out_rank_scores, out_scores,
                               out_ids, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_conv1x1_bn_relu_split3(const float *x, int64_t x_batch_stride, int cin, const float *scale1_or_null,
                                const float *shift1_or_null, const void *w3, const float *bias_or_null, int64_t n,
                                int hw, int cout, int relu_out, float *y, int64_t y_batch_stride, void *stream) {
    MIRX_CHECK(n >= 0 && hw >= 1 && cin >= 16 && cin % 16 == 0 && cout >= 128 && cout % 128 == 0,
               "conv1x1_split3: cin must be a multiple of 16 and cout of 128");
    MIRX_CHECK((scale1_or_null == nullptr) == (shift1_or_null == nullptr), "conv1x1_split3: scale and shift go together");
    MIRX_CHECK(n == 0 || (x && w3 && y), "conv1x1_split3: null buffer");
    MIRX_CHECK(x_batch_stride >= (int64_t)cin * hw, "conv1x1_split3: batch stride smaller than the channel prefix");
    MIRX_CHECK(y_batch_stride >= (int64_t)cout * hw, "conv1x1_split3: output batch stride smaller than cout * hw");
    MIRX_HIP(launch_conv1x1_s3(x, x_batch_stride, cin, scale1_or_null, shift1_or_null,
                               reinterpret_cast<const uint16_t *>(w3), bias_or_null, n, hw, cout, relu_out, y,
                               y_batch_stride, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_conv1x1_bn_relu_split2h(const float *x, int64_t x_batch_stride, int cin, const float *scale1_or_null,
                                 const float *shift1_or_null, const void *w2, const float *oscale,
                                 const float *bias_or_null, int64_t n, int hw, int cout, int relu_out, float *y,
                                 int64_t y_batch_stride, const float *in_range_or_null, float in_ks, float in_kb,
                                 float *out_range_or_null, int64_t x_plane_stride, int64_t y_plane_stride, void *stream) {
    MIRX_CHECK(n >= 0 && hw >= 1 && cin >= 16 && cin % 16 == 0 && cout >= 128 && cout % 128 == 0,
               "conv1x1_split2h: cin must be a multiple of 16 and cout of 128");
    if (!x_plane_stride) x_plane_stride = hw;
    if (!y_plane_stride) y_plane_stride = hw;
    MIRX_CHECK(x_plane_stride >= hw && y_plane_stride >= hw, "conv1x1_split2h: a plane stride is 0 (= hw) or at least hw");
    MIRX_CHECK((scale1_or_null == nullptr) == (shift1_or_null == nullptr), "conv1x1_split2h: scale and shift go together");
    MIRX_CHECK(n == 0 || (x && w2 && y && oscale), "conv1x1_split2h: null buffer");
    MIRX_CHECK(x_batch_stride >= (int64_t)cin * x_plane_stride, "conv1x1_split2h: batch stride smaller than the channel prefix");
    MIRX_CHECK(y_batch_stride >= (int64_t)cout * y_plane_stride, "conv1x1_split2h: output batch stride smaller than cout planes");
    MIRX_CHECK(in_ks >= 0.f && in_kb >= 0.f && (in_range_or_null || in_kb > 0.f),
               "conv1x1_split2h: in_ks / in_kb are non-negative; without range slots in_kb is the bound itself");
    MIRX_HIP(launch_conv1x1_h2(x, x_batch_stride, cin, scale1_or_null, shift1_or_null,
                               reinterpret_cast<const uint16_t *>(w2), oscale, bias_or_null, n, hw, cout, relu_out, y,
                               y_batch_stride, in_range_or_null, in_ks, in_kb, out_range_or_null, 0.f, 0.f, nullptr,
                               x_plane_stride, y_plane_stride, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}


int mirx_conv1x1_bn_relu_split2h_terms(const float *x, int64_t x_batch_stride, int cin, const float *scale1,
                                       const float *shift1, const void *w2, const float *oscale, const float *bias,
                                       int64_t n, int hw, void *y_terms, const float *in_range, float in_ks, float in_kb,
                                       float y_ks, float y_kb, float *y_inv_out, int64_t x_plane_stride, void *stream) {
    MIRX_CHECK(n >= 0 && hw >= 1 && cin >= 16 && cin % 16 == 0, "conv1x1_split2h_terms: cin must be a multiple of 16");
    MIRX_CHECK(n == 0 || (x && w2 && y_terms && oscale && scale1 && shift1 && bias && in_range && y_inv_out),
               "conv1x1_split2h_terms: null buffer");
    if (!x_plane_stride) x_plane_stride = hw;
    MIRX_CHECK(x_plane_stride >= hw, "conv1x1_split2h_terms: the plane stride is 0 (= hw) or at least hw");
    MIRX_CHECK(x_batch_stride >= (int64_t)cin * x_plane_stride, "conv1x1_split2h_terms: batch stride smaller than the channel prefix");
    MIRX_CHECK(in_ks >= 0.f && in_kb >= 0.f && y_ks >= 0.f && y_kb >= 0.f, "conv1x1_split2h_terms: bounds are non-negative");
    MIRX_HIP(launch_conv1x1_h2(x, x_batch_stride, cin, scale1, shift1, reinterpret_cast<const uint16_t *>(w2), oscale, bias, n,
                               hw, 128, 1, reinterpret_cast<float *>(y_terms), 0, in_range, in_ks, in_kb, nullptr, y_ks, y_kb,
                               y_inv_out, x_plane_stride, 0, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_conv3x3_direct_terms_nchw(const void *y_terms, const void *w2, const float *oscale, int64_t n, int side, float *out,
                                   int64_t out_batch_stride, const float *y_inv, float *out_range_or_null,
                                   int64_t out_plane_stride, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535, "conv3x3_terms: batch must be in [0, 65535]");
    MIRX_CHECK(side == 56 || side == 28 || side == 14 || side == 7, "conv3x3_terms: side must be 56, 28, 14 or 7");
    MIRX_CHECK(n == 0 || (y_terms && w2 && oscale && out && y_inv), "conv3x3_terms: null buffer");
    if (!out_plane_stride) out_plane_stride = (int64_t)side * side;
    MIRX_CHECK(out_plane_stride >= (int64_t)side * side, "conv3x3_terms: the plane stride is 0 (= side^2) or at least side^2");
    MIRX_CHECK(out_batch_stride >= 32 * out_plane_stride, "conv3x3_terms: output batch stride too small");
    MIRX_HIP(launch_conv3x3_d2p(reinterpret_cast<const uint16_t *>(y_terms), reinterpret_cast<const uint16_t *>(w2), oscale, n,
                                side, out, out_batch_stride, y_inv, out_range_or_null, out_plane_stride,
                                reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_conv3x3_direct_terms_nchw_pool(const void *y_terms, const void *w2, const float *oscale, int64_t n, int side, float *out,
                                        int64_t out_batch_stride, const float *y_inv, float *out_range_or_null,
                                        int64_t out_plane_stride, const float *pool_scale, const float *pool_shift,
                                        float *pooled, int64_t pooled_batch_stride, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535, "conv3x3_terms_pool: batch must be in [0, 65535]");
    MIRX_CHECK(side == 56 || side == 28 || side == 14, "conv3x3_terms_pool: side must be 56, 28 or 14");
    MIRX_CHECK(n == 0 || (y_terms && w2 && oscale && out && y_inv && pool_scale && pool_shift && pooled),
               "conv3x3_terms_pool: null buffer");
    if (!out_plane_stride) out_plane_stride = (int64_t)side * side;
    MIRX_CHECK(out_plane_stride >= (int64_t)side * side, "conv3x3_terms_pool: the plane stride is 0 (= side^2) or at least side^2");
    MIRX_CHECK(out_batch_stride >= 32 * out_plane_stride, "conv3x3_terms_pool: output batch stride too small");
    MIRX_CHECK(pooled_batch_stride >= (int64_t)32 * (side / 2) * (side / 2), "conv3x3_terms_pool: pooled batch stride too small");
    MIRX_CHECK(!conv3x3_takes_small(n, side),
               "conv3x3_terms_pool: a launch this small runs on the one-wave-per-block kernel, which has no pooled twin "
               "(mirx_conv3x3_small_launch tells; use mirx_conv3x3_direct_terms_nchw + mirx_bn_relu_avgpool2)");
    MIRX_HIP(launch_conv3x3_d2p(reinterpret_cast<const uint16_t *>(y_terms), reinterpret_cast<const uint16_t *>(w2), oscale, n,
                                side, out, out_batch_stride, y_inv, out_range_or_null, out_plane_stride,
                                reinterpret_cast<hipStream_t>(stream), pool_scale, pool_shift, pooled, pooled_batch_stride));
    return MIRX_OK;
}

int mirx_conv3x3_small_launch(int64_t n, int side) {
    return (side == 56 || side == 28 || side == 14 || side == 7) && n > 0 && conv3x3_takes_small(n, side) ? 1 : 0;
}

int mirx_dense_layer_fused(float *buf, int64_t batch_stride, int64_t plane_stride, int cin, const float *scale1,
                           const float *shift1, const void *w2, const float *oscale, const float *bias, const void *c3w2,
                           const float *c3oscale, int64_t n, int side, float *range_row, float in_ks, float in_kb, float y_ks,
                           float y_kb, void *stream) {
    MIRX_CHECK(n >= 0 && n <= (int64_t)1 << 30, "dense_layer_fused: bad batch");
    MIRX_CHECK(side == 14 || side == 7, "dense_layer_fused: side must be 14 or 7 (the bottleneck of a 196-pixel unit fits the LDS)");
    MIRX_CHECK(cin >= 128 && cin <= 1024 && cin % 32 == 0, "dense_layer_fused: cin must be a multiple of 32 in [128, 1024]");
    if (!plane_stride) plane_stride = (int64_t)side * side;
    MIRX_CHECK(plane_stride == (int64_t)side * side, "dense_layer_fused: channel planes must be packed (plane stride 0 or side^2)");
    MIRX_CHECK(batch_stride >= (int64_t)(cin + 32) * plane_stride && batch_stride % 4 == 0,
               "dense_layer_fused: batch stride smaller than cin + 32 planes, or not a multiple of 4 floats");
    MIRX_CHECK((reinterpret_cast<uintptr_t>(buf) & 15) == 0, "dense_layer_fused: buf must be 16-byte aligned");
    MIRX_CHECK(n == 0 || (buf && scale1 && shift1 && w2 && oscale && bias && c3w2 && c3oscale && range_row),
               "dense_layer_fused: null buffer");
    MIRX_CHECK(in_ks >= 0.f && in_kb >= 0.f && y_ks >= 0.f && y_kb >= 0.f, "dense_layer_fused: bounds are non-negative");
    MIRX_HIP(launch_dense_fused(buf, batch_stride, cin, scale1, shift1, reinterpret_cast<const uint16_t *>(w2), oscale,
                                bias, reinterpret_cast<const uint16_t *>(c3w2), c3oscale, n, side, range_row, in_ks, in_kb, y_ks,
                                y_kb, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_linear_split3(const float *x, int64_t m, int k, const void *w3, const float *bias_or_null, int n, int act,
                       const float *residual_or_null, const float *gamma_or_null, float *y, void *stream) {
    MIRX_CHECK(m >= 0 && k >= 16 && k % 16 == 0 && n >= 1, "linear_split3: k must be a multiple of 16");
    MIRX_CHECK(act >= 0 && act <= 2 && !(act == 2 && residual_or_null), "linear_split3: act is 0 (none), 1 (erf gelu) or 2 (tanh gelu, no residual)");
    MIRX_CHECK(m == 0 || (x && w3 && y), "linear_split3: null buffer");
    MIRX_CHECK(residual_or_null || !gamma_or_null, "linear_split3: gamma scales the residual branch only");
    MIRX_CHECK(x != y, "linear_split3: y may alias the residual, not the input");
    MIRX_HIP(launch_linear_s3(x, m, k, reinterpret_cast<const uint16_t *>(w3), bias_or_null, n, act, residual_or_null,
                              gamma_or_null, y, 0, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_linear_split2h(const float *x, int64_t m, int k, const void *w2, const float *bias_or_null, int n, int act,
                        const float *residual_or_null, const float *gamma_or_null, float x_scale, float out_scale,
                        float *y, void *stream) {
    MIRX_CHECK(m >= 0 && k >= 16 && k % 16 == 0 && n >= 1, "linear_split2h: k must be a multiple of 16");
    MIRX_CHECK(act >= 0 && act <= 2 && !(act == 2 && residual_or_null), "linear_split2h: act is 0 (none), 1 (erf gelu) or 2 (tanh gelu, no residual)");
    MIRX_CHECK(m == 0 || (x && w2 && y), "linear_split2h: null buffer");
    MIRX_CHECK(residual_or_null || !gamma_or_null, "linear_split2h: gamma scales the residual branch only");
    MIRX_CHECK(x != y, "linear_split2h: y may alias the residual, not the input");
    MIRX_CHECK(x_scale > 0.f && out_scale > 0.f, "linear_split2h: scales must be positive powers of two");
    MIRX_HIP(launch_linear_h2(x, m, k, reinterpret_cast<const uint16_t *>(w2), bias_or_null, n, act, residual_or_null,
                              gamma_or_null, x_scale, out_scale, y, 0, nullptr, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_linear_split2h_gelu_grn(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w2,
                                 const float *bias_or_null, int n, float x_scale, float out_scale, float *y, float *partials,
                                 float *gx, void *stream) {
    MIRX_CHECK(n_img >= 0 && tokens_per_image >= 128 && k >= 16 && k % 16 == 0 && n >= 1,
               "linear_split2h_gelu_grn: k must be a multiple of 16, tokens_per_image at least 128");
    MIRX_CHECK(n_img == 0 || (x && w2 && y && partials && gx), "linear_split2h_gelu_grn: null buffer");
    MIRX_CHECK(x_scale > 0.f && out_scale > 0.f, "linear_split2h_gelu_grn: scales must be positive");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MIRX_HIP(launch_linear_h2(x, n_img * tokens_per_image, k, reinterpret_cast<const uint16_t *>(w2), bias_or_null, n, 1, nullptr,
                              nullptr, x_scale, out_scale, y, tokens_per_image, nullptr, st, false, partials));
    MIRX_HIP(launch_grn_norm_partials(partials, tokens_per_image, n_img, n, gx, st));
    return MIRX_OK;
}

int mirx_linear_split2h_grn_rows(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w2,
                                 const float *bias_or_null, int n, const float *residual_or_null, const float *input_scale,
                                 float x_bound, const float *input_scale_max, float w_inv, float *y, void *stream) {
    MIRX_CHECK(n_img >= 0 && tokens_per_image >= 1 && k >= 16 && k % 16 == 0 && n >= 1,
               "linear_split2h_grn_rows: k must be a multiple of 16");
    MIRX_CHECK(n_img == 0 || (x && w2 && y && input_scale && input_scale_max), "linear_split2h_grn_rows: null buffer");
    MIRX_CHECK(x != y, "linear_split2h_grn_rows: y may alias the residual, not the input");
    MIRX_CHECK(x_bound > 0.f && w_inv > 0.f, "linear_split2h_grn_rows: x_bound and w_inv must be positive");
    MIRX_HIP(launch_linear_h2(x, n_img * tokens_per_image, k, reinterpret_cast<const uint16_t *>(w2), bias_or_null, n, 0,
                              residual_or_null, input_scale, x_bound, w_inv, y, tokens_per_image, input_scale_max,
                              reinterpret_cast<hipStream_t>(stream), true));
    return MIRX_OK;
}

int mirx_linear_split2h_nchw(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w2,
                             const float *bias_or_null, int n, const float *residual_or_null,
                             const float *input_scale_or_null, float x_bound, const float *input_scale_max_or_null,
                             float w_inv, float *y, void *stream) {
    MIRX_CHECK(n_img >= 0 && tokens_per_image >= 1 && k >= 16 && k % 16 == 0 && n >= 1,
               "linear_split2h_nchw: k must be a multiple of 16");
    MIRX_CHECK(n_img == 0 || (x && w2 && y), "linear_split2h_nchw: null buffer");
    MIRX_CHECK(x != y, "linear_split2h_nchw: y may alias the residual, not the input");
    MIRX_CHECK(x_bound > 0.f && w_inv > 0.f, "linear_split2h_nchw: x_bound and w_inv must be positive");
    MIRX_CHECK(!input_scale_or_null == !input_scale_max_or_null,
               "linear_split2h_nchw: an input scale needs the device scalar that bounds it (and only then)");
    if (input_scale_max_or_null) {
        // the kernel derives 2^s from x_bound * input_scale_max[0]
        MIRX_HIP(launch_linear_h2(x, n_img * tokens_per_image, k, reinterpret_cast<const uint16_t *>(w2), bias_or_null, n, 0,
                                  residual_or_null, input_scale_or_null, x_bound, w_inv, y, tokens_per_image,
                                  input_scale_max_or_null, reinterpret_cast<hipStream_t>(stream)));
    } else {
        int e = 0;                                     // x_bound * 2^s in [2^14, 2^15)
        (void)frexpf(x_bound, &e);                     // x_bound = f * 2^e, f in [0.5, 1)
        const float xs = ldexpf(1.f, 15 - e);
        MIRX_CHECK(std::isfinite(x_bound) && std::isfinite(xs) && xs > 0.f, "linear_split2h_nchw: x_bound out of range");
        MIRX_HIP(launch_linear_h2(x, n_img * tokens_per_image, k, reinterpret_cast<const uint16_t *>(w2), bias_or_null, n, 0,
                                  residual_or_null, nullptr, xs, w_inv / xs, y, tokens_per_image, nullptr,
                                  reinterpret_cast<hipStream_t>(stream)));
    }
    return MIRX_OK;
}

int mirx_linear_split3_nchw(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w3,
                            const float *bias_or_null, int n, const float *residual_or_null,
                            const float *input_scale_or_null, float *y, void *stream) {
    MIRX_CHECK(n_img >= 0 && tokens_per_image >= 1 && k >= 16 && k % 16 == 0 && n >= 1,
               "linear_split3_nchw: k must be a multiple of 16");
    MIRX_CHECK(n_img == 0 || (x && w3 && y), "linear_split3_nchw: null buffer");
    MIRX_CHECK(x != y, "linear_split3_nchw: y may alias the residual, not the input");
    MIRX_HIP(launch_linear_s3(x, n_img * tokens_per_image, k, reinterpret_cast<const uint16_t *>(w3), bias_or_null, n, 0,
                              residual_or_null, input_scale_or_null, y, tokens_per_image,
                              reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_grn_norm_nhwc(const float *x, int64_t n, int hw, int c, float *gx, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && hw >= 1 && c >= 1 && (n == 0 || (x && gx)), "grn_norm: bad argument");
    MIRX_HIP(launch_grn_norm(x, n, hw, c, gx, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_grn_scale(const float *gx, const float *weight, int64_t n, int c, float eps, float *scale, float *scale_max,
                   void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && c >= 1 && eps >= 0.f, "grn_scale: bad argument");
    MIRX_CHECK(n == 0 || (gx && weight && scale && scale_max), "grn_scale: null buffer");
    MIRX_HIP(launch_grn_scale(gx, weight, n, c, eps, scale, scale_max, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}


int mirx_layernorm(const float *x, int64_t m, int c, const float *gamma_or_null, const float *beta_or_null, float eps,
                   float *y, int tokens_per_image, void *stream) {
    MIRX_CHECK(m >= 0 && c >= 4 && c % 4 == 0 && c <= 8192, "layernorm: c must be a multiple of 4, at most 8192");
    MIRX_CHECK(m == 0 || (x && y), "layernorm: null buffer");
    MIRX_CHECK(tokens_per_image >= 0 && (tokens_per_image == 0 || (c <= 512 && x != y)),
               "layernorm: the channels-first form needs c <= 512 and y != x");
    MIRX_CHECK(eps >= 0.f, "layernorm: eps must be non-negative");
    MIRX_HIP(launch_layernorm_rows(x, m, c, gamma_or_null, beta_or_null, eps, y, tokens_per_image,
                                   reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_layernorm_patch2_nhwc(const float *x, int64_t n_img, int h, int w, int c, const float *gamma_or_null,
                               const float *beta_or_null, float eps, float *y, void *stream) {
    MIRX_CHECK(n_img >= 0 && h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "layernorm_patch2_nhwc: h and w must be even");
    MIRX_CHECK(c >= 4 && c % 4 == 0 && c <= 8192, "layernorm_patch2_nhwc: c must be a multiple of 4, at most 8192");
    MIRX_CHECK(n_img == 0 || (x && y), "layernorm_patch2_nhwc: null buffer");
    MIRX_CHECK(x != y && eps >= 0.f, "layernorm_patch2_nhwc: not in place; eps must be non-negative");
    MIRX_HIP(launch_layernorm_rows(x, n_img * h * w, c, gamma_or_null, beta_or_null, eps, y, 0, reinterpret_cast<hipStream_t>(stream),
                                   nullptr, 1.f, w, h));
    return MIRX_OK;
}

int mirx_layernorm_terms(const float *x, int64_t m, int c, const float *gamma_or_null, const float *beta_or_null, float eps,
                         float scale, void *yt, void *stream) {
    MIRX_CHECK(m >= 0 && c >= 4 && c % 4 == 0 && c <= 8160, "layernorm_terms: c must be a multiple of 4, at most 8160");
    MIRX_CHECK(m == 0 || (x && yt), "layernorm_terms: null buffer");
    MIRX_CHECK(eps >= 0.f && scale > 0.f, "layernorm_terms: eps must be non-negative and scale positive");
    MIRX_HIP(launch_layernorm_rows(x, m, c, gamma_or_null, beta_or_null, eps, nullptr, 0, reinterpret_cast<hipStream_t>(stream),
                                   yt, scale));
    return MIRX_OK;
}

int mirx_rows_to_terms(const float *x, int64_t m, int k, int64_t row_stride, float scale, void *xt, void *stream) {
    MIRX_CHECK(m >= 0 && k >= 1 && row_stride >= k && row_stride % 4 == 0, "rows_to_terms: bad geometry (row_stride % 4 == 0)");
    MIRX_CHECK(m == 0 || (x && xt), "rows_to_terms: null buffer");
    MIRX_CHECK((reinterpret_cast<uintptr_t>(x) & 15) == 0, "rows_to_terms: x must be 16-byte aligned");
    MIRX_CHECK(scale > 0.f, "rows_to_terms: scale must be positive");
    MIRX_HIP(launch_rows_to_terms(x, m, k, row_stride, scale, xt, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int64_t mirx_linear_terms_workspace_bytes(int64_t m, int k, int n) { return (int64_t)linear_t2_workspace_bytes(m, k, n); }

int mirx_linear_terms(const void *xt, int64_t m, int k, const void *wt, const float *bias_or_null, int n, int act,
                      const float *residual_or_null, const float *gamma_or_null, float out_scale, float *y_or_null,
                      void *yt_or_null, float yt_scale, void *workspace_or_null, int64_t workspace_bytes, void *stream) {
    MIRX_CHECK(m >= 0 && k >= 1 && n >= 4 && n % 4 == 0, "linear_terms: n must be a multiple of 4");
    MIRX_CHECK(act >= 0 && act <= 2, "linear_terms: act is 0 (none), 1 (GELU) or 2 (tanh GELU)");
    MIRX_CHECK(m == 0 || (xt && wt), "linear_terms: null operand");
    MIRX_CHECK((y_or_null != nullptr) != (yt_or_null != nullptr), "linear_terms: exactly one of y and yt");
    MIRX_CHECK(!(yt_or_null && residual_or_null), "linear_terms: the terms output has no residual form");
    MIRX_CHECK(!(residual_or_null && act), "linear_terms: the residual form has no activation");
    MIRX_CHECK(!gamma_or_null || residual_or_null, "linear_terms: gamma scales the residual form only");
    MIRX_CHECK(!yt_or_null || yt_scale > 0.f, "linear_terms: yt_scale must be positive");
    MIRX_CHECK(workspace_bytes >= 0, "linear_terms: negative workspace size");
    MIRX_HIP(launch_linear_t2(xt, m, k, wt, bias_or_null, n, act, residual_or_null, gamma_or_null, out_scale, y_or_null,
                              yt_or_null, yt_scale, workspace_or_null, workspace_or_null ? (size_t)workspace_bytes : 0,
                              reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_patchify_nchw(const float *x, int64_t n, int c, int h, int w, int patch, const float *ln_gamma_or_null,
                       const float *ln_beta_or_null, float eps, float *out, int row_stride, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && c >= 1 && patch >= 1 && h >= patch && w >= patch, "patchify: bad geometry");
    MIRX_CHECK(row_stride >= c * patch * patch, "patchify: row_stride smaller than c * patch * patch");
    MIRX_CHECK((ln_gamma_or_null == nullptr) == (ln_beta_or_null == nullptr), "patchify: gamma and beta go together");
    MIRX_CHECK(n == 0 || (x && out), "patchify: null buffer");
    MIRX_CHECK((size_t)2 * patch * w * sizeof(float) <= 64 * 1024, "patchify: strip too wide for the LayerNorm2d prologue");
    MIRX_HIP(launch_patchify(x, n, c, h, w, patch, ln_gamma_or_null, ln_beta_or_null, eps, out, row_stride,
                             reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_attention_small(const float *q, int64_t q_row_stride, const float *k, const float *v, int64_t kv_row_stride,
                         const uint8_t *key_mask_or_null, int64_t batch, int heads, int head_dim, int n_queries, int n_keys,
                         float scale, float *out, void *stream) {
    MIRX_CHECK(batch >= 0 && heads >= 1 && n_queries >= 0 && n_keys >= 1, "attention_small: bad sizes");
    MIRX_CHECK(head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 72, "attention_small: head_dim 16 / 32 / 64 / 72");
    MIRX_CHECK(q_row_stride >= (int64_t)heads * head_dim && kv_row_stride >= (int64_t)heads * head_dim &&
                   q_row_stride % 4 == 0 && kv_row_stride % 4 == 0,
               "attention_small: row strides must cover heads * head_dim and be multiples of 4");
    MIRX_CHECK(batch == 0 || n_queries == 0 || (q && k && v && out), "attention_small: null buffer");
    MIRX_HIP(launch_attention_small(q, q_row_stride, k, v, kv_row_stride, key_mask_or_null, batch, heads, head_dim,
                                    n_queries, n_keys, scale, out, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_conv3x3_winograd_nchw(const float *x, const float *u, int64_t n, int side, float *out, int64_t out_batch_stride,
                               void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535, "conv3x3: batch must be in [0, 65535]");
    MIRX_CHECK(side == 56 || side == 28 || side == 14 || side == 7, "conv3x3: side must be 56, 28, 14 or 7");
    MIRX_CHECK(n == 0 || (x && u && out), "conv3x3: null buffer");
    MIRX_CHECK(out_batch_stride >= (int64_t)32 * side * side, "conv3x3: output batch stride too small");
    MIRX_HIP(launch_conv3x3_wino(x, u, n, side, out, out_batch_stride, nullptr, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}



int mirx_conv3x3_winograd_split3_nchw(const float *x, const void *u3, int64_t n, int side, float *out,
                                      int64_t out_batch_stride, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535, "conv3x3_split3: batch must be in [0, 65535]");
    MIRX_CHECK(side == 56 || side == 28 || side == 14, "conv3x3_split3: side must be 56, 28 or 14");
    MIRX_CHECK(n == 0 || (x && u3 && out), "conv3x3_split3: null buffer");
    MIRX_CHECK(out_batch_stride >= (int64_t)32 * side * side, "conv3x3_split3: output batch stride too small");
    MIRX_HIP(launch_conv3x3_wino_s3(x, reinterpret_cast<const uint16_t *>(u3), n, side, out, out_batch_stride,
                                    reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_conv3x3_direct_split3_nchw(const float *x, const void *w3, int64_t n, int side, float *out,
                                    int64_t out_batch_stride, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535, "conv3x3_direct: batch must be in [0, 65535]");
    MIRX_CHECK(side == 56 || side == 28 || side == 14, "conv3x3_direct: side must be 56, 28 or 14");
    MIRX_CHECK(n == 0 || (x && w3 && out), "conv3x3_direct: null buffer");
    MIRX_CHECK(out_batch_stride >= (int64_t)32 * side * side, "conv3x3_direct: output batch stride too small");
    MIRX_HIP(launch_conv3x3_d3(x, reinterpret_cast<const uint16_t *>(w3), n, side, out, out_batch_stride,
                               reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_attention_qkv_f32(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim, float scale,
                           float *out, void *stream) {
    MIRX_CHECK(batch >= 0 && n_tokens >= 0 && heads >= 1, "attention: bad sizes");
    MIRX_CHECK(head_dim == 32 || head_dim == 64 || head_dim == 72 || head_dim == 96,
               "attention: head_dim must be 32, 64, 72 or 96");
    MIRX_CHECK(batch == 0 || n_tokens == 0 || (qkv && out), "attention: null buffer");
    MIRX_CHECK(batch <= 65535 && heads <= 65535, "attention: batch and heads must be <= 65535");
    MIRX_HIP(launch_attention(qkv, batch, n_tokens, heads, head_dim, scale, out, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_attention_qkv_f32_split3(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim, float scale,
                                  float *out, void *stream) {
    MIRX_CHECK(batch >= 0 && n_tokens >= 0 && heads >= 1, "attention_split3: bad sizes");
    MIRX_CHECK(head_dim == 32 || head_dim == 64 || head_dim == 72 || head_dim == 96,
               "attention_split3: head_dim must be 32, 64, 72 or 96");
    MIRX_CHECK(batch <= 65535 && heads <= 65535, "attention_split3: batch and heads must be <= 65535");
    MIRX_CHECK(batch == 0 || n_tokens == 0 || (qkv && out), "attention_split3: null buffer");
    MIRX_HIP(launch_attention_s3(qkv, batch, n_tokens, heads, head_dim, scale, out, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_attention_qkv_f32_split2h(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim, float scale,
                                   float qk_bound, float v_bound, float *out, void *stream) {
    MIRX_CHECK(batch >= 0 && n_tokens >= 0 && heads >= 1, "attention_split2h: bad sizes");
    MIRX_CHECK(head_dim == 64 || head_dim == 72 || head_dim == 96 || head_dim == 32,
               "attention_split2h: head_dim must be 32, 64, 72 or 96");
    MIRX_CHECK(batch <= 65535 && heads <= 65535, "attention_split2h: batch and heads must be <= 65535");
    MIRX_CHECK(batch == 0 || n_tokens == 0 || (qkv && out), "attention_split2h: null buffer");
    MIRX_CHECK(qk_bound > 0.f && v_bound > 0.f && scale > 0.f, "attention_split2h: bounds and scale must be positive");
    MIRX_HIP(launch_attention_h2(qkv, batch, n_tokens, heads, head_dim, scale, qk_bound, v_bound, out,
                                 reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_attention_qkv_f32_split2h_terms(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim, float scale,
                                         float qk_bound, float v_bound, float out_scale, void *out_terms, void *stream) {
    MIRX_CHECK(batch >= 0 && n_tokens >= 0 && heads >= 1, "attention_split2h_terms: bad sizes");
    MIRX_CHECK(head_dim == 64 || head_dim == 72 || head_dim == 96 || head_dim == 32,
               "attention_split2h_terms: head_dim must be 32, 64, 72 or 96");
    MIRX_CHECK(batch <= 65535 && heads <= 65535, "attention_split2h_terms: batch and heads must be <= 65535");
    MIRX_CHECK(batch == 0 || n_tokens == 0 || (qkv && out_terms), "attention_split2h_terms: null buffer");
    MIRX_CHECK(qk_bound > 0.f && v_bound > 0.f && scale > 0.f && out_scale > 0.f,
               "attention_split2h_terms: bounds and scales must be positive");
    MIRX_HIP(launch_attention_h2(qkv, batch, n_tokens, heads, head_dim, scale, qk_bound, v_bound, nullptr,
                                 reinterpret_cast<hipStream_t>(stream), out_terms, out_scale));
    return MIRX_OK;
}

int mirx_rank_metrics(const int64_t *ranks, int64_t nq, int64_t n, int64_t row_stride,
                      const int64_t *gallery_labels, int64_t n_labels, const int64_t *query_labels,
                      const int64_t *query_ids_or_null, int drop_self, int rel_kind, double jaccard_threshold,
                      int ap_kind,
                      const int32_t *kappas, int nk, double *out_ap, int64_t *out_cnt, int64_t *out_nrel,
                      int64_t *out_maxpos, void *stream) {
    MIRX_CHECK(nq >= 0 && n >= 0 && row_stride >= n && n_labels >= 0, "rank_metrics: bad sizes");
    MIRX_CHECK(nq == 0 || (ranks && gallery_labels && query_labels && out_ap && out_nrel && out_maxpos),
               "rank_metrics: null buffer");
    MIRX_CHECK(nk >= 0 && nk <= MIRX_MAX_KAPPAS && (nk == 0 || (kappas && out_cnt)), "rank_metrics: 0 <= nk <= 8");
    MIRX_CHECK((rel_kind == 0 || rel_kind == 1) && (ap_kind == 0 || ap_kind == 1), "rank_metrics: bad kind");
    RankMetricsArgs a{};
    a.ranks = ranks; a.nq = nq; a.n = n; a.row_stride = row_stride;
    a.gallery_labels = gallery_labels; a.n_labels = n_labels; a.query_labels = query_labels;
    a.query_ids = query_ids_or_null; a.drop_self = (drop_self && query_ids_or_null) ? 1 : 0;
    a.jaccard_threshold = jaccard_threshold; a.nk = nk;
    for (int j = 0; j < nk; ++j) {
        MIRX_CHECK(kappas[j] >= 1, "rank_metrics: kappa must be >= 1");
        a.kappas[j] = kappas[j];
    }
    a.out_ap = out_ap; a.out_cnt = out_cnt; a.out_nrel = out_nrel; a.out_maxpos = out_maxpos;
    MIRX_HIP(launch_rank_metrics(a, rel_kind, ap_kind, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

static const char *group_limits(int limit, int group_size) {
    if (limit < 1 || limit > MIRX_GROUP_MAX_LIMIT) return "limit must be in [1, 1024]";
    if (group_size < 1 || group_size > MIRX_GROUP_MAX_SIZE) return "group_size must be in [1, 64]";
    if ((int64_t)limit * group_size > MIRX_GROUP_MAX_HITS) return "limit * group_size must not exceed 16384";
    return nullptr;
}

int mirx_group_walk(const int64_t *ranks, const int64_t *table_index_or_null, const double *scores_or_null, int64_t nq, int64_t depth,
                    int64_t row_stride, const int64_t *group_of, int64_t n_table, const int64_t *group_rows, int64_t n_groups,
                    int64_t live_groups, const int64_t *excl_group_or_null, int limit, int group_size, int64_t *out_ids,
                    double *out_scores_or_null, int64_t *out_codes, int32_t *out_kept, int32_t *out_state, void *stream) {
    if (const char *why = group_limits(limit, group_size)) return fail(MIRX_EINVAL, std::string("group_walk: ") + why);
    MIRX_CHECK(nq >= 0 && depth >= 0 && row_stride >= depth && n_table >= 0, "group_walk: bad sizes");
    MIRX_CHECK(n_groups >= 0 && n_groups <= 0x7FFFFFFFll && live_groups >= 0 && live_groups <= n_groups,
               "group_walk: 0 <= live_groups <= n_groups < 2^31");
    MIRX_CHECK(nq == 0 || (out_ids && out_codes && out_kept && out_state), "group_walk: null output");
    MIRX_CHECK(nq == 0 || depth == 0 || ranks, "group_walk: null ranks");
    MIRX_CHECK(nq == 0 || ((group_of || n_table == 0) && (group_rows || n_groups == 0)), "group_walk: null table");
    MIRX_CHECK(!out_scores_or_null || scores_or_null || depth == 0, "group_walk: out_scores without scores");
    GroupWalkArgs a{};
    a.ranks = ranks; a.table_index = table_index_or_null; a.scores = out_scores_or_null ? scores_or_null : nullptr;
    a.nq = nq; a.depth = depth; a.row_stride = row_stride;
    a.group_of = group_of; a.n_table = n_table; a.group_rows = group_rows; a.n_groups = n_groups; a.live_groups = live_groups;
    a.excl_group = excl_group_or_null; a.limit = limit; a.group_size = group_size;
    a.out_ids = out_ids; a.out_scores = out_scores_or_null; a.out_codes = out_codes; a.out_kept = out_kept; a.out_state = out_state;
    MIRX_HIP(launch_group_walk(a, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_group_count(const int64_t *groups, const uint8_t *allow_or_null, int64_t n, int64_t n_groups, int64_t *out_counts, void *stream) {
    MIRX_CHECK(n >= 0 && n_groups >= 0 && n_groups <= 0x7FFFFFFFll, "group_count: bad sizes");
    MIRX_CHECK((groups || n == 0) && (out_counts || n_groups == 0), "group_count: null buffer");
    if (n_groups == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MIRX_HIP(hipMemsetAsync(out_counts, 0, (size_t)n_groups * sizeof(int64_t), st));
    MIRX_HIP(launch_group_count(groups, allow_or_null, n, n_groups, out_counts, st));
    return MIRX_OK;
}

int mirx_index_group_fill(mirx_index *ix, const float *q, int64_t nq, const int64_t *exclude_ids_or_null, int limit, int group_size,
                          const int64_t *pair_query, const int64_t *pair_slot, const int64_t *pair_first, const int64_t *pair_len,
                          int64_t n_pairs, const int64_t *members, int64_t n_members, int max_members, int64_t *out_ids,
                          double *out_rank_scores, void *stream) {
    MIRX_CHECK(ix, "group_fill: null index");
    if (const char *why = group_limits(limit, group_size)) return fail(MIRX_EINVAL, std::string("group_fill: ") + why);
    MIRX_CHECK(nq >= 0 && nq <= 0x7FFFFF00ll && n_pairs >= 0 && n_pairs <= 0x7FFFFFFFll && n_members >= 0, "group_fill: bad sizes");
    MIRX_CHECK(max_members >= 1 && max_members <= MIRX_GROUP_FILL_MAX, "group_fill: max_members must be in [1, 4096]");
    MIRX_CHECK(n_pairs == 0 || (q && pair_query && pair_slot && pair_first && pair_len && members && out_ids && out_rank_scores),
               "group_fill: null buffer");
    if (ix->pend.active || ix->begun)
        return fail(MIRX_ESTATE, "group_fill: a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    if (n_pairs == 0 || nq == 0) return MIRX_OK;
    ix->range_valid = false;
    DeviceGuard dg(ix->device);
    if (!dg.ok) return fail(MIRX_EHIP, "group_fill: cannot select the index device");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    MIRX_HIP(ix->q32p.ensure((size_t)nq * ix->dimp * sizeof(float)));
    MIRX_HIP(ix->q16.ensure((size_t)nq * ix->dimp * sizeof(uint16_t)));
    MIRX_HIP(ix->qnorm.ensure((size_t)nq * sizeof(float)));
    MIRX_HIP(launch_prep_queries(q, nq, nq, ix->dim, ix->dimp, ix->q32p.as<float>(), ix->q16.as<uint16_t>(), ix->qnorm.as<float>(), st));
    GroupFillArgs a{};
    a.q32p = ix->q32p.as<float>(); a.g32 = ix->g32; a.ids = ix->ids; a.exclude = exclude_ids_or_null;
    a.nq = nq; a.n_rows = ix->size; a.dimp = ix->dimp; a.limit = limit; a.group_size = group_size;
    a.pair_query = pair_query; a.pair_slot = pair_slot; a.pair_first = pair_first; a.pair_len = pair_len; a.n_pairs = n_pairs;
    a.members = members; a.n_members = n_members; a.max_members = max_members;
    a.out_ids = out_ids; a.out_f64 = out_rank_scores;
    MIRX_HIP(launch_group_fill(a, ix->metric, st));
    return MIRX_OK;
}

int mirx_fuse_ranked(const int64_t *codes, const float *distances_or_null, int64_t nq, int64_t row_stride, int64_t n_codes,
                     const int32_t *segment_offsets, int n_requests, int ranker, double rrf_k, const double *weights_or_null,
                     const int32_t *norms_or_null, int limit, int64_t *out_codes, double *out_scores, int32_t *out_request,
                     int32_t *out_slot, int32_t *out_count, void *stream) {
    MIRX_CHECK(n_requests >= 1 && n_requests <= MIRX_FUSE_MAX_REQUESTS, "fuse_ranked: n_requests must be in [1, 8]");
    MIRX_CHECK(limit >= 1 && limit <= MIRX_FUSE_MAX_LIMIT, "fuse_ranked: limit must be in [1, 1024]");
    MIRX_CHECK(segment_offsets, "fuse_ranked: null segment_offsets");
    MIRX_CHECK(segment_offsets[0] == 0, "fuse_ranked: segment_offsets must start at 0");
    FuseArgs a{};
    for (int r = 0; r < n_requests; ++r) {
        MIRX_CHECK(segment_offsets[r + 1] > segment_offsets[r], "fuse_ranked: segment_offsets must ascend (every list has a slot)");
        MIRX_CHECK(segment_offsets[r + 1] <= MIRX_FUSE_MAX_ENTRIES, "fuse_ranked: the lists hold more than 4096 entries together");
    }
    for (int r = 0; r <= n_requests; ++r) a.offsets[r] = segment_offsets[r];
    a.m = segment_offsets[n_requests]; a.n_requests = n_requests;
    MIRX_CHECK(nq >= 0 && nq <= 0x7FFFFFFFll && row_stride >= a.m, "fuse_ranked: bad sizes (0 <= nq < 2^31, row_stride >= m)");
    MIRX_CHECK(n_codes >= 0 && n_codes <= 0x7FFFFFFFll, "fuse_ranked: n_codes must be in [0, 2^31)");
    MIRX_CHECK(ranker == MIRX_FUSE_RRF || ranker == MIRX_FUSE_WEIGHTED, "fuse_ranked: unknown ranker");
    if (ranker == MIRX_FUSE_RRF) {
        MIRX_CHECK(rrf_k > 0.0 && rrf_k < 16384.0, "fuse_ranked: rrf_k must be in (0, 16384)");
        a.rrf_k = rrf_k;
    } else {
        MIRX_CHECK(weights_or_null && norms_or_null, "fuse_ranked: the weighted ranker needs weights and norms");
        for (int r = 0; r < n_requests; ++r) {
            MIRX_CHECK(weights_or_null[r] >= 0.0 && weights_or_null[r] <= 1.0, "fuse_ranked: a weight must be in [0, 1]");
            MIRX_CHECK(norms_or_null[r] >= MIRX_FUSE_NORM_RAW && norms_or_null[r] <= MIRX_FUSE_NORM_L2, "fuse_ranked: unknown norm");
            a.weights[r] = weights_or_null[r];
            a.norms[r] = norms_or_null[r];
        }
        MIRX_CHECK(nq == 0 || distances_or_null, "fuse_ranked: the weighted ranker needs distances");
    }
    MIRX_CHECK(nq == 0 || codes, "fuse_ranked: null codes");
    MIRX_CHECK(nq == 0 || (out_codes && out_scores && out_request && out_slot && out_count), "fuse_ranked: null output");
    a.codes = codes; a.distances = distances_or_null; a.nq = nq; a.row_stride = row_stride; a.n_codes = n_codes;
    a.ranker = ranker; a.limit = limit;
    a.out_codes = out_codes; a.out_scores = out_scores; a.out_request = out_request; a.out_slot = out_slot; a.out_count = out_count;
    MIRX_HIP(launch_fuse_ranked(a, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_l2_normalize(float *x, int64_t n, int dim, void *stream) {
    MIRX_CHECK(x && n >= 0 && dim >= 1, "l2_normalize: bad argument");
    MIRX_HIP(launch_l2_normalize(x, n, dim, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_bn_relu_gap_l2norm(const float *x, const float *scale, const float *shift, int64_t n, int c,
                            int hw, int normalize, float *y, void *stream) {
    MIRX_CHECK(x && y && n >= 0 && c >= 1 && c <= 16384 && hw >= 1, "bn_relu_gap_l2norm: bad argument");
    MIRX_HIP(launch_bn_relu_gap_l2norm(x, scale, shift, n, c, hw, normalize, y,
                                       reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_bn_relu_nchw(const float *x, int64_t x_batch_stride, const float *scale, const float *shift,
                      int64_t n, int c, int hw, float *y, void *stream) {
    MIRX_CHECK(x && scale && shift && y && n >= 0 && c >= 1 && hw >= 1, "bn_relu_nchw: bad argument");
    MIRX_CHECK(((int64_t)c * hw) % 4 == 0 && x_batch_stride % 4 == 0 && x_batch_stride >= (int64_t)c * hw,
               "bn_relu_nchw: c*hw and the batch stride must be multiples of 4");
    MIRX_HIP(launch_bn_relu_nchw(x, x_batch_stride, scale, shift, n, c, hw, y,
                                 reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_bn_relu_avgpool2(const float *x, int64_t x_batch_stride, const float *scale, const float *shift,
                          int64_t n, int c, int h, int w, float *y, int64_t x_plane_stride, void *stream) {
    MIRX_CHECK(x && scale && shift && y && n >= 0 && c >= 1, "bn_relu_avgpool2: bad argument");
    MIRX_CHECK(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && x_batch_stride % 2 == 0,
               "bn_relu_avgpool2: h, w and the batch stride must be even");
    MIRX_CHECK(x_plane_stride == 0 || (x_plane_stride >= (int64_t)h * w && x_plane_stride % 4 == 0),
               "bn_relu_avgpool2: the plane stride is 0 (= h * w) or a multiple of 4 that is at least h * w");
    MIRX_HIP(launch_bn_relu_avgpool2(x, x_batch_stride, scale, shift, n, c, h, w, y, x_plane_stride,
                                     reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_bn_relu_avgpool2_into(const float *x, int64_t x_batch_stride, const float *scale, const float *shift,
                               int64_t n, int c, int h, int w, float *y, int64_t y_batch_stride, int64_t x_plane_stride,
                               void *stream) {
    MIRX_CHECK(x && scale && shift && y && n >= 0 && c >= 1, "bn_relu_avgpool2_into: bad argument");
    MIRX_CHECK(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0 && x_batch_stride % 2 == 0,
               "bn_relu_avgpool2_into: h, w and the batch stride must be even");
    MIRX_CHECK(x_plane_stride == 0 || (x_plane_stride >= (int64_t)h * w && x_plane_stride % 4 == 0),
               "bn_relu_avgpool2_into: the plane stride is 0 (= h * w) or a multiple of 4 that is at least h * w");
    MIRX_CHECK(y_batch_stride >= (int64_t)c * (h / 2) * (w / 2) && y_batch_stride % 2 == 0,
               "bn_relu_avgpool2_into: the output batch stride must be even and at least c * (h / 2) * (w / 2)");
    MIRX_HIP(launch_bn_relu_avgpool2(x, x_batch_stride, scale, shift, n, c, h, w, y, x_plane_stride,
                                     reinterpret_cast<hipStream_t>(stream), y_batch_stride));
    return MIRX_OK;
}

int mirx_stem_conv7_bn_relu_pool(const float *x, const float *w, const float *scale, const float *shift,
                                 int64_t n, int h, int wd, float *y, void *stream) {
    MIRX_CHECK(x && w && scale && shift && y && n >= 0, "stem: null argument");
    MIRX_CHECK(h >= 8 && wd >= 8 && h % 4 == 0 && wd % 4 == 0, "stem: H and W must be multiples of 4");
    MIRX_HIP(launch_stem(x, w, scale, shift, n, h, wd, y, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_stem_conv7_bn_relu_pool_split3(const float *x, const void *w3, const float *scale, const float *shift,
                                        int64_t n, int h, int wd, float *y, void *stream) {
    MIRX_CHECK(x && w3 && scale && shift && y && n >= 0 && n <= 65535, "stem_split3: null argument or batch > 65535");
    MIRX_CHECK(h >= 8 && wd >= 8 && h % 4 == 0 && wd % 4 == 0, "stem_split3: H and W must be multiples of 4");
    MIRX_HIP(launch_stem_s3(x, reinterpret_cast<const uint16_t *>(w3), scale, shift, n, h, wd, y,
                            (int64_t)64 * (h / 4) * (wd / 4), nullptr, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_range_absmax(const float *x, int64_t per_image, int64_t n, float *range_row, void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && per_image >= 0, "range_absmax: batch must be in [0, 65535]");
    MIRX_CHECK(n == 0 || per_image == 0 || (x && range_row), "range_absmax: null buffer");
    MIRX_HIP(launch_range_absmax(x, per_image, n, range_row, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_range_absmax_u8(const uint8_t *x, int64_t hw, int64_t n, const float *mean3, const float *std3, float *range_row,
                         void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && hw >= 0, "range_absmax_u8: batch must be in [0, 65535]");
    MIRX_CHECK(n == 0 || hw == 0 || (x && mean3 && std3 && range_row), "range_absmax_u8: null buffer");
    MIRX_HIP(launch_range_absmax_u8(x, hw, n, mean3, std3, range_row, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_stem_conv7_bn_relu_pool_split2h_u8_into(const uint8_t *x, const float *mean3, const float *std3, const void *w2,
                                                 const float *oscale, const float *scale, const float *shift, int64_t n, int h,
                                                 int wd, float *y, int64_t y_batch_stride, const float *in_range,
                                                 float *out_range_or_null, void *stream) {
    MIRX_CHECK(x && mean3 && std3 && w2 && oscale && scale && shift && y && in_range && n >= 0 && n <= 65535,
               "stem_split2h_u8: null argument or batch > 65535");
    MIRX_CHECK(h >= 8 && wd >= 8 && h % 4 == 0 && wd % 4 == 0, "stem_split2h_u8: H and W must be multiples of 4");
    MIRX_CHECK(y_batch_stride >= (int64_t)64 * (h / 4) * (wd / 4), "stem_split2h_u8: output batch stride too small");
    MIRX_HIP(launch_stem_h2_u8(x, mean3, std3, reinterpret_cast<const uint16_t *>(w2), oscale, scale, shift, n, h, wd, y,
                               y_batch_stride, in_range, out_range_or_null, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_stem_conv7_bn_relu_pool_split2h_into(const float *x, const void *w2, const float *oscale, const float *scale,
                                              const float *shift, int64_t n, int h, int wd, float *y, int64_t y_batch_stride,
                                              const float *in_range, float *out_range_or_null, void *stream) {
    MIRX_CHECK(x && w2 && oscale && scale && shift && y && in_range && n >= 0 && n <= 65535,
               "stem_split2h: null argument or batch > 65535");
    MIRX_CHECK(h >= 8 && wd >= 8 && h % 4 == 0 && wd % 4 == 0, "stem_split2h: H and W must be multiples of 4");
    MIRX_CHECK(y_batch_stride >= (int64_t)64 * (h / 4) * (wd / 4), "stem_split2h: output batch stride too small");
    MIRX_HIP(launch_stem_h2(x, reinterpret_cast<const uint16_t *>(w2), oscale, scale, shift, n, h, wd, y, y_batch_stride,
                            in_range, out_range_or_null, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}


int mirx_conv1x1_bn_relu(const float *x, int64_t x_batch_stride, int cin, const float *scale, const float *shift,
                         const float *wt, const float *bias, int64_t n, int hw, int cout, int relu_out, float *y,
                         void *stream) {
    MIRX_CHECK(x && wt && y && n >= 0 && hw >= 1, "conv1x1: null argument");
    MIRX_CHECK((scale == nullptr) == (shift == nullptr), "conv1x1: scale and shift go together");
    MIRX_CHECK(cin >= 32 && cin % 32 == 0 && cout >= 128 && cout % 128 == 0, "conv1x1: cin % 32 and cout % 128 must be 0");
    MIRX_CHECK(x_batch_stride >= (int64_t)cin * hw, "conv1x1: batch stride smaller than cin * hw");
    MIRX_HIP(launch_conv1x1(x, x_batch_stride, cin, scale, shift, wt, bias, n, hw, cout, relu_out, y,
                            reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_dwconv7x7_nhwc(const float *x, const float *w_taps_first, const float *bias, int64_t n, int c, int h, int wd, float *y,
                        void *stream) {
    MIRX_CHECK(n >= 0 && n <= 65535 && c >= 1 && h >= 1 && wd >= 1, "dwconv7x7_nhwc: bad geometry (n <= 65535)");
    MIRX_CHECK((int64_t)h * wd * c <= 0x7fffffff, "dwconv7x7_nhwc: one image must stay below 2^31 elements");
    MIRX_CHECK(n == 0 || (x && w_taps_first && y), "dwconv7x7_nhwc: null buffer");
    MIRX_CHECK(x != y, "dwconv7x7_nhwc: in place is not supported");
    MIRX_HIP(launch_dwconv7_nhwc(x, w_taps_first, bias, n, c, h, wd, y, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_dwconv7x7_nchw_to_nhwc(const float *x, const float *w, const float *bias, int64_t n, int c, int h,
                                int wd, float *y, void *stream) {
    MIRX_CHECK(x && w && y && n >= 0 && c >= 1 && h >= 1 && wd >= 1, "dwconv7x7: bad argument");
    MIRX_HIP(launch_dwconv7(x, w, bias, n, c, h, wd, y, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

// ---- anomaly evaluation (k_anomaly.hip) -----------------------------------------------------------------------------------------
static const char *anomaly_rows_limits(int64_t n, int d, int k) {
    if (n < 1 || n > MIRX_ANOMALY_MAX_N) return "anomaly: n must be in [1, 2^30]";
    if (d < 1 || d > MIRX_ANOMALY_MAX_D) return "anomaly: d must be in [1, 16384]";
    if (k < 1 || k > MIRX_ANOMALY_MAX_K) return "anomaly: k must be in [1, 64]";
    return nullptr;
}

static const char *anomaly_metric_limits(int64_t s, int64_t n) {
    if (n < 1 || n > MIRX_ANOMALY_MAX_N) return "binary_rank_metrics: n must be in [1, 2^30]";
    if (s < 1 || s > MIRX_ANOMALY_MAX_SEGMENTS) return "binary_rank_metrics: s must be in [1, 65535]";
    return nullptr;
}

static bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int64_t mirx_class_centroids_workspace_bytes(int64_t n, int d, int k) {
    if (const char *msg = anomaly_rows_limits(n, d, k)) return fail(MIRX_EINVAL, msg);
    return class_centroids_workspace_bytes(n, d, k);
}

int mirx_class_centroids(const float *rows, int64_t n, int d, const int64_t *labels, const int64_t *classes, int k, void *workspace,
                         int64_t workspace_bytes, double *centroids, int64_t *counts, int *bad_flag, void *stream) {
    if (const char *msg = anomaly_rows_limits(n, d, k)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(rows && labels && classes && workspace && centroids && counts && bad_flag, "class_centroids: null buffer");
    MIRX_CHECK(aligned_to(rows, 4) && aligned_to(labels, 8) && aligned_to(centroids, 8) && aligned_to(counts, 8) &&
                   aligned_to(bad_flag, 4) && aligned_to(workspace, 256),
               "class_centroids: misaligned buffer (workspace: 256 bytes)");
    MIRX_CHECK(workspace_bytes >= class_centroids_workspace_bytes(n, d, k),
               "class_centroids: workspace smaller than mirx_class_centroids_workspace_bytes()");
    MIRX_HIP(launch_class_centroids(rows, n, d, labels, classes, k, workspace, centroids, counts, bad_flag,
                                    reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_centroid_min_dist(const float *rows, int64_t n, int d, const double *centroids, int k, double *dist, int32_t *nearest,
                           double *max_out, void *stream) {
    if (const char *msg = anomaly_rows_limits(n, d, k)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(rows && centroids && dist && nearest && max_out, "centroid_min_dist: null buffer");
    MIRX_CHECK(aligned_to(rows, 4) && aligned_to(centroids, 8) && aligned_to(dist, 8) && aligned_to(nearest, 4) && aligned_to(max_out, 8),
               "centroid_min_dist: misaligned buffer");
    MIRX_HIP(launch_centroid_min_dist(rows, n, d, centroids, k, dist, nearest, max_out, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int64_t mirx_binary_rank_metrics_workspace_bytes(int64_t s, int64_t n) {
    if (const char *msg = anomaly_metric_limits(s, n)) return fail(MIRX_EINVAL, msg);
    return binary_rank_metrics_workspace_bytes(s, n);
}

int mirx_binary_rank_metrics(const double *scores, const uint8_t *positive, int64_t s, int64_t n, const double *norm_or_null,
                             double recall_level, void *workspace, int64_t workspace_bytes, double *thresholds, int64_t *tps,
                             int64_t *fps, int64_t *out_t, double *out_auroc, double *out_aupr, double *out_fpr, int *bad_flag,
                             void *stream) {
    if (const char *msg = anomaly_metric_limits(s, n)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(recall_level >= 0.0 && recall_level <= 1.0, "binary_rank_metrics: recall_level must be in [0, 1]");
    MIRX_CHECK(scores && positive && workspace && thresholds && tps && fps && out_t && out_auroc && out_aupr && out_fpr && bad_flag,
               "binary_rank_metrics: null buffer");
    MIRX_CHECK(aligned_to(scores, 8) && aligned_to(norm_or_null, 8) && aligned_to(thresholds, 8) && aligned_to(tps, 8) &&
                   aligned_to(fps, 8) && aligned_to(out_t, 8) && aligned_to(out_auroc, 8) && aligned_to(out_aupr, 8) &&
                   aligned_to(out_fpr, 8) && aligned_to(bad_flag, 4) && aligned_to(workspace, 256),
               "binary_rank_metrics: misaligned buffer (workspace: 256 bytes)");
    MIRX_CHECK(workspace_bytes >= binary_rank_metrics_workspace_bytes(s, n),
               "binary_rank_metrics: workspace smaller than mirx_binary_rank_metrics_workspace_bytes()");
    MIRX_HIP(launch_binary_rank_metrics(scores, positive, s, n, norm_or_null, recall_level, workspace, thresholds, tps, fps, out_t,
                                        out_auroc, out_aupr, out_fpr, bad_flag, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

// ---- insertion / deletion curves (k_insdel.hip) ---------------------------------------------------------------------------------
static const char *insdel_steps_limits(int64_t k, int64_t hw) {
    if (hw < 1 || hw > MIRX_INSDEL_MAX_HW) return "insdel_steps: hw must be in [1, 2^20]";
    if (k < 1 || k > MIRX_INSDEL_MAX_K) return "insdel_steps: k must be in [1, 65535]";
    return nullptr;
}

int64_t mirx_insdel_steps_workspace_bytes(int64_t k, int64_t hw) {
    if (const char *msg = insdel_steps_limits(k, hw)) return fail(MIRX_EINVAL, msg);
    return insdel_steps_workspace_bytes(k, hw);
}

int mirx_insdel_steps(const float *sal, int64_t k, int64_t hw, int64_t step, void *workspace, int64_t workspace_bytes, int32_t *t,
                      void *stream) {
    if (const char *msg = insdel_steps_limits(k, hw)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(step >= 1, "insdel_steps: step must be >= 1");
    MIRX_CHECK(sal && workspace && t, "insdel_steps: null buffer");
    MIRX_CHECK(aligned_to(sal, 4) && aligned_to(t, 4) && aligned_to(workspace, 256), "insdel_steps: misaligned buffer (workspace: 256 bytes)");
    MIRX_CHECK(workspace_bytes >= insdel_steps_workspace_bytes(k, hw),
               "insdel_steps: workspace smaller than mirx_insdel_steps_workspace_bytes()");
    MIRX_HIP(launch_insdel_steps(sal, k, hw, step, workspace, t, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_blur2d_same(const float *x, int64_t n, int c, int h, int w, const float *kernel, int klen, float *y, void *stream) {
    MIRX_CHECK(klen >= 1 && klen <= MIRX_BLUR_MAX_KLEN && (klen & 1), "blur2d_same: klen must be odd and in [1, 63]");
    MIRX_CHECK(n >= 0 && c >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "blur2d_same: needs n >= 0, c >= 1, 1 <= h, w <= 16384");
    MIRX_CHECK(n <= INT32_MAX && blur2d_blocks(n * c, h, w) <= INT32_MAX, "blur2d_same: more than 2^31 - 1 workgroups");
    MIRX_CHECK(x && kernel && y, "blur2d_same: null buffer");
    MIRX_CHECK(aligned_to(x, 4) && aligned_to(kernel, 4) && aligned_to(y, 4), "blur2d_same: misaligned buffer");
    MIRX_HIP(launch_blur2d_same(x, n * c, h, w, kernel, klen, y, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_insdel_compose(const int32_t *t, int64_t n_rows, int64_t hw, const float *bank, int64_t n_bank, const int32_t *start,
                        const int32_t *finish, const int32_t *row, int64_t n_curves, int64_t n_steps, int64_t g0, int64_t n,
                        float *out, void *stream) {
    MIRX_CHECK(hw >= 1 && hw <= MIRX_INSDEL_MAX_HW, "insdel_compose: hw must be in [1, 2^20]");
    MIRX_CHECK(n_rows >= 1 && n_rows <= INT32_MAX && n_bank >= 1 && n_bank <= INT32_MAX && n_curves >= 1 && n_curves <= INT32_MAX,
               "insdel_compose: n_rows, n_bank and n_curves must be in [1, 2^31)");
    MIRX_CHECK(n_steps >= 1 && n_steps <= MIRX_INSDEL_MAX_HW, "insdel_compose: n_steps must be in [1, 2^20]");
    MIRX_CHECK(g0 >= 0 && n >= 0 && n <= INT32_MAX && g0 + n <= n_curves * (n_steps + 1),
               "insdel_compose: [g0, g0 + n) must lie within the job's n_curves * (n_steps + 1) images");
    MIRX_CHECK(t && bank && start && finish && row && out, "insdel_compose: null buffer");
    MIRX_CHECK(aligned_to(t, 4) && aligned_to(bank, 4) && aligned_to(start, 4) && aligned_to(finish, 4) && aligned_to(row, 4) &&
                   aligned_to(out, 4),
               "insdel_compose: misaligned buffer");
    MIRX_HIP(launch_insdel_compose(t, n_rows, hw, bank, n_bank, start, finish, row, n_steps, g0, n, out,
                                   reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_insdel_curves(const float *q_feat, const float *r_feats, int64_t n_curves, int64_t n_steps, int d, double *scores,
                       double *auc, int64_t *zero_counter, void *stream) {
    MIRX_CHECK(d >= 1 && d <= (1 << 20), "insdel_curves: d must be in [1, 2^20]");
    MIRX_CHECK(n_curves >= 1 && n_steps >= 1 && n_curves <= (1LL << 30) && n_steps <= (1LL << 30) &&
                   n_curves * (n_steps + 1) <= (1LL << 30),
               "insdel_curves: needs n_curves, n_steps >= 1 and n_curves * (n_steps + 1) <= 2^30");
    MIRX_CHECK(q_feat && r_feats && scores && auc && zero_counter, "insdel_curves: null buffer");
    MIRX_CHECK(aligned_to(q_feat, 4) && aligned_to(r_feats, 4) && aligned_to(scores, 8) && aligned_to(auc, 8) && aligned_to(zero_counter, 8),
               "insdel_curves: misaligned buffer");
    MIRX_HIP(launch_insdel_curves(q_feat, r_feats, n_curves, n_steps, d, scores, auc, zero_counter,
                                  reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

// ---- SBSM occlusion saliency (k_sbsm.hip) ---------------------------------------------------------------------------------------
static const char *sbsm_grid_limits(int h, int w, int nr, int nc) {
    if (h < 1 || w < 1 || (int64_t)h * w > MIRX_SBSM_MAX_HW) return "sbsm: needs h, w >= 1 and h * w <= 2^20";
    if (nr < 1 || nr > MIRX_SBSM_MAX_WINDOWS || nc < 1 || nc > MIRX_SBSM_MAX_WINDOWS) return "sbsm: nr and nc must be in [1, 4096]";
    return nullptr;
}

int mirx_sbsm_compose(const float *x, int64_t b, int c, int h, int w, const int32_t *row_iv, int nr, const int32_t *col_iv, int nc,
                      int64_t g0, int64_t n, float *out, void *stream) {
    if (const char *msg = sbsm_grid_limits(h, w, nr, nc)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(c >= 1 && (int64_t)c * h * w <= (1LL << 30), "sbsm_compose: needs c >= 1 and c * h * w <= 2^30");
    MIRX_CHECK(b >= 1 && b <= INT32_MAX, "sbsm_compose: b must be in [1, 2^31)");
    MIRX_CHECK(g0 >= 0 && n >= 0 && n <= INT32_MAX && g0 <= (int64_t)nr * nc * b && n <= (int64_t)nr * nc * b - g0,
               "sbsm_compose: [g0, g0 + n) must lie within the job's nr * nc * b images");
    MIRX_CHECK(x && row_iv && col_iv && out, "sbsm_compose: null buffer");
    MIRX_CHECK(aligned_to(x, 4) && aligned_to(row_iv, 4) && aligned_to(col_iv, 4) && aligned_to(out, 4), "sbsm_compose: misaligned buffer");
    MIRX_HIP(launch_sbsm_compose(x, b, c, h, w, row_iv, col_iv, nc, g0, n, out, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_sbsm_gain(const float *e_q, int64_t q, const float *e_m, int64_t n_masks, int64_t b, const float *e_r_or_null, int d,
                   double *gain, void *stream) {
    MIRX_CHECK(d >= 1 && d <= MIRX_SBSM_MAX_D, "sbsm_gain: d must be in [1, 16384]");
    MIRX_CHECK(q >= 1 && b >= 1 && n_masks >= 1 && q <= (1LL << 30) && b <= (1LL << 30) && n_masks <= (1LL << 30),
               "sbsm_gain: q, b and n_masks must be in [1, 2^30]");
    MIRX_CHECK(e_r_or_null || q == b, "sbsm_gain: self-similarity (null e_r) needs q == b");
    const int64_t rows = e_r_or_null ? q * b : b;
    MIRX_CHECK(rows <= (1LL << 30) && rows * n_masks <= (1LL << 30) && n_masks * b <= (1LL << 30),
               "sbsm_gain: needs rows * n_masks <= 2^30 and n_masks * b <= 2^30");
    MIRX_CHECK(e_q && e_m && gain, "sbsm_gain: null buffer");
    MIRX_CHECK(aligned_to(e_q, 4) && aligned_to(e_m, 4) && aligned_to(e_r_or_null, 4) && aligned_to(gain, 8), "sbsm_gain: misaligned buffer");
    MIRX_HIP(launch_sbsm_gain(e_q, e_m, e_r_or_null, rows, n_masks, b, d, gain, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

static const char *sbsm_accumulate_limits(int64_t rows, int nr, int w) {
    if (nr < 1 || nr > MIRX_SBSM_MAX_WINDOWS || w < 1 || w > MIRX_SBSM_MAX_HW) return "sbsm_accumulate: needs 1 <= nr <= 4096 and 1 <= w <= 2^20";
    if ((int64_t)nr * w > (1LL << 30)) return "sbsm_accumulate: needs nr * w <= 2^30";
    if (rows < 1 || rows > (1LL << 30) || rows * nr * (int64_t)w > (1LL << 40)) return "sbsm_accumulate: needs rows >= 1 and rows * nr * w <= 2^40";
    return nullptr;
}

int64_t mirx_sbsm_workspace_bytes(int64_t rows, int nr, int w) {
    if (const char *msg = sbsm_accumulate_limits(rows, nr, w)) return fail(MIRX_EINVAL, msg);
    return sbsm_workspace_bytes(rows, nr, w);
}

int mirx_sbsm_accumulate(const double *gain, int64_t rows, const int32_t *row_iv, int nr, const int32_t *col_iv, int nc, int h, int w,
                         void *workspace, int64_t workspace_bytes, float *sal, void *stream) {
    if (const char *msg = sbsm_grid_limits(h, w, nr, nc)) return fail(MIRX_EINVAL, msg);
    if (const char *msg = sbsm_accumulate_limits(rows, nr, w)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(rows * nr * (int64_t)nc <= (1LL << 30), "sbsm_accumulate: needs rows * nr * nc <= 2^30");
    MIRX_CHECK(gain && row_iv && col_iv && workspace && sal, "sbsm_accumulate: null buffer");
    MIRX_CHECK(aligned_to(gain, 8) && aligned_to(row_iv, 4) && aligned_to(col_iv, 4) && aligned_to(workspace, 8) && aligned_to(sal, 4),
               "sbsm_accumulate: misaligned buffer (workspace: 8 bytes)");
    MIRX_CHECK(workspace_bytes >= sbsm_workspace_bytes(rows, nr, w), "sbsm_accumulate: workspace smaller than mirx_sbsm_workspace_bytes()");
    MIRX_HIP(launch_sbsm_accumulate(gain, rows, row_iv, nr, col_iv, nc, h, w, workspace, sal, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

// ---- batched Resize + CenterCrop (k_resample.hip) -------------------------------------------------------------------------------
static const char *resample_axis_limits(int in_size, int out_size, int filter) {
    if (filter != MIRX_RESAMPLE_BILINEAR && filter != MIRX_RESAMPLE_BICUBIC)
        return "resample: unknown filter (MIRX_RESAMPLE_BILINEAR = 0, MIRX_RESAMPLE_BICUBIC = 1)";
    if (in_size < 1 || in_size > MIRX_RESAMPLE_MAX_SIDE) return "resample: source side outside [1, MIRX_RESAMPLE_MAX_SIDE = 8192]";
    if (out_size < 1 || out_size > MIRX_RESAMPLE_MAX_RESIZED) return "resample: resized side outside [1, 2^24]";
    if (resample_taps(in_size, out_size, filter) > MIRX_RESAMPLE_MAX_TAPS)
        return filter == MIRX_RESAMPLE_BILINEAR ? "resample: tap count over the cap (MIRX_RESAMPLE_MAX_TAPS = 65: scale > 32)"
                                                : "resample: tap count over the cap (MIRX_RESAMPLE_MAX_TAPS = 65: bicubic scale > 16)";
    return nullptr;
}

int mirx_resample_taps_filter(int in_size, int out_size, int filter) {
    if (const char *msg = resample_axis_limits(in_size, out_size, filter)) return fail(MIRX_EINVAL, msg);
    return resample_taps(in_size, out_size, filter);
}

int mirx_resample_plan_filter(int in_size, int out_size, int first, int n, int filter, int32_t *table, int64_t table_words) {
    if (const char *msg = resample_axis_limits(in_size, out_size, filter)) return fail(MIRX_EINVAL, msg);
    MIRX_CHECK(n >= 1 && n <= MIRX_RESAMPLE_MAX_OUT && first >= 0 && first <= out_size - n,
               "resample_plan: the window [first, first + n) must lie inside the resized axis, n in [1, 1024]");
    MIRX_CHECK(table && aligned_to(table, 4), "resample_plan: null or misaligned table");
    MIRX_CHECK(table_words >= 4 + 2 * (int64_t)n + (int64_t)n * resample_taps(in_size, out_size, filter),
               "resample_plan: table smaller than 4 + 2 n + n * mirx_resample_taps()");
    resample_plan(in_size, out_size, first, n, filter, table);
    return MIRX_OK;
}

int mirx_resample_taps(int in_size, int out_size) { return mirx_resample_taps_filter(in_size, out_size, MIRX_RESAMPLE_BILINEAR); }

int mirx_resample_plan(int in_size, int out_size, int first, int n, int32_t *table, int64_t table_words) {
    return mirx_resample_plan_filter(in_size, out_size, first, n, MIRX_RESAMPLE_BILINEAR, table, table_words);
}

int mirx_resample_batch(const void *blob_host, const void *blob_dev, int64_t blob_bytes, int64_t b, int s, int out_kind,
                        const float *mean3, const float *std3, void *out, void *stream) {
    MIRX_CHECK(b >= 1 && b <= MIRX_RESAMPLE_MAX_BATCH, "resample: b must be in [1, 65536]");
    MIRX_CHECK(s >= 1 && s <= MIRX_RESAMPLE_MAX_OUT, "resample: s must be in [1, 1024]");
    MIRX_CHECK(out_kind == MIRX_RESAMPLE_OUT_U8 || out_kind == MIRX_RESAMPLE_OUT_F32, "resample: unknown output kind");
    MIRX_CHECK(blob_bytes >= 1 && blob_bytes <= MIRX_RESAMPLE_MAX_BYTES, "resample: buffer size outside [1, 2^40]");
    MIRX_CHECK(blob_host && blob_dev && out, "resample: null buffer");
    MIRX_CHECK(out_kind == MIRX_RESAMPLE_OUT_U8 || (mean3 && std3), "resample: the fp32 form needs mean and std");
    const size_t elem = out_kind == MIRX_RESAMPLE_OUT_F32 ? 4 : 1;
    MIRX_CHECK(aligned_to(blob_host, 8) && aligned_to(blob_dev, 16) && aligned_to(out, (s & 3) ? elem : 4 * elem),
               "resample: misaligned buffer (device buffer: 16 bytes; output: 4 elements when s % 4 == 0)");
    int64_t lds = 0;
    if (const char *msg = resample_check(blob_host, blob_bytes, b, s, &lds)) return fail(MIRX_EINVAL, msg);
    MIRX_HIP(launch_resample(blob_dev, b, s, out_kind == MIRX_RESAMPLE_OUT_F32, mean3, std3, out, lds, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

}  // extern "C"
