// mirx_index.hip -- the index half of the C ABI (include/mirx.h): the index object, its workspace and the search orchestration
// behind every mirx_index_* entry point.  (The stateless one-launch wrappers are in mirx_api.hip.)
//
// A search is a fixed sequence of launches on the caller's stream:
//   prep queries -> [group-max GEMM on a strided row sample -> thresholds] -> filter GEMM
//   -> finalize (sort candidates, completeness guard, fp64 re-rank, top-k)
//   -> exact scan (fp64 score tiles + row top-k) for the queries the guard rejected.
// The only host<->device synchronisation is one read of the rejected-query count.
// The six top-k entry points (mirx_index_search, _f64, _begin, _masked, _deep, _leave_out) each fill a SearchCall; search_call
// checks it, asks mirx_route.h which route answers and builds the one SearchRows the sequence runs over:
//   a mask           a SearchRows that stands for the allowed rows (neutralised in place, or gathered);
//   the deep route   k_eff past TIER1_MAX_K with SearchRows::deep set: gemm_plan_deep's candidate regions, its own threshold rank
//                    and k_finalize at DEEP_CAP;
//   leave-group-out  SearchRows::rcodes / qcodes set: k_finalize's CODES twins drop the candidates that carry the query's code,
//                    and the exact scan turns their scores into NaN.
// A range search (mirx_index_range_search) runs prep -> threshold from the radius -> filter GEMM -> its own finalize, the radix
// ranking for what that cannot answer, and a CSR assembly (k_range.hip).
// The radix ranking (radix_plan / radix_sort_batch) serves mirx_index_rank_all / _rank_top / _rank_top_masked and the range
// search's exact route; a mask reaches it as the allow bytes themselves.
// Every entry point that uses the workspace or moves rows starts with enter_idle: between mirx_index_search_begin and
// mirx_index_search_end it answers MIRX_ESTATE, because the pending search holds pointers into both.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "mirx_kernels.h"
#include "mirx_route.h"

using namespace mirx;

// What a search scans (built by search_call alone).  The index itself without a mask; under one, a stand-in for the allowed rows:
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
    bool deep = false;                    // tier 1 with the deep route's plan, threshold target and finalize (mirx_index_search_deep)
    // leave-group-out (mirx_index_search_leave_out): row r is not eligible for query i when qcodes[i] >= 0 and rcodes[r] == qcodes[i]
    const int32_t *rcodes = nullptr;      // one code per row of g32 (gathered with the rows where those are gathered), or null
    const int32_t *qcodes = nullptr;      // one code per query of the batch
    int64_t extra = 0;                    // rows a query may leave out (the caller's hint): sizes the sampled threshold only
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
    // workspace (each buffer frees itself with the index)
    DevBuf q32p, q16, qnorm, tau, cnt, cand, ovf_cnt, ovf, groupmax, fail_list, retry_list, tau2, q16r, taur,
        scores, stage, rankwork, spill, rkeys, rpay, rhist, idperm, creq, cpos, cpart, mallow, mbias, mids, mrows, mcodes,
        rstage, rcount, rxoff, rfirst, rexcl, rseg, rres, mwalk;
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

// (QUERY_BATCH, TIER1_MIN_ROWS and TIER1_MAX_K are defined in mirx_api.hip: the tests read them there)
constexpr size_t EXACT_WS_BYTES = (size_t)1 << 30;   // fp64 score tile workspace per pass
constexpr size_t COMPACT_SCRATCH_BYTES = (size_t)256 << 20;   // most a removal's chunk scratch takes by default

// The index's device stays selected until the entry point returns (declares the DeviceGuard `dg`).
#define MIRX_SELECT_DEVICE(ix, who)  \
    DeviceGuard dg((ix)->device);    \
    if (!dg.ok) return fail(MIRX_EHIP, std::string(who) + ": cannot select the index device")

// The first step of every entry point that uses the workspace or moves rows (searches, rankings, add, reserve, remove): a search
// that is begun holds GemmArgs / FinalizeArgs that point into both, so until mirx_index_search_end the index is busy.
// Drops a pending range result.
int enter_idle(mirx_index *ix, const char *who) {
    if (!ix) return fail(MIRX_EINVAL, std::string(who) + ": null index");
    if (ix->pend.active || ix->begun)
        return fail(MIRX_ESTATE, std::string(who) + ": a search begun with mirx_index_search_begin is still pending (call mirx_index_search_end)");
    ix->range_valid = false;
    return MIRX_OK;
}
#define MIRX_ENTER_IDLE(ix, who)                    \
    if (int rc_ = enter_idle(ix, who)) return rc_;  \
    MIRX_SELECT_DEVICE(ix, who)
// MIRX_CHECK for the bodies several entry points share: `who` (a C string) goes in front of the message.
#define MIRX_WHO_CHECK(who, cond, msg) MIRX_CHECK(cond, std::string(who) + ": " msg)

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

// q[0 .. n) as the padded fp32 rows, the bf16 rows and the norms of n_pad queries in ix->q32p / q16 / qnorm.
int prep_queries(mirx_index *ix, const float *q, int64_t n, int64_t n_pad, hipStream_t st) {
    MIRX_HIP(ix->q32p.ensure((size_t)n_pad * ix->dimp * sizeof(float)));
    MIRX_HIP(ix->q16.ensure((size_t)n_pad * ix->dimp * sizeof(uint16_t)));
    MIRX_HIP(ix->qnorm.ensure((size_t)n_pad * sizeof(float)));
    MIRX_HIP(launch_prep_queries(q, n, n_pad, ix->dim, ix->dimp, ix->q32p.as<float>(), ix->q16.as<uint16_t>(),
                                 ix->qnorm.as<float>(), st));
    return MIRX_OK;
}

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
        if (sr.rcodes)
            MIRX_HIP(launch_leave_out_scores(ix->scores.as<double>(), ld, sr.n, sr.rcodes, list_dev ? sr.qcodes : sr.qcodes + b, lst,
                                             cnt, st));
        MIRX_HIP(launch_row_topk(ix->scores.as<double>(), ld, sr.n, sr.ids, lst, cnt, exb, k,
                                 ix->metric, of, oi, ov, st));
    }
    return MIRX_OK;
}

// ---- the deep route (mirx_index_search_deep; where it is taken: mirx_route.h) ------------------------------------
// The constants the route decision reads.
RouteLimits route_limits() { return {TIER1_MIN_ROWS, TIER1_MAX_K, MAX_K, DEEP_TARGET_MUL, DEEP_TARGET_ADD, DEEP_GROUP_ROWS}; }

// The rank j whose group maximum leaves about target = deep_target(k_eff) (mirx_route.h) rows above it.  A fraction f of the groups
// has its maximum above tau when each of a group's G sampled rows passes with probability p, 1 - f = (1 - p)^G; the rows expected above tau are p * G * ngroups *
// stride = -ln(1 - f) * ngroups * stride for large G.  So f = 1 - exp(-target / (ngroups * stride)), at most one half.  (Speed
// only: the guard decides what is answered.)
int deep_sample_rank(int64_t k_eff, int ngroups, int64_t stride) {
    const double f = 1.0 - std::exp(-(double)deep_target(route_limits(), k_eff) / ((double)ngroups * (double)stride));
    const int64_t j = (int64_t)std::ceil(f * ngroups);
    return (int)std::max<int64_t>(1, std::min<int64_t>(j, ngroups / 2));
}

// The filter GEMM's workspace for a batch of nb_pad queries and the arguments every filter launch over the whole gallery shares
// (thresholds in ix->tau, which the caller fills; the counters are the caller's to zero).
int filter_args(mirx_index *ix, int64_t nb_pad, int bn, const float *bias_or_null, GemmArgs *out, bool deep = false) {
    int regions = 0, slots = 0;
    (deep ? gemm_plan_deep : gemm_plan)(ix->size, nb_pad, bn, &regions, &slots);
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
    {
        StageTimer t(ix, st, MIRX_STAGE_PREP);
        int rc = prep_queries(ix, qb, nb, nb_pad, st);
        if (rc) return rc;
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
        int rc = filter_args(ix, nb_pad, bn, sr.bias, &ga, sr.deep);
        if (rc) return rc;
    }
    const int regions = ga.regions;
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
        const int64_t k_eff = (int64_t)k + (exb ? 1 : 0) + sr.extra;
        const int64_t rank_k = std::min<int64_t>((4 * k_eff + stride - 1) / stride, ngroups / 2);
        rank_j = (int)std::max<int64_t>(rank_j, rank_k);
        if (sr.deep) rank_j = deep_sample_rank(k_eff, ngroups, stride);
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
    fa.lists = ga.lists();
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
    fa.row_codes = sr.rcodes;
    fa.query_codes = sr.qcodes;
    {
        StageTimer t(ix, st, MIRX_STAGE_FINALIZE);
        MIRX_HIP(launch_finalize(fa, sr.deep, st));
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
        const bool deep = ix->pend.rows.deep;
        (deep ? gemm_plan_deep : gemm_plan)(ix->size, nr_pad, bn2, &regions2, &slots2);
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
        f2.lists = g2.lists();
        f2.nq = nretry;
        f2.retry_list = nullptr;          // no third chance: what fails now goes to the exact scan
        f2.tau2 = nullptr;
        f2.qmap = ix->retry_list.as<int32_t>();
        {
            StageTimer t(ix, st, MIRX_STAGE_FINALIZE);
            MIRX_HIP(launch_finalize(f2, deep, st));
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

// A call's row mask on the device: a device pointer as it is, a host mask through ix->mallow (enqueued on st).
int device_allow(mirx_index *ix, const uint8_t *allow, hipStream_t st, const char *who, const uint8_t **out) {
    *out = allow;
    if (is_device_pointer(allow)) return MIRX_OK;
    if (ix->mallow.ensure((size_t)ix->size) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, std::string(who) + ": the mask does not fit the device");
    }
    MIRX_HIP(hipMemcpyAsync(ix->mallow.p, allow, (size_t)ix->size, hipMemcpyHostToDevice, st));
    *out = ix->mallow.as<uint8_t>();
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

// A batch of the radix ranking.  Per query: n fp64 scores (ix->scores, row stride ld), two key and two payload buffers (ix->rkeys,
// ix->rpay) = 32 bytes per row; `per` queries fill RANK_WS_BYTES (16 queries at 2^20 rows), and a gallery whose single query
// does not fit is bounded by the allocation alone.
struct RadixBatch {
    int64_t per, ld;
    const int32_t *perm;         // the rows in (id, row) order, or null while ids ascend with the row
    uint64_t *ka;                // [per, n] keys and payloads (rows); the sort's second buffers lie behind them
    int32_t *pa;
};

// Sizes the batch for `m` queries and ensures its workspace, the id permutation included.
int radix_plan(mirx_index *ix, int64_t m, const char *who, hipStream_t st, RadixBatch *out) {
    const int64_t n = ix->size;
    if (!ix->ids_ascend && !ix->idperm_valid) {
        int rc = build_id_permutation(ix, st);
        if (rc) return rc;
    }
    RadixBatch rb{};
    rb.perm = ix->ids_ascend ? nullptr : ix->idperm.as<int32_t>();
    rb.ld = round_up(n, 64);
    rb.per = std::max<int64_t>(1, std::min<int64_t>((int64_t)RANK_WS_BYTES / (rb.ld * 32), std::min<int64_t>(1024, m)));
    if (ix->scores.ensure((size_t)rb.per * rb.ld * sizeof(double)) != hipSuccess ||
        ix->rkeys.ensure((size_t)2 * rb.per * n * sizeof(uint64_t)) != hipSuccess ||
        ix->rpay.ensure((size_t)2 * rb.per * n * sizeof(int32_t)) != hipSuccess ||
        ix->rhist.ensure((size_t)rb.per * 256 * rank_sort_tiles(n) * sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, std::string(who) + ": the sort workspace (32 bytes per gallery row) does not fit the device");
    }
    rb.ka = ix->rkeys.as<uint64_t>();
    rb.pa = ix->rpay.as<int32_t>();
    *out = rb;
    return MIRX_OK;
}

// Scores, keys and the sort for cnt <= per prepared queries: those `list` (device) names out of q32p, or q32p's first cnt.  Leaves
// the scores in ix->scores and the rows of query i, best first, in rb.pa[i * n ..] under the ascending keys rb.ka[i * n ..];
// rows with allow[r] == 0 (and the excluded id, when it is dropped) sort behind every score.
int radix_sort_batch(mirx_index *ix, const RadixBatch &rb, const float *q32p, const int32_t *list, int cnt, const int64_t *exb,
                     bool drop_excluded, const uint8_t *allow, hipStream_t st) {
    const int64_t n = ix->size;
    MIRX_HIP(launch_scores_f64(q32p, list, cnt, ix->g32, n, ix->dimp, ix->metric, ix->scores.as<double>(), rb.ld, st));
    MIRX_HIP(launch_rank_sort_build(ix->scores.as<double>(), rb.ld, n, ix->ids, rb.perm, exb, drop_excluded ? 1 : 0, cnt, rb.ka,
                                    rb.pa, st));
    if (allow) MIRX_HIP(launch_mask_rank_keys(rb.ka, rb.pa, n, allow, cnt, st));
    MIRX_HIP(launch_rank_sort(rb.ka, rb.pa, rb.ka + rb.per * n, rb.pa + rb.per * n, ix->rhist.as<unsigned>(), n, cnt, st));
    return MIRX_OK;
}

// Ranks 0 .. kout-1 of every query by the radix sort.  allow (rank_top under a mask): the device allow bytes; the slots of
// masked rows read (-1, -inf).
int rank_radix(mirx_index *ix, const float *q, int64_t nq, int64_t kout, const int64_t *exclude, bool drop_excluded,
               int64_t *out_ids, float *out_val, double *out_f64, hipStream_t st, const uint8_t *allow = nullptr) {
    const int64_t n = ix->size;
    RadixBatch rb;
    int rc = radix_plan(ix, nq, "rank", st, &rb);
    if (rc) return rc;
    for (int64_t b = 0; b < nq; b += rb.per) {
        const int cnt = (int)std::min<int64_t>(rb.per, nq - b);
        const int64_t *exb = exclude ? exclude + b : nullptr;
        int64_t *oi = out_ids + b * kout;
        float *ov = out_val ? out_val + b * kout : nullptr;
        double *of = out_f64 ? out_f64 + b * kout : nullptr;
        if ((rc = prep_queries(ix, q + b * ix->dim, cnt, cnt, st))) return rc;
        if ((rc = radix_sort_batch(ix, rb, ix->q32p.as<float>(), nullptr, cnt, exb, drop_excluded, allow, st))) return rc;
        MIRX_HIP(launch_rank_sort_write(rb.pa, n, kout, ix->scores.as<double>(), rb.ld, ix->ids, exb, drop_excluded ? 1 : 0,
                                        ix->metric, cnt, oi, ov, of, st));
        if (allow) MIRX_HIP(launch_mask_rank_tail(rb.pa, n, kout, allow, cnt, oi, ov, of, st));
    }
    return MIRX_OK;
}

// The one pass over a masked search's allow bytes (k_mask.hip) and the scan of its keep flags (k_compact.hip): leaves the bias
// vector in ix->mbias (capacity floats), the masked ids in ix->mids, the scanned positions in ix->cpos (size + 1) and the number
// of allowed rows in *n_allowed.  Every buffer, with `gather_bytes` of ix->mrows for the caller's gather of the allowed rows, is
// allocated before the first kernel; one host wait, for the count.
int mask_prepare(mirx_index *ix, const uint8_t *allow, size_t gather_bytes, hipStream_t st, int64_t *n_allowed, const char *who) {
    const int64_t size = ix->size;
    const uint8_t *am = nullptr;
    int rc = device_allow(ix, allow, st, who, &am);
    if (rc) return rc;
    hipError_t e;
    if ((e = ix->mbias.ensure((size_t)ix->cap * sizeof(float))) != hipSuccess ||
        (e = ix->mids.ensure((size_t)size * sizeof(int64_t))) != hipSuccess ||
        (e = ix->mrows.ensure(gather_bytes)) != hipSuccess ||
        (e = ix->cpos.ensure((size_t)(size + 1) * sizeof(int32_t))) != hipSuccess ||
        (e = ix->cpart.ensure((size_t)compact_tiles(size) * sizeof(int32_t))) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, std::string(who) + ": " + hipGetErrorString(e));
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

// ---- the top-k search call ------------------------------------------------------------------------------------------------
// Every argument a top-k entry point can receive: each of the six fills one and hands it to search_call.
struct SearchCall {
    const char *who;                      // the entry point, in front of every message
    mirx_index *ix;
    const float *q;
    int64_t nq;
    int k;
    const int64_t *exclude;               // one id per query, or null
    float *out_val;                       // fp32 reported values and / or
    double *out_f64;                      //   fp64 ranking scores
    int64_t *out_ids;
    void *stream;
    bool wait_last = true;                // false: the last internal batch is left pending (mirx_index_search_begin); batch_back completes it
    bool allow_deep = false;              // the deep route is open to the call (mirx_index_search_deep / _leave_out)
    const uint8_t *allow = nullptr;       // the row mask, host or device, or null
    bool has_n_allow = false;             // the entry point takes the mask's length from its caller (mirx_index_search_masked):
    int64_t n_allow = 0;                  //   it must be the index's size
    bool leave_out = false;               // mirx_index_search_leave_out: codes, queries and outputs are required, even at nq == 0
    const int32_t *rcodes = nullptr;      // one code per index row
    const int32_t *qcodes = nullptr;      // one code per query
    int64_t max_left_out = 0;             // the caller's bound on the rows a query leaves out, -1 = unknown: picks the route only
};

// The one top-k search: checks the call, enters idle, counts the mask, asks mirx_route.h for the route, builds the SearchRows it
// names and runs the internal batches over it.
int search_call(const SearchCall &c) {
    MIRX_WHO_CHECK(c.who, c.k >= 1 && c.k <= MAX_K, "k must be in [1, 1024]");
    MIRX_WHO_CHECK(c.who, c.nq >= 0, "nq < 0");
    MIRX_WHO_CHECK(c.who, !c.leave_out || (c.rcodes && c.qcodes), "null codes");
    MIRX_WHO_CHECK(c.who, (c.nq == 0 && !c.leave_out) || (c.q && c.out_ids && (c.out_val || c.out_f64)), "null buffer");
    MIRX_WHO_CHECK(c.who, c.max_left_out >= -1, "max_left_out must be -1 (unknown) or a row count");
    mirx_index *ix = c.ix;
    MIRX_ENTER_IDLE(ix, c.who);
    if (c.has_n_allow) {
        MIRX_WHO_CHECK(c.who, c.n_allow == ix->size, "the mask needs one byte per row of the index (n_allow != size)");
        MIRX_WHO_CHECK(c.who, c.allow || c.n_allow == 0, "null mask");
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
    MIRX_HIP(hipMemsetAsync(ix->stats_dev, 0, sizeof(mirx_search_stats), st));
    ix->stats_host = mirx_search_stats{};
    ix->stats_host.nq = c.nq;
    ix->spans.clear();
    ix->ev_used = 0;
    if (c.nq == 0) return MIRX_OK;

    // ---- the route (an empty index has nothing to mask: the plain call, where every slot becomes (-1, -inf)) -------------------
    const int64_t size = ix->size;
    const bool masked = c.allow && size > 0;
    const RouteLimits lim = route_limits();
    RouteCall rc{};
    rc.tiers_auto = ix->tiers == MIRX_TIER_AUTO;
    rc.size = size;
    rc.k = c.k;
    rc.has_exclude = c.exclude != nullptr;
    rc.extra = std::max<int64_t>(c.max_left_out, 0);
    rc.allow_deep = c.allow_deep;
    rc.tile_groups = gemm_groups_per_tile(gemm_query_tile(std::min<int64_t>(c.nq, QUERY_BATCH)));   // the widest tile of the call's batches
    rc.row_bytes = (int64_t)ix->dimp * sizeof(float) + sizeof(int64_t);
    rc.gather_max = ix->mask_gather_bytes < 0 ? (int64_t)EXACT_WS_BYTES : ix->mask_gather_bytes;
    int64_t n_allowed = size;
    if (masked) {
        // one mask pass, one count; the gather's scratch is sized before the count is known
        const int64_t most_rows = route_most_rows(lim, rc);
        if (c.rcodes && ix->mcodes.ensure((size_t)most_rows * sizeof(int32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MIRX_ENOMEM, std::string(c.who) + ": the gathered codes do not fit the device");
        }
        int r = mask_prepare(ix, c.allow, (size_t)std::min(most_rows * rc.row_bytes, rc.gather_max), st, &n_allowed, c.who);
        if (r) return r;
    }
    const Route route = route_pick(lim, rc, masked, n_allowed);

    SearchRows sr;
    sr.tier1 = route.list != RouteList::EXACT;
    sr.deep = route.list == RouteList::DEEP;
    sr.rcodes = c.rcodes;                 // in row order: right wherever all rows are scanned
    sr.qcodes = c.qcodes;
    sr.extra = rc.extra;
    switch (route.rows) {
        case RouteRows::INDEX:
            sr.g32 = ix->g32;
            sr.ids = ix->ids;
            sr.n = size;
            break;
        case RouteRows::NEUTRALISED:
            // all rows, the masked ones neutralised: tier 1 by the bias, the exact scan by -inf scores and the masked ids
            sr.g32 = ix->g32;
            sr.ids = ix->mids.as<int64_t>();
            sr.n = size;
            sr.mpos = ix->cpos.as<int32_t>();
            sr.bias = sr.tier1 ? ix->mbias.as<float>() : nullptr;
            break;
        case RouteRows::GATHERED: {
            // few allowed rows: gather them (ascending, so ids keep their order) and scan only those; their codes go with them
            if ((size_t)(n_allowed * rc.row_bytes) > ix->mrows.bytes)
                return fail(MIRX_EHIP, std::string(c.who) + ": the gather scratch is smaller than the count needs");
            float *s32 = ix->mrows.as<float>();
            int64_t *sid = reinterpret_cast<int64_t *>(s32 + n_allowed * ix->dimp);
            MIRX_HIP(launch_compact_gather(ix->g32, ix->ids, ix->cpos.as<int32_t>(), size, ix->dimp, s32, sid, st));
            sr.g32 = s32;
            sr.ids = sid;
            sr.n = n_allowed;
            if (c.rcodes) {
                if ((size_t)n_allowed * sizeof(int32_t) > ix->mcodes.bytes)
                    return fail(MIRX_EHIP, std::string(c.who) + ": the code scratch is smaller than the count needs");
                MIRX_HIP(launch_mask_gather_codes(c.rcodes, ix->cpos.as<int32_t>(), size, ix->mcodes.as<int32_t>(), st));
                sr.rcodes = ix->mcodes.as<int32_t>();
            }
            break;
        }
        case RouteRows::NONE:             // nothing is allowed: n = 0, every slot reads (-1, -inf) and no row is scored
            break;
    }

    // ---- the internal batches -----------------------------------------------------------------------------------------------
    for (int64_t q0 = 0; q0 < c.nq; q0 += QUERY_BATCH) {
        if (c.qcodes) sr.qcodes = c.qcodes + q0;
        const int64_t nb = std::min<int64_t>(QUERY_BATCH, c.nq - q0);
        const float *qb = c.q + q0 * ix->dim;
        const int64_t *exb = c.exclude ? c.exclude + q0 : nullptr;
        float *ovb = c.out_val ? c.out_val + q0 * c.k : nullptr;
        int64_t *oib = c.out_ids + q0 * c.k;
        // fp64 ranking scores are always produced (user buffer or workspace)
        double *ofb;
        if (c.out_f64) {
            ofb = c.out_f64 + q0 * c.k;
        } else {
            MIRX_HIP(ix->stage.ensure((size_t)nb * c.k * sizeof(double)));
            ofb = ix->stage.as<double>();
        }
        int r = batch_front(ix, qb, nb, c.k, exb, ovb, ofb, oib, sr, st);
        if (r) return r;
        if (c.wait_last || q0 + QUERY_BATCH < c.nq) {
            r = batch_back(ix);
            if (r) return r;
        }
    }
    return MIRX_OK;
}

// mirx_index_rank_top and _rank_top_masked (masked: allow / n_allow are the caller's, and n_allow must be the index's size).
int rank_top_call(const char *who, mirx_index *ix, const float *q, int64_t nq, int64_t k, const int64_t *exclude, bool masked,
                  const uint8_t *allow, int64_t n_allow, float *out_val, double *out_f64, int64_t *out_ids, void *stream) {
    MIRX_WHO_CHECK(who, k >= 1, "k must be at least 1");
    MIRX_WHO_CHECK(who, nq >= 0, "nq < 0");
    MIRX_WHO_CHECK(who, out_ids, "out_ids is null");
    MIRX_WHO_CHECK(who, out_val || out_f64, "both score outputs are null");
    MIRX_ENTER_IDLE(ix, who);
    if (masked) {
        MIRX_WHO_CHECK(who, n_allow == ix->size, "the mask needs one byte per row of the index (n_allow != size)");
        MIRX_WHO_CHECK(who, allow || n_allow == 0, "null mask");
    }
    MIRX_WHO_CHECK(who, q || nq == 0, "null queries");
    MIRX_WHO_CHECK(who, k <= ix->size, "k is larger than the index");
    if (nq == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t *am = nullptr;          // (masked and past the checks: the index has rows, so the mask is not null)
    if (masked) {
        int rc = device_allow(ix, allow, st, who, &am);
        if (rc) return rc;
    }
    return rank_radix(ix, q, nq, k, exclude, /*drop_excluded=*/true, out_ids, out_val, out_f64, st, am);
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
    RadixBatch rb;
    int r = radix_plan(ix, m, "range_search", st, &rb);
    if (r) return r;
    if (ix->rfirst.ensure((size_t)rb.per * sizeof(int32_t)) != hipSuccess ||
        ix->rexcl.ensure((size_t)rb.per * sizeof(int64_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, "range_search: the cut's workspace does not fit the device");
    }
    int32_t *count = ix->rcount.as<int32_t>();
    int64_t *xoff = ix->rxoff.as<int64_t>();
    for (int64_t b = 0; b < m; b += rb.per) {
        const int cnt = (int)std::min<int64_t>(rb.per, m - b);
        const int32_t *lst = list_dev ? list_dev + b : nullptr;
        const float *qb = list_dev ? ix->q32p.as<float>() : ix->q32p.as<float>() + b * ix->dimp;
        const int64_t *exb = nullptr;
        if (rc.exclude && list_dev) {
            MIRX_HIP(launch_range_gather_exclude(rc.exclude, lst, cnt, ix->rexcl.as<int64_t>(), st));
            exb = ix->rexcl.as<int64_t>();
        } else if (rc.exclude) {
            exb = rc.exclude + b;
        }
        if ((r = radix_sort_batch(ix, rb, qb, lst, cnt, exb, /*drop_excluded=*/true, rc.allow, st))) return r;
        MIRX_HIP(launch_range_cut(rb.ka, n, cnt, rc.lo, rc.hi, lst, b, ix->rfirst.as<int32_t>(), count, st));
        MIRX_HIP(launch_range_scan(count, lst, b, cnt, rc.seg_total, xoff, nullptr, ix->range_total_dev, st));
        MIRX_HIP(hipMemcpyAsync(ix->range_total_host, ix->range_total_dev, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        MIRX_HIP(hipStreamSynchronize(st));
        const int64_t seg_total = ix->range_total_host[0];
        if (seg_total < rc.seg_total) return fail(MIRX_EHIP, "range_search: the scan returned an impossible count");
        if (rc.res_total + seg_total > range_limit(ix))
            return fail(MIRX_ENOMEM, "range_search: more hits than one call may return (MIRX_OPT_RANGE_MAX_HITS; default 2^28)");
        r = grow_keep(ix->rseg, (size_t)rc.seg_total * sizeof(Hit), (size_t)seg_total * sizeof(Hit), st, "range_search");
        if (r) return r;
        MIRX_HIP(launch_range_emit(rb.pa, n, ix->scores.as<double>(), rb.ld, ix->ids, cnt, lst, b, ix->rfirst.as<int32_t>(), count,
                                   xoff, ix->rseg.as<Hit>(), st));
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
    MIRX_HIP(ix->rcount.ensure((size_t)nb * sizeof(int32_t)));
    MIRX_HIP(ix->rxoff.ensure((size_t)nb * sizeof(int64_t)));
    {
        int r = prep_queries(ix, qb, nb, nb_pad, st);
        if (r) return r;
    }
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
        const int regions = ga.regions;
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
        fa.lists = ga.lists();
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
    DeviceGuard dg(ix->device);           // (nothing to report to: the frees go ahead whether or not the device could be selected)
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
    delete ix;                            // the workspace: every DevBuf releases itself, inside dg's scope
}

int mirx_index_reserve(mirx_index *ix, int64_t capacity_rows) {
    MIRX_CHECK(ix && capacity_rows >= 0, "index_reserve: bad argument");
    MIRX_ENTER_IDLE(ix, "index_reserve");
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
    MIRX_ENTER_IDLE(ix, "index_add");
    if (n == 0) return MIRX_OK;
    MIRX_CHECK(ix->size + n <= 0x7FFFFF00ll, "index_add: more than 2^31 rows per index");
    int rc = grow(ix, ix->size + n);
    if (rc) return rc;
    const bool rows_dev = is_device_pointer(rows), ids_dev = ids_or_null && is_device_pointer(ids_or_null);
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
    MIRX_ENTER_IDLE(ix, "remove_ids");
    if (out_removed_or_null) *out_removed_or_null = 0;
    if (n == 0 || ix->size == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t size = ix->size;
    const bool ids_dev = is_device_pointer(ids);
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

int mirx_index_get_rows(const mirx_index *ix, int64_t first, int64_t n, float *out_rows,
                        int64_t *out_ids_or_null) {
    MIRX_CHECK(ix && out_rows && first >= 0 && n >= 0 && first + n <= ix->size, "get_rows: bad range");
    MIRX_SELECT_DEVICE(ix, "get_rows");
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
    MIRX_SELECT_DEVICE(ix, "get_ids");
    MIRX_HIP(hipMemcpy(out_ids, ix->ids + first, (size_t)n * sizeof(int64_t), hipMemcpyDefault));
    return MIRX_OK;
}

// The top-k entry points: each fills a SearchCall (who, the index, queries, nq, k, exclude ids, the three outputs, the stream, then
// what only it has) for search_call.
int mirx_index_search(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                      float *out_scores, int64_t *out_ids, void *stream) {
    return search_call({"search", ix, q, nq, k, exclude_ids_or_null, out_scores, nullptr, out_ids, stream});
}

int mirx_index_search_f64(mirx_index *ix, const float *q, int64_t nq, int k,
                          const int64_t *exclude_ids_or_null, double *out_rank_scores, int64_t *out_ids,
                          void *stream) {
    return search_call({"search_f64", ix, q, nq, k, exclude_ids_or_null, nullptr, out_rank_scores, out_ids, stream});
}

int mirx_index_search_begin(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                            float *out_scores_or_null, double *out_rank_scores_or_null, int64_t *out_ids, void *stream) {
    SearchCall c{"search_begin", ix, q, nq, k, exclude_ids_or_null, out_scores_or_null, out_rank_scores_or_null, out_ids, stream};
    c.wait_last = false;
    const int rc = search_call(c);
    if (rc == MIRX_OK) ix->begun = true;
    return rc;
}

int mirx_index_search_masked(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                             const uint8_t *allow, int64_t n_allow, float *out_scores_or_null, double *out_rank_scores_or_null,
                             int64_t *out_ids, void *stream) {
    SearchCall c{"search_masked", ix, q, nq, k, exclude_ids_or_null, out_scores_or_null, out_rank_scores_or_null, out_ids, stream};
    c.allow = allow;
    c.has_n_allow = true;
    c.n_allow = n_allow;
    return search_call(c);
}

int mirx_index_search_deep(mirx_index *ix, const float *queries, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                           const uint8_t *allow_or_null, float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids,
                           void *stream) {
    SearchCall c{"search_deep", ix, queries, nq, k, exclude_ids_or_null, out_values_or_null, out_f64_or_null, out_ids, stream};
    c.allow_deep = true;
    c.allow = allow_or_null;
    return search_call(c);
}

int mirx_index_search_leave_out(mirx_index *ix, const float *queries, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                                const uint8_t *allow_or_null, const int32_t *row_codes, const int32_t *query_codes,
                                int64_t max_left_out, float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids,
                                void *stream) {
    SearchCall c{"search_leave_out", ix, queries, nq, k, exclude_ids_or_null, out_values_or_null, out_f64_or_null, out_ids, stream};
    c.allow_deep = true;
    c.allow = allow_or_null;
    c.leave_out = true;
    c.rcodes = row_codes;
    c.qcodes = query_codes;
    c.max_left_out = max_left_out;
    return search_call(c);
}

int mirx_tier1_max_k(void) { return TIER1_MAX_K; }

int64_t mirx_deep_min_rows(int k_eff, int64_t nq) {
    if (k_eff < 1 || nq < 1) return -1;
    return deep_min_rows(route_limits(), k_eff, gemm_groups_per_tile(gemm_query_tile(std::min<int64_t>(nq, QUERY_BATCH))));
}

int mirx_index_range_search(mirx_index *ix, const float *q, int64_t nq, double lo, double hi, const int64_t *exclude_ids_or_null,
                            const uint8_t *allow_or_null, int64_t n_allow, int64_t *out_lims, int64_t *out_total, void *stream) {
    MIRX_ENTER_IDLE(ix, "range_search");
    MIRX_CHECK(nq >= 0, "range_search: nq < 0");
    MIRX_CHECK(nq <= 0x7FFFFF00ll, "range_search: more than 2^31 queries in one call");
    MIRX_CHECK(!(lo != lo) && !(hi != hi), "range_search: a bound is NaN");
    MIRX_CHECK(out_lims && out_total, "range_search: null output");
    MIRX_CHECK(q || nq == 0, "range_search: null queries");
    MIRX_CHECK(allow_or_null ? n_allow == ix->size : n_allow == 0,
               "range_search: the mask needs one byte per row of the index (n_allow != size)");
    *out_total = 0;
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
    RangeCall rc{};
    rc.lo = lo;
    rc.hi = hi;
    if (allow_or_null) {
        int r = device_allow(ix, allow_or_null, st, "range_search", &rc.allow);
        if (r) return r;
    }
    const bool filter = ix->tiers == MIRX_TIER_AUTO && ix->size >= TIER1_MIN_ROWS && lo > -INFINITY;
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
    MIRX_SELECT_DEVICE(ix, "range_fetch");
    MIRX_HIP(launch_range_fetch(ix->rres.as<Hit>(), ix->range_total, ix->metric, out_values_or_null, out_f64_or_null, out_ids,
                                reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_index_range_last_stats(mirx_index *ix, mirx_range_stats *out) {
    MIRX_CHECK(ix && out, "range_last_stats: null argument");
    *out = ix->range_stats;
    if (!ix->range_stats_dev) return MIRX_OK;
    MIRX_SELECT_DEVICE(ix, "range_last_stats");
    unsigned long long d[2] = {0, 0};
    MIRX_HIP(hipDeviceSynchronize());
    MIRX_HIP(hipMemcpy(d, ix->range_stats_dev, sizeof(d), hipMemcpyDeviceToHost));
    out->filter_answered = (int64_t)d[0];
    out->candidates = (int64_t)d[1];
    return MIRX_OK;
}

int mirx_index_search_end(mirx_index *ix) {
    MIRX_CHECK(ix, "search_end: null index");
    MIRX_SELECT_DEVICE(ix, "search_end");
    ix->begun = false;
    return batch_back(ix);
}

int mirx_index_last_stats(mirx_index *ix, void *stream, mirx_search_stats *out) {
    MIRX_CHECK(ix && out, "last_stats: null argument");
    MIRX_SELECT_DEVICE(ix, "last_stats");
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
    MIRX_SELECT_DEVICE(ix, "last_timings");
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
    MIRX_ENTER_IDLE(ix, "rank_all");
    if (nq == 0 || ix->size == 0) return MIRX_OK;
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
    for (int64_t b = 0; b < nq; b += per) {
        const int cnt = (int)std::min<int64_t>(per, nq - b);
        if (int rc = prep_queries(ix, q + b * ix->dim, cnt, cnt, st)) return rc;
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
    return rank_top_call("rank_top", ix, q, nq, k, exclude_ids_or_null, /*masked=*/false, nullptr, 0, out_scores_or_null,
                         out_rank_scores_or_null, out_ids, stream);
}

int mirx_index_rank_top_masked(mirx_index *ix, const float *q, int64_t nq, int64_t k, const int64_t *exclude_ids_or_null,
                               const uint8_t *allow, int64_t n_allow, float *out_scores_or_null,
                               double *out_rank_scores_or_null, int64_t *out_ids, void *stream) {
    return rank_top_call("rank_top_masked", ix, q, nq, k, exclude_ids_or_null, /*masked=*/true, allow, n_allow, out_scores_or_null,
                         out_rank_scores_or_null, out_ids, stream);
}

int mirx_index_rank_metrics(mirx_index *ix, const float *q, int64_t nq, const int64_t *exclude_ids_or_null, int self_kind,
                            const int64_t *row_labels, const int64_t *query_labels, const int32_t *row_codes_or_null,
                            const int32_t *query_codes_or_null, int rel_kind, double jaccard_threshold, int ap_kind,
                            const int32_t *kappas, int nk, double *out_ap, int64_t *out_cnt, int64_t *out_nrel, int64_t *out_maxpos,
                            void *stream) {
    MIRX_CHECK(nq >= 0, "rank_metrics: nq < 0");
    MIRX_CHECK(self_kind >= 0 && self_kind <= 2, "rank_metrics: self_kind must be 0, 1 or 2");
    MIRX_CHECK(self_kind == 0 || exclude_ids_or_null, "rank_metrics: self_kind 1 and 2 need exclude_ids");
    MIRX_CHECK((row_codes_or_null == nullptr) == (query_codes_or_null == nullptr),
               "rank_metrics: row_codes and query_codes go together (both or neither)");
    MIRX_CHECK(nk >= 0 && nk <= MIRX_MAX_KAPPAS && (nk == 0 || (kappas && out_cnt)), "rank_metrics: 0 <= nk <= 8");
    MIRX_CHECK((rel_kind == 0 || rel_kind == 1) && (ap_kind == 0 || ap_kind == 1), "rank_metrics: bad kind");
    MIRX_CHECK(nq == 0 || (q && query_labels && out_ap && out_nrel && out_maxpos), "rank_metrics: null buffer");
    RankWalkArgs a{};
    for (int j = 0; j < nk; ++j) {
        MIRX_CHECK(kappas[j] >= 1, "rank_metrics: kappa must be >= 1");
        a.kappas[j] = kappas[j];
    }
    MIRX_CHECK(ix, "rank_metrics: null index");
    MIRX_ENTER_IDLE(ix, "rank_metrics");
    MIRX_CHECK(nq == 0 || ix->size == 0 || row_labels, "rank_metrics: null row_labels");
    if (nq == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n = ix->size;
    RadixBatch rb{};
    rb.per = std::min<int64_t>(1024, nq);
    if (n > 0) {
        int rc = radix_plan(ix, nq, "rank_metrics", st, &rb);
        if (rc) return rc;
    }
    if (ix->mwalk.ensure(std::max<size_t>(256, rank_walk_workspace_bytes(rb.per, n))) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MIRX_ENOMEM, "rank_metrics: the walk's partials do not fit the device");
    }
    a.n = n; a.ids = ix->ids; a.self_kind = self_kind; a.row_labels = row_labels; a.row_codes = row_codes_or_null;
    a.jaccard_threshold = jaccard_threshold; a.nk = nk; a.pay = rb.pa;
    rank_walk_carve(a, ix->mwalk.p, rb.per);
    for (int64_t b = 0; b < nq; b += rb.per) {
        const int cnt = (int)std::min<int64_t>(rb.per, nq - b);
        const int64_t *exb = exclude_ids_or_null ? exclude_ids_or_null + b : nullptr;
        if (n > 0) {
            int rc = prep_queries(ix, q + b * ix->dim, cnt, cnt, st);
            if (rc) return rc;
            // rank_all's order: the excluded row keeps its place behind every score
            if ((rc = radix_sort_batch(ix, rb, ix->q32p.as<float>(), nullptr, cnt, exb, /*drop_excluded=*/false, nullptr, st))) return rc;
        }
        a.nq = cnt; a.exclude = exb; a.query_labels = query_labels + b;
        a.query_codes = query_codes_or_null ? query_codes_or_null + b : nullptr;
        a.out_ap = out_ap + b; a.out_cnt = reinterpret_cast<unsigned long long *>(out_cnt) + b * nk;
        a.out_nrel = out_nrel + b; a.out_maxpos = out_maxpos + b;
        MIRX_HIP(launch_rank_walk(a, rel_kind, ap_kind, st));
    }
    return MIRX_OK;
}

int mirx_index_group_fill(mirx_index *ix, const float *q, int64_t nq, const int64_t *exclude_ids_or_null, int limit, int group_size,
                          const int64_t *pair_query, const int64_t *pair_slot, const int64_t *pair_first, const int64_t *pair_len,
                          int64_t n_pairs, const int64_t *members, int64_t n_members, int max_members, int64_t *out_ids,
                          double *out_rank_scores, void *stream) {
    MIRX_ENTER_IDLE(ix, "group_fill");
    if (const char *why = group_limits(limit, group_size)) return fail(MIRX_EINVAL, std::string("group_fill: ") + why);
    MIRX_CHECK(nq >= 0 && nq <= 0x7FFFFF00ll && n_pairs >= 0 && n_pairs <= 0x7FFFFFFFll && n_members >= 0, "group_fill: bad sizes");
    MIRX_CHECK(max_members >= 1 && max_members <= MIRX_GROUP_FILL_MAX, "group_fill: max_members must be in [1, 4096]");
    MIRX_CHECK(n_pairs == 0 || (q && pair_query && pair_slot && pair_first && pair_len && members && out_ids && out_rank_scores),
               "group_fill: null buffer");
    if (n_pairs == 0 || nq == 0) return MIRX_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (int rc = prep_queries(ix, q, nq, nq, st)) return rc;
    GroupFillArgs a{};
    a.q32p = ix->q32p.as<float>(); a.g32 = ix->g32; a.ids = ix->ids; a.exclude = exclude_ids_or_null;
    a.nq = nq; a.n_rows = ix->size; a.dimp = ix->dimp; a.limit = limit; a.group_size = group_size;
    a.pair_query = pair_query; a.pair_slot = pair_slot; a.pair_first = pair_first; a.pair_len = pair_len; a.n_pairs = n_pairs;
    a.members = members; a.n_members = n_members; a.max_members = max_members;
    a.out_ids = out_ids; a.out_f64 = out_rank_scores;
    MIRX_HIP(launch_group_fill(a, ix->metric, st));
    return MIRX_OK;
}

}  // extern "C"
