/*
 * mirx.h -- C ABI of libmirx.so: MI355X-native exhaustive retrieval + embedding-head kernels.
 *
 * This is the drop-in boundary underneath the reference's Python protocol.  The reference
 * (100 % Python, /root/reference) has no FFI of its own; each entry point below names the
 * reference call it stands in for, and INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference adds at that call site.
 *
 * Conventions
 *   - plain C types only; every pointer is a raw address, no torch/HIP C++ types;
 *   - return 0 on success, a negative MIRX_E* code on failure; mirx_last_error() gives the
 *     text for the calling thread; nothing throws across the ABI;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work of a
 *     call is enqueued on it and the call returns without waiting unless stated;
 *   - "device pointer" = memory of the index's device (hipMalloc / torch.cuda tensor
 *     data_ptr()); "host pointer" = ordinary host memory.  mirx_index_add accepts either
 *     (it asks the runtime); search inputs/outputs must be device pointers;
 *   - the caller owns every buffer it passes; the index owns its device copies;
 *   - an index is not re-entrant: add / search / destroy on one index must not overlap.
 *
 * Semantics of a search (pinned by oracle/search_ref.c):
 *   score   = fp64 accumulation of the fp32 inputs in the fixed "lane tree" order
 *   ranking = higher score first; equal scores -> lower id first
 *   metric MIRX_METRIC_IP      score = <q, g>               (cosine on unit rows)
 *   metric MIRX_METRIC_NEG_L2  ranks by -||q-g||^2, reports -||q-g||_2
 * The bf16 MFMA pass only proposes candidates; every returned hit is re-scored in fp64 and
 * a completeness guard proves that no better row was left out (otherwise the query falls
 * through to the exact scan), so results never depend on which tier answered.
 */
#ifndef MIRX_H
#define MIRX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRX_VERSION 305

#define MIRX_OK 0
#define MIRX_EINVAL (-1)   /* bad argument (null pointer, dim mismatch, k out of range) */
#define MIRX_ENOMEM (-2)   /* device or host allocation failed */
#define MIRX_EHIP (-3)     /* a HIP runtime call failed; text in mirx_last_error() */
#define MIRX_ESTATE (-4)   /* call not valid in the index's current state */

#define MIRX_METRIC_IP 0
#define MIRX_METRIC_NEG_L2 1

/* search-tier selection (mirx_index_set_option MIRX_OPT_TIERS) */
#define MIRX_TIER_AUTO 0        /* bf16 MFMA candidates + guard, exact scan for the rest   */
#define MIRX_TIER_EXACT_ONLY 3  /* fp64 exact scan for every query (small galleries, tests) */

#define MIRX_OPT_TIERS 1
#define MIRX_OPT_SAMPLE_RANK 2   /* j: threshold = j-th largest sampled group maximum (default 8; deeper where 4 (k + 1 excluded id) candidates need it) */
#define MIRX_OPT_FORCE_TAU 3     /* test hook: float bits of a fixed threshold; 0x7fc00000 = off  */
#define MIRX_OPT_PROFILE 4       /* 1: record HIP events around every stage of a search           */
#define MIRX_OPT_RANK_SORT 5     /* which sort mirx_index_rank_all runs: MIRX_RANK_SORT_*          */
#define MIRX_OPT_COMPACT_CHUNK_ROWS 6   /* test hook: rows per compaction chunk of mirx_index_remove_ids; 0 = default */
#define MIRX_OPT_MASK_GATHER_BYTES 7    /* test hook: most scratch a masked search gathers its allowed rows into; -1 = default (1 GiB) */
#define MIRX_OPT_RANGE_MAX_HITS 8       /* test hook: most hits one mirx_index_range_search call may return; 0 = default (2^28) */

/* values of MIRX_OPT_RANK_SORT.  Both sorts return the same ranking; forcing one lets a test run either on any gallery. */
#define MIRX_RANK_SORT_AUTO 0     /* bitonic network up to 65536 rows, radix sort above            */
#define MIRX_RANK_SORT_BITONIC 1  /* always the bitonic network: more than 65536 rows is MIRX_EINVAL */
#define MIRX_RANK_SORT_RADIX 2    /* always the segmented radix sort (any size >= 1)               */

/* stages timed when MIRX_OPT_PROFILE is on (mirx_index_last_timings) */
#define MIRX_STAGE_PREP 0        /* query conversion                                  */
#define MIRX_STAGE_SAMPLE 1      /* group-max GEMM on the row sample + threshold pick */
#define MIRX_STAGE_GEMM 2        /* the filter GEMM over the whole gallery            */
#define MIRX_STAGE_FINALIZE 3    /* candidate sort, guard, fp64 re-rank               */
#define MIRX_STAGE_EXACT 4       /* exact scan of rejected / routed queries           */
#define MIRX_NUM_STAGES 5

typedef struct mirx_index mirx_index;

/* Counters of the most recent search on an index (host-visible after the stream is idle). */
typedef struct mirx_search_stats {
    int64_t nq;               /* queries in the call                                        */
    int64_t tier1_answered;   /* answered by the bf16 MFMA pass + fp64 re-rank              */
    int64_t exact_answered;   /* fell through to (or were routed to) the fp64 exact scan    */
    int64_t candidates;       /* rows that passed the threshold, summed over queries        */
    int64_t reranked;         /* rows re-scored in fp64 by tier 1, summed over queries      */
    int64_t overflowed;       /* queries whose candidate list overflowed its capacity       */
    int64_t incomplete;       /* queries whose completeness guard failed                    */
    int64_t left_out;         /* candidates dropped by mirx_index_search_leave_out's predicate on the filter routes,
                                 summed over the queries those routes answered              */
} mirx_search_stats;

const char *mirx_last_error(void);
int mirx_version(void);

/*
 * Process-wide kernel-selection knobs.  They choose between kernels that return the SAME bits, so they change speed only
 * (the tests use them to run both kernels of a pair on one input).  No reference analogue: the reference leaves such
 * choices to cuDNN / MIOpen heuristics behind model(x) (model.py:71-84).
 *   MIRX_TUNE_CONV1X1_SMALL_MAX_WG  a 1x1 convolution of fewer than this many 128-channel x 128-pixel workgroups runs as
 *                                   one wave per 32 x 32 tile (small batches: test.py:1513 B = 64, milvus_retrieval.py:53-66
 *                                   B = 1); 0 = never.  Default 128.
 *   MIRX_TUNE_CONV3X3_SMALL_MAX_WG  the same for the dense layer's 3x3 convolution: fewer strip workgroups than this ->
 *                                   one wave per 32 output pixels; 0 = never.  Default 96.
 *   MIRX_TUNE_CONV1X1_RING          1: a large 1x1 convolution runs on the LDS-DMA ring arm of its kernel where that arm
 *                                   applies; 0: always on the register-staged tiled arm.  Default 1.
 */
#define MIRX_TUNE_CONV1X1_SMALL_MAX_WG 1
#define MIRX_TUNE_CONV3X3_SMALL_MAX_WG 2
#define MIRX_TUNE_CONV1X1_RING 3
int mirx_set_tuning(int key, int64_t value);

/*
 * Index lifetime.  Replaces: Collection(name, schema) + create_index + load
 * (milvus/milvus_setup.py:139-222) -- an in-process, device-resident flat index.
 * `dim` is the embedding width (any value >= 1; rows are stored padded to 64).
 */
int mirx_index_create(int dim, int metric, int device, mirx_index **out);
void mirx_index_destroy(mirx_index *ix);

/*
 * Append n rows.  Replaces collection.insert([paths, labels, embeddings.tolist()])
 * (ingest_embeddings.py:399-411) for the embedding column; path/label metadata stay with the
 * Python Retriever.  rows: row-major [n, dim] fp32, host or device.  ids: n int64 (host or
 * device) or NULL for auto ids (previous size + i, Milvus auto_id analogue,
 * milvus_setup.py:170).  Synchronous: returns when the rows are resident.
 * mirx_index_add and mirx_index_reserve (room for capacity_rows rows ahead of the adds) may move the rows to a larger
 * allocation.  Between mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.
 */
int mirx_index_add(mirx_index *ix, const float *rows, int64_t n, const int64_t *ids_or_null);
int mirx_index_reserve(mirx_index *ix, int64_t capacity_rows);
int64_t mirx_index_size(const mirx_index *ix);
int mirx_index_dim(const mirx_index *ix);
int mirx_index_set_option(mirx_index *ix, int option, int64_t value);

/* Copy rows [first, first+n) of the fp32 master back out (device or host destination). */
int mirx_index_get_rows(const mirx_index *ix, int64_t first, int64_t n, float *out_rows,
                        int64_t *out_ids_or_null);

/*
 * Remove every row whose id occurs in ids[0 .. n) (host or device pointer).  Replaces collection.delete(expr="id in [..]")
 * of pymilvus, the counterpart of the reference's collection.insert (ingest_embeddings.py:399-411) that the reference itself
 * only reaches through drop_old (milvus_setup.py:150-158): one wrong or leaked image no longer costs a re-embedding of the
 * gallery.  Duplicates in the request count once, ids that are not in the index are ignored, and when a user id repeats in
 * the index all its rows go.  The survivors keep their order in every buffer, rows from the new size up to the capacity read
 * as zeros again and the capacity stays, so mirx_index_search / _search_f64 / _rank_top / _rank_all afterwards return exactly
 * the ids and fp64 scores of a fresh index built from the survivors in order (stats may differ: the bound on the rows' norms
 * is kept, it is still an upper bound).  Auto ids of later mirx_index_add calls go on past the largest auto id handed out so
 * far: a removed row's id is not used again.
 *   out_removed_or_null  host: the number of rows removed
 * Work: the request is sorted on the device (the ranking's radix sort), then a binary search of each row's id in it, an
 * exclusive scan of the keep flags (three launches) and 16-byte row moves, chunk by chunk through a scratch of at most 256 MiB (MIRX_OPT_COMPACT_CHUNK_ROWS sets the chunk's rows
 * for tests); no atomics, workgroups synchronise at launch boundaries only, two calls on equal indexes leave equal buffers.
 * Synchronous: enqueued on `stream`, returns when the index is compact.  Every allocation happens before the first row moves:
 * MIRX_ENOMEM leaves the index untouched.  Between mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.
 * mirx_compact_tile: rows per workgroup of the scan (the sizes around its multiples are the scan's edges); no device touched.
 */
int mirx_index_remove_ids(mirx_index *ix, const int64_t *ids, int64_t n, int64_t *out_removed_or_null, void *stream);
int mirx_compact_tile(void);

/*
 * Exhaustive top-k.  Replaces collection.search(data=[q], anns_field="embedding", limit=k)
 * (milvus/milvus_retrieval.py:80-86, nih_zilliz_utils.py:263-270) and the brute force
 * `-torch.cdist` / `e @ e.t()` + fill_diagonal_(-inf) + topk of test.py:1080-1085,44.
 *   q            device, [nq, dim] fp32 row-major
 *   exclude_ids  device, nq int64 or NULL: gallery rows with this id are skipped for query i
 *                (the -inf diagonal of test.py:1081); use -1 for "nothing"
 *   out_scores   device, [nq, k] fp32: reported value (metric 0: dot; metric 1: -L2)
 *   out_ids      device, [nq, k] int64; slots past the number of eligible rows: id -1, -inf
 *   1 <= k <= 1024
 */
int mirx_index_search(mirx_index *ix, const float *q, int64_t nq, int k,
                      const int64_t *exclude_ids_or_null, float *out_scores, int64_t *out_ids,
                      void *stream);

/* fp64 ranking scores of the same hits ([nq, k] device doubles) for bit-exact parity tests. */
int mirx_index_search_f64(mirx_index *ix, const float *q, int64_t nq, int k,
                          const int64_t *exclude_ids_or_null, double *out_rank_scores,
                          int64_t *out_ids, void *stream);

/*
 * The same search in two calls, so that the host does not block while the first pass runs (the caller may enqueue the next
 * embed micro-batch, on this or another stream, between them):
 *   mirx_index_search_begin  enqueues query preparation, threshold sampling, the filter GEMM and finalize on `stream` and
 *       returns; the two counters that say whether any query needs the second-chance filter or the exact scan travel to
 *       pinned host memory behind an event.  Either output form may be NULL (not both).
 *   mirx_index_search_end    waits for that event (a host wait; the stream is not drained), runs the rare follow-up passes
 *       the counters ask for on the same stream, and returns.  The outputs are complete when work enqueued on the stream
 *       up to this call has finished; stats / timings refer to this search.
 * Between the two calls the index is busy and the query / output buffers must stay valid: the pending search holds pointers
 * into the index's workspace and rows, so every call that uses the workspace or moves rows -- mirx_index_search, _search_f64,
 * _search_begin, _search_masked, _search_deep, _search_leave_out, _range_search, _rank_all, _rank_top, _rank_top_masked, _group_fill, _add, _reserve,
 * _remove_ids -- returns MIRX_ESTATE and changes nothing.  mirx_index_search_end, _range_fetch, _range_last_stats, _last_stats,
 * _last_timings, _get_rows, _get_ids, _size, _dim and _set_option stay callable.
 * mirx_index_search == begin + end.  (No reference counterpart: MilvusRetriever.search is a blocking RPC,
 * milvus/milvus_retrieval.py:80-86.)
 */
int mirx_index_search_begin(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                            float *out_scores_or_null, double *out_rank_scores_or_null, int64_t *out_ids, void *stream);
int mirx_index_search_end(mirx_index *ix);

/*
 * The search under a row mask: pymilvus' collection.search(..., expr=...) once the expression has been evaluated per row.
 *   allow    n_allow bytes, one per row of the index in row order, non-zero = eligible; a host or a device pointer (as the ids
 *            of mirx_index_remove_ids).  n_allow != mirx_index_size: MIRX_EINVAL.
 * The other arguments are those of mirx_index_search_begin (either score output may be NULL, not both).  The mask is an argument,
 * not index state: nothing of it outlives the call.  Between mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.
 * Result: exactly what mirx_index_search / _search_f64 return on a fresh index that holds only the allowed rows, in order, with
 * their ids -- ids, fp64 rank scores and reported fp32 values bit for bit, ties by lowest id, the excluded id skipped; slots
 * past the number of eligible rows read (-1, -inf); a masked row's id appears in no output.  A mask of all ones is the unmasked
 * call (it is handed over to it), a mask of all zeros fills every slot with (-1, -inf) and scores nothing.
 * Work: one pass over the mask (counts the allowed rows, writes a per-row fp32 bias for every row up to the capacity, the keep
 * flags and the masked ids) and the removal's scan of the flags, then one host wait for the count, which picks the route:
 *   - at least 32768 allowed rows, k (+1 with exclude ids) <= 64, tiers on auto: the tier-1 sequence of the plain search with
 *     that bias in the sample and the filter GEMM (-inf on a masked row: it passes no threshold, so it is never a candidate);
 *     the queries the completeness guard rejects are scanned exactly over all rows with the masked entries neutralised;
 *   - otherwise the exact scan over the allowed rows alone, gathered (fp32 rows and ids, ascending) into a scratch of at most
 *     1 GiB; allowed rows that do not fit it are scanned in place with the masked entries neutralised instead, at the cost of
 *     the unmasked exact tier (MIRX_OPT_MASK_GATHER_BYTES lowers the limit for tests).
 * Workspace besides the plain search's: 16 bytes per row (bias, positions, masked ids), the mask itself when it comes from the
 * host, and the gather scratch.  All of it is allocated before the first launch; the gather scratch, whose need only the count
 * tells, at its upper bound: the rows of 32767 allowed rows when the filter route is open to the call, else of the whole index,
 * and never more than the 1 GiB limit.  The plain search's own workspace is allocated where the plain search allocates it, batch
 * by batch, after the mask pass: a MIRX_ENOMEM there leaves outputs of earlier batches written, as in mirx_index_search.  No
 * floating-point atomics; the result does not depend on scheduling.  mirx_index_last_stats / _last_timings describe the masked call (the mask
 * pass itself is not among the timed stages).
 */
int mirx_index_search_masked(mirx_index *ix, const float *q, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                             const uint8_t *allow, int64_t n_allow, float *out_scores_or_null,
                             double *out_rank_scores_or_null, int64_t *out_ids, void *stream);

/*
 * The search for 64 < k (+1 with exclude ids) <= 1024 on the filter GEMM ("deep route"): Milvus' collection.search(limit=100),
 * recall@100-style evaluation, the per-request lists of a hybrid search.  mirx_index_search answers such a k by scoring every row.
 *   queries, nq, k, exclude_ids, stream    as for mirx_index_search; 1 <= k <= 1024, else MIRX_EINVAL
 *   allow            NULL, or one byte per row of the index (host or device, non-zero = eligible): mirx_index_search_masked's mask
 *   out_values / out_f64 / out_ids          fp32 reported values and / or fp64 ranking scores (either may be NULL, not both), ids
 * Result: exactly what mirx_index_search / _search_f64 / _search_masked return for the same arguments -- ids, fp64 scores and
 * fp32 values bit for bit, (score desc, id asc), the excluded id skipped, (-1, -inf) in the slots past the eligible rows.
 * A null index, null queries or null ids: MIRX_EINVAL before any device call.  Between mirx_index_search_begin and
 * mirx_index_search_end: MIRX_ESTATE.
 * Route, decided on the host: the deep route answers when the tiers are on auto, k_eff = k (+1 with exclude ids) > 64 and the
 * rows that can rank (the index's, or the mask's allowed rows) number at least mirx_deep_min_rows(k_eff, nq) =
 * max(32768, (2 k_eff + 512) * 512 / g), g = 8 / 4 / 2 threshold groups per gallery tile at up to 64 / 128 / more queries: below
 * that the sampled threshold cannot resolve the 2 k_eff + 512 candidates per query the route aims at.  Every other call is handed
 * to mirx_index_search / _search_masked unchanged (result, stats and stage timings are theirs).
 * The deep route is the tier-1 sequence with its own capacities: candidate regions of about 8192 slots per query, a per-query
 * finalize (k_finalize_deep.hip) that sorts up to 4096 candidates, applies the same completeness guard (tau < kth - 2 eps),
 * re-scores the guard band in fp64 and writes k results; guard-rejected queries are filtered once more with the threshold the
 * guard derived, and what still fails -- more than 4096 candidates, fewer than k_eff -- is scanned exactly.  No result comes
 * from an approximate score.  mirx_index_last_stats: tier1_answered = queries the deep filter answered, exact_answered = the
 * rest; candidates / reranked / overflowed / incomplete as for mirx_index_search.  Workspace at 8192 queries: 512 MiB of
 * candidate regions (64 MiB for mirx_index_search), allocated on the first deep call and kept.
 * mirx_tier1_max_k: the 64 above.  mirx_deep_min_rows: the bound (-1 for k_eff < 1 or nq < 1); neither touches a device.
 */
int mirx_index_search_deep(mirx_index *ix, const float *queries, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                           const uint8_t *allow_or_null, float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids,
                           void *stream);
int mirx_tier1_max_k(void);
int64_t mirx_deep_min_rows(int k_eff, int64_t nq);

/*
 * Leave-group-out search: the top k of the rows that do NOT share the query's key.  Replaces the host-side filters
 * `r.image_path != query.image_path` of fusion_eval/metrics.py:65 and retrieval_analysis/milvus_adapter.py:204-207 (every row
 * whose field value equals the query's is dropped, not only the query's own row), which pymilvus cannot express for a batch:
 * one `expr` serves all its queries.  Patient-wise evaluation of NIH ChestX-ray14 / VinDr / COVIDx galleries is the use.
 *   row_codes    device, [mirx_index_size] int32, one code per row in row order (as an allow mask); a negative code is the
 *                field's null and is never left out
 *   query_codes  device, [nq] int32; a negative code leaves nothing out for that query
 *   max_left_out a speed hint only: an upper bound on the rows any query of the call leaves out, or -1 = unknown (routes as 0)
 *   queries, nq, k, exclude_ids, allow, the three outputs, stream: as for mirx_index_search_deep; 1 <= k <= 1024
 * Row r is eligible for query i  <=>  r is live, allow[r] != 0 (when a mask is given), id[r] != exclude_ids[i] (when given)
 * and !(query_codes[i] >= 0 && row_codes[r] == query_codes[i]).
 * Result: the top k of the eligible rows, (score desc, id asc), (-1, -inf) in the slots past them -- ids, fp64 ranking scores
 * and fp32 values bit for bit what mirx_index_search_masked returns for that one query under allow[r] = (row_codes[r] !=
 * query_codes[i]) ANDed with the caller's mask, hence what a fresh index of the eligible rows returns.
 * A null index, queries, ids, row_codes or query_codes, both score outputs null, or k out of range: MIRX_EINVAL before any
 * device call.  Between mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.
 * Route, decided on the host as if k_eff were k (+1 with exclude ids) + max_left_out: the candidate lists of
 * mirx_index_search while that is <= mirx_tier1_max_k(); the deep route while k + max_left_out <= 1024 and the rows that can rank number
 * at least mirx_deep_min_rows of it; else the exact scan.  The sampled threshold is sized for that count.  The hint never
 * changes the answer: on the filter routes the finalize kernel drops a candidate that shares the query's code BEFORE the
 * completeness guard counts the list (it asks for k_eff eligible candidates and takes the k_eff-th eligible score), so a
 * hint that is too small only sends more queries to the retry pass or the exact scan.  The exact scan turns the left-out
 * entries of its fp64 score tile into NaN, which ranks before nothing, not even an empty slot.  Under a mask the routes are
 * those of mirx_index_search_masked; where the allowed rows are gathered their codes are gathered with them.
 * mirx_index_last_stats / _last_timings describe the call; left_out counts the dropped candidates.  No host wait beyond the
 * routes' own, no floating-point atomics; the result does not depend on scheduling.
 */
int mirx_index_search_leave_out(mirx_index *ix, const float *queries, int64_t nq, int k, const int64_t *exclude_ids_or_null,
                                const uint8_t *allow_or_null, const int32_t *row_codes, const int32_t *query_codes,
                                int64_t max_left_out, float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids,
                                void *stream);

/* Counters of the most recent range search on an index. */
typedef struct mirx_range_stats {
    int64_t nq;               /* queries in the call                                                     */
    int64_t filter_answered;  /* answered by the filter GEMM + fp64 re-score of every candidate          */
    int64_t exact_answered;   /* answered by the exact scan (routed there, or their candidates overflowed) */
    int64_t candidates;       /* rows that passed the threshold, summed over the filter's queries        */
    int64_t hits;             /* rows returned, summed over queries                                      */
} mirx_range_stats;

/*
 * Exact range search: EVERY row within a radius, not the best k.  pymilvus' collection.search(..., param={"params":
 * {"radius": .., "range_filter": ..}}) (the reference only ever passes nprobe / ef there, milvus/milvus_retrieval.py:80-86);
 * the near-duplicate / leakage self-join over a gallery with exclude_ids = the row's own id.
 * Membership is decided on the fp64 ranking score s (what mirx_index_search_f64 returns: the lane-tree dot product for
 * MIRX_METRIC_IP, MINUS THE SQUARED distance for MIRX_METRIC_NEG_L2 -- not the rounded fp32 value that is reported):
 *     row r is a hit of query i  <=>  lo < s(i, r) <= hi,  allow[r] != 0 (when a mask is given),  id[r] != exclude_ids[i]
 *   q            device, [nq, dim] fp32
 *   lo, hi       the bounds; lo = -inf returns every eligible row, hi = +inf is "no upper bound"; a NaN: MIRX_EINVAL;
 *                hi <= lo: every query is empty and nothing is launched
 *   exclude_ids  device, nq int64, or NULL
 *   allow        n_allow bytes, one per row, non-zero = eligible, a host or a device pointer, or NULL with n_allow = 0;
 *                otherwise n_allow != mirx_index_size: MIRX_EINVAL (the conventions of mirx_index_search_masked)
 *   out_lims     device, [nq + 1] int64: the hits of query i are the entries lims[i] .. lims[i + 1] of what
 *                mirx_index_range_fetch copies out; lims[0] = 0, lims[nq] = *out_total
 *   out_total    host: the number of hits
 * Within a query the hits are ordered by score descending, equal scores by ascending id (mirx_index_rank_all's order).
 * Routes (the answer never depends on the route; no hit is decided from an approximate score):
 *   filter  tiers on auto, size >= 32768, lo > -inf: the filter GEMM of mirx_index_search, unchanged, with a threshold derived
 *           from lo and the GEMM's error bound instead of from a sample (every row with s > lo passes it); EVERY candidate is
 *           re-scored in fp64 and tested.  A query with more than 1280 candidates (or an overflowed overflow list) goes to
 *   exact   fp64 scores of all rows, the radix ranking of mirx_index_rank_top with masked / excluded rows behind every score,
 *           then the span [first s <= hi, first s <= lo) of the sorted keys by binary search.  Also: small galleries,
 *           MIRX_TIER_EXACT_ONLY, lo = -inf.  Cost and workspace per query are those of mirx_index_rank_top.
 * Synchronous in the host sense: one host wait per internal batch of 8192 queries on the filter route (the overflow counter and
 * the batch's hit count travel together), one more per sub-batch of the exact route.  The hits stay in a scratch of the index
 * (16 bytes per hit, besides the staging rows of a filter batch: 1280 * 16 bytes per query) until mirx_index_range_fetch copies
 * them out.  More than 2^28 hits in a call (MIRX_OPT_RANGE_MAX_HITS lowers it for tests): MIRX_ENOMEM, the index stays usable.
 * Between mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.  No atomics decide a position: two calls return the
 * same arrays.
 *
 * mirx_index_range_fetch: the `total` hits of the last range search as arrays of length total (device): fp32 reported values
 *   (metric 0: dot, metric 1: -L2) and / or the fp64 ranking scores (either may be NULL, not both), and ids.  Without a
 *   preceding range search, or after any other search / rank / add / remove call on the index: MIRX_ESTATE.
 * mirx_index_range_last_stats: waits for the device, then copies the counters of the last range search.
 */
int mirx_index_range_search(mirx_index *ix, const float *q, int64_t nq, double lo, double hi, const int64_t *exclude_ids_or_null,
                            const uint8_t *allow_or_null, int64_t n_allow, int64_t *out_lims, int64_t *out_total, void *stream);
int mirx_index_range_fetch(mirx_index *ix, float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids, void *stream);
int mirx_index_range_last_stats(mirx_index *ix, mirx_range_stats *out);

/* Waits for `stream`, then copies the counters of the last search. */
int mirx_index_last_stats(mirx_index *ix, void *stream, mirx_search_stats *out);

/*
 * Device time of each stage of the last search in milliseconds, measured with HIP events
 * recorded on the search's own stream (needs MIRX_OPT_PROFILE = 1 before the search; stages
 * that did not run report 0; a search split into several internal passes reports sums).
 * out_ms: host array of MIRX_NUM_STAGES floats.
 */
int mirx_index_last_timings(mirx_index *ix, float *out_ms);

/*
 * Full ranking of every gallery row for each query (row = query): replaces
 * torch.argsort(dists, dim=0, descending=True) (test.py:1090,179) and the
 * top_k = num_entities search of query_nih_zilliz.py:53-63.  out_ids: device [nq, size]
 * int64 (excluded row last); out_scores_or_null: device [nq, size] fp32 reported values.
 * Order: score descending, equal scores by ascending id (-0.0 and +0.0 are equal); rows with equal ids keep row order.
 * Up to 65536 rows the sort is a bitonic network, above that a segmented radix sort over 64-bit images of the fp64 scores
 * (MIRX_OPT_RANK_SORT forces either).  The radix sort works on batches of queries with 32 bytes of workspace per gallery row
 * and query, at most 512 MiB unless one query needs more; the size is bounded by 2^31 rows and by that allocation
 * (MIRX_ENOMEM).  NaN scores have no defined place in either sort.  Between mirx_index_search_begin and mirx_index_search_end:
 * MIRX_ESTATE.
 */
int mirx_index_rank_all(mirx_index *ix, const float *q, int64_t nq,
                        const int64_t *exclude_ids_or_null, int64_t *out_ids,
                        float *out_scores_or_null, void *stream);

/*
 * The first k entries of the same ranking, for 1 <= k <= size, without an [nq, size] array on the caller's side: the search
 * for k past mirx_index_search's 1024 (Milvus' collection.search allows limit = 16384; query_nih_zilliz.py:53-63 passes
 * top_k = num_entities).  Arguments and conventions are those of mirx_index_search_begin, not of mirx_index_rank_all: the row
 * with the excluded id is LEFT OUT, slots past the number of eligible rows read id -1 and -inf, and either score output may be
 * NULL (not both): out_scores fp32 reported values, out_rank_scores the fp64 ranking scores, [nq, k] each.  Always the radix
 * sort of the whole gallery (MIRX_OPT_RANK_SORT does not apply); cost and workspace are those of mirx_index_rank_all.
 * Between mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.
 */
int mirx_index_rank_top(mirx_index *ix, const float *q, int64_t nq, int64_t k, const int64_t *exclude_ids_or_null,
                        float *out_scores_or_null, double *out_rank_scores_or_null, int64_t *out_ids, void *stream);

/*
 * mirx_index_rank_top under a row mask (allow / n_allow as in mirx_index_search_masked; 1 <= k <= size): the first k entries of
 * the ranking of the allowed rows, the excluded id left out, (-1, -inf) in the slots past the eligible rows -- what
 * mirx_index_rank_top returns on a fresh index of the allowed rows, bit for bit.  Cost: that of the unmasked call whatever the
 * mask, all ones included -- every row is scored and sorted (32 bytes of workspace per row and query), masked rows carry the key
 * behind every score's -- plus two small passes per batch of queries that read the allow bytes themselves (a host mask is copied
 * to the device first); the mask is neither counted nor scanned and the host does not wait.  MIRX_ESTATE as for
 * mirx_index_search_masked.
 */
int mirx_index_rank_top_masked(mirx_index *ix, const float *q, int64_t nq, int64_t k, const int64_t *exclude_ids_or_null,
                               const uint8_t *allow, int64_t n_allow, float *out_scores_or_null,
                               double *out_rank_scores_or_null, int64_t *out_ids, void *stream);

/*
 * For tests.  mirx_rank_key: the radix sort's 64-bit key of an fp64 ranking score -- key(a) < key(b) iff a > b, and
 * key(-0.0) == key(+0.0).  mirx_rank_sort_tile: elements per workgroup tile of its scatter (the sizes around multiples of it
 * are the sort's edges).  Neither touches a device.
 */
uint64_t mirx_rank_key(double score);
int mirx_rank_sort_tile(void);

/*
 * Merge per-shard top-k lists (multi-GPU: after the all-gather of SURVEY 8e).
 * in_scores/in_ids: device [nshard, nq, k] fp64 ranking scores / int64 ids; out: [nq, k].
 * Same order rule as search (score desc, id asc); id -1 entries sort last.
 */
int mirx_topk_merge(const double *in_scores, const int64_t *in_ids, int nshard, int64_t nq,
                    int k, int metric, double *out_rank_scores, float *out_scores,
                    int64_t *out_ids, void *stream);

/*
 * mirx_conv1x1_bn_relu with the operands carried as three bf16 terms each (x = xh + xm + xl, six bf16
 * MFMAs per product block, fp32 accumulation): fp32-grade results at 2.67x less matrix-pipe time, for
 * the layers with many input channels.  Same arguments as mirx_conv1x1_bn_relu except the weights:
 * w3 = device bf16 [cout / 128][cin / 16][3][128][16], the three terms of W[co, k] (already multiplied
 * by the folded norm2 scale) for output block co / 128 and input stage k / 16 (mirx.model._split3_weights),
 * and the output batch stride: image b is written at y + b * y_batch_stride as [cout, hw] (cout * hw for a
 * packed tensor; the channel-prefix of the next dense block's buffer for a transition).
 * cin % 16 == 0, cout % 128 == 0; any hw.
 */
int mirx_conv1x1_bn_relu_split3(const float *x, int64_t x_batch_stride, int cin, const float *scale1_or_null,
                                const float *shift1_or_null, const void *w3, const float *bias_or_null,
                                int64_t n, int hw, int cout, int relu_out, float *y, int64_t y_batch_stride,
                                void *stream);

/*
 * The two-fp16-term DenseNet path (224 x 224 inputs).  fp16 has 5 exponent bits, so the RANGE of every buffer travels with
 * it, PER IMAGE: a "range row" is device fp32 [n] (one float per image of the call, zeroed by the caller once per forward);
 * every mirx kernel that writes image b of a dense block's buffer folds the largest |value| it wrote into row[b] (unsigned
 * atomic max on the float bits), and every kernel that reads image b scales what it stages by a power of two derived from
 * row[b] alone.  An image's arithmetic therefore does not depend on its batch mates; a non-finite value makes THAT image's
 * outputs NaN (never a silently wrong finite value) and leaves the others untouched.
 *
 * mirx_conv1x1_bn_relu_split2h: mirx_conv1x1_bn_relu_split3 with TWO fp16 terms per operand (three MFMAs per product block
 * instead of six).  `in_range_or_null` = range row of x; the kernel stages act_in(x_b) * 2^s with
 *     bound_b = in_ks * row[b] + in_kb         (in_ks = max |scale1|, in_kb = max |shift1|; 1, 0 without prologue;
 *                                               row NULL: bound = in_kb, a caller-proved constant)
 * and s chosen so that bound_b * 2^s is in [2^14, 2^15).  w2 = device fp16 [cout / 128][cin / 16][2][128][16]: the two terms
 * of W[co, k] * ws[co], ws a power of two per output channel (mirx.model._split2h_weights); oscale = device fp32 [cout] =
 * 1 / ws.  `out_range_or_null`: range row of y.
 * x_plane_stride / y_plane_stride: floats between consecutive channel planes of x / y (0 = hw, packed planes).
 * Otherwise the contract of mirx_conv1x1_bn_relu_split3 (reference: the conv1 / transition conv calls inside
 * torchvision densenet121, model.py:53-60).
 */
int mirx_conv1x1_bn_relu_split2h(const float *x, int64_t x_batch_stride, int cin, const float *scale1_or_null,
                                 const float *shift1_or_null, const void *w2, const float *oscale,
                                 const float *bias_or_null, int64_t n, int hw, int cout, int relu_out, float *y,
                                 int64_t y_batch_stride, const float *in_range_or_null, float in_ks, float in_kb,
                                 float *out_range_or_null, int64_t x_plane_stride, int64_t y_plane_stride, void *stream);

/*
 * The dense layer with the 128-channel bottleneck handed over ALREADY SPLIT into its two fp16 terms (same bytes as fp32,
 * but the 3x3 conv then stages it by LDS DMA alone -- no register prefetch, no split, no LDS stores -- and the 1x1 conv
 * writes 16-byte runs instead of 4-byte channel-plane stores):
 *   mirx_conv1x1_bn_relu_split2h_terms: mirx_conv1x1_bn_relu_split2h for cout = 128 with relu, writing
 *       y_terms = device fp16 [n][8 groups][2 terms][hw][16]: group g holds the 16 channels
 *       64 (g >> 2) + 32 ((g >> 1) & 1) + 4 (g & 1) + {0..3, 8..11, 16..19, 24..27} (mirx.model.YTERMS_CHANNEL_ORDER; the
 *       consumer's weights use the same order), image b scaled by 2^t where |y_b| <= y_ks * bound_b + y_kb
 *       (y_ks = max_o sum_c |W[o, c]|, y_kb = max |bias|: a bound known before the kernel runs) is brought into
 *       [2^14, 2^15); y_inv_out = device fp32 [n] receives 2^-t of every image.
 *   mirx_conv3x3_direct_terms_nchw: the 3x3 conv (128 -> 32, pad 1) as a direct implicit GEMM on such y_terms and y_inv
 *       (device fp32 [n]); the padding ring of the staged strip comes from out-of-range buffer loads (zero); w2 = device fp16
 *       [8 stages][9 taps][2 terms][32 oc][16 c] in the permuted channel order, scaled per output channel by a power of two
 *       (mirx.model._conv3x3_weights_split2h), oscale = device fp32 [32] = 1 / that scale.  side 56 / 28 / 14, and 7 (four
 *       whole images per workgroup, each with its own zero ring).  `out_range_or_null`: range row of `out`.
 *   x_plane_stride / out_plane_stride: floats between consecutive channel planes of the dense block's buffer (0 = packed,
 *       hw resp. side^2).
 * (reference: the conv1 / conv2 calls inside torchvision densenet121, model.py:53-60)
 */
int mirx_conv1x1_bn_relu_split2h_terms(const float *x, int64_t x_batch_stride, int cin, const float *scale1,
                                       const float *shift1, const void *w2, const float *oscale, const float *bias,
                                       int64_t n, int hw, void *y_terms, const float *in_range, float in_ks, float in_kb,
                                       float y_ks, float y_kb, float *y_inv_out, int64_t x_plane_stride, void *stream);
int mirx_conv3x3_direct_terms_nchw(const void *y_terms, const void *w2, const float *oscale, int64_t n, int side, float *out,
                                   int64_t out_batch_stride, const float *y_inv, float *out_range_or_null,
                                   int64_t out_plane_stride, void *stream);
/*
 * mirx_conv3x3_direct_terms_nchw_pool (sides 56 / 28 / 14): the same launch ALSO writes the transition's pooled input for
 * its 32 new channels -- pooled[b, oc] = avgpool2x2(relu(out[b, oc] * pool_scale[oc] + pool_shift[oc])) with images
 * `pooled_batch_stride` floats apart and packed (side/2)^2 planes; pool_scale / pool_shift / pooled already point at this
 * layer's first channel.  The values are computed from the stored fp32 outputs by the same operations in the same order as
 * mirx_bn_relu_avgpool2: bit-identical to running that pass afterwards, without reading the block's map from HBM again
 * (the transition's mirx_bn_relu_avgpool2_into then covers only the block's first channels).  Exists in the strip kernel
 * only: mirx_conv3x3_small_launch(n, side) = 1 means a launch of n images takes the one-wave-per-block kernel (see
 * mirx_set_tuning) and this entry point refuses it.
 * (reference: torchvision _DenseLayer.conv2 followed, at the end of the block, by _Transition.norm / relu / pool, model.py:53-60)
 */
int mirx_conv3x3_direct_terms_nchw_pool(const void *y_terms, const void *w2, const float *oscale, int64_t n, int side, float *out,
                                        int64_t out_batch_stride, const float *y_inv, float *out_range_or_null,
                                        int64_t out_plane_stride, const float *pool_scale, const float *pool_shift,
                                        float *pooled, int64_t pooled_batch_stride, void *stream);
int mirx_conv3x3_small_launch(int64_t n, int side);

/*
 * mirx_dense_layer_fused: the dense layer of the 14 x 14 and 7 x 7 maps (dense blocks 3 and 4) in ONE launch --
 *     buf[b, cin : cin + 32] = conv2_3x3( relu( conv1_1x1( relu( buf[b, 0 : cin] * scale1 + shift1 ) ) + bias ) )
 * with the 128-channel bottleneck of a 196-pixel unit (one 14 x 14 image, four 7 x 7 images) kept in the CU's LDS: it never
 * reaches HBM.  Arguments as mirx_conv1x1_bn_relu_split2h_terms (w2, oscale, bias, in_ks, in_kb, y_ks, y_kb) and
 * mirx_conv3x3_direct_terms_nchw (c3w2 in the permuted channel order, c3oscale); buf = device fp32 [n, >= cin + 32, side^2]
 * (packed planes: plane_stride 0 or side^2; 16-byte aligned) at batch_stride floats per image (a multiple of 4); range_row = the buffer's range row (device fp32 [n]): read
 * for the input bound of every image, then raised to the largest |value| of its 32 new channels.  The 32 channels are
 * bit-identical to the two-launch form.  cin % 32 == 0, 128 <= cin <= 1024.
 * (reference: _DenseLayer of torchvision densenet121, model.py:53-60)
 */
int mirx_dense_layer_fused(float *buf, int64_t batch_stride, int64_t plane_stride, int cin, const float *scale1,
                           const float *shift1, const void *w2, const float *oscale, const float *bias, const void *c3w2,
                           const float *c3oscale, int64_t n, int side, float *range_row, float in_ks, float in_kb, float y_ks,
                           float y_kb, void *stream);

/* mirx_range_absmax: range_row[b] = max(range_row[b], largest |x| of image b), x = n images of `per_image` contiguous
 * fp32 each -- the range of the input images for mirx_stem_conv7_bn_relu_pool_split2h_into, the stem (conv 7x7 / 2 + norm0 +
 * relu0 + maxpool 3x3 / 2, one kernel) on two fp16 terms per operand: w2 = device fp16 [2][11][2][32][16], oscale = device
 * fp32 [64] (mirx.model._stem_weights_split2h); image b is written at y + b * y_batch_stride (the channel prefix of dense
 * block 1's buffer: no copy); in_range = range row of x, out_range_or_null = range row of y.  n <= 65535.
 * (reference: conv0 / norm0 / relu0 / pool0 of torchvision densenet121, model.py:53-60) */
int mirx_range_absmax(const float *x, int64_t per_image, int64_t n, float *range_row, void *stream);
/* The same two entry points for RAW 8-bit images x = device uint8 [n, 3, h, w] (hw = h * w): the reference's ToTensor +
 * Normalize (x = u / 255, then (x - mean3[c]) / std3[c] in fp32: test.py:1309-1332) is applied while the stem stages its input
 * patch (and by the range pass), through a 3 x 256 table built with exactly those operations -- the embeddings are
 * bit-identical to feeding the normalised fp32 tensor, at a quarter of the input bytes over PCIe and out of HBM.
 * mean3 / std3 = device fp32 [3]. */
int mirx_range_absmax_u8(const uint8_t *x, int64_t hw, int64_t n, const float *mean3, const float *std3, float *range_row,
                         void *stream);
int mirx_stem_conv7_bn_relu_pool_split2h_u8_into(const uint8_t *x, const float *mean3, const float *std3, const void *w2,
                                                 const float *oscale, const float *scale, const float *shift, int64_t n, int h,
                                                 int w, float *y, int64_t y_batch_stride, const float *in_range,
                                                 float *out_range_or_null, void *stream);
int mirx_stem_conv7_bn_relu_pool_split2h_into(const float *x, const void *w2, const float *oscale, const float *scale,
                                              const float *shift, int64_t n, int h, int w, float *y, int64_t y_batch_stride,
                                              const float *in_range, float *out_range_or_null, void *stream);

/*
 * Memory-bound glue of the token-major backbones, so that their forward runs without a library kernel:
 *
 * mirx_layernorm: y = (x - mean) / sqrt(var + eps) * gamma + beta over the last axis of x [m, c] (nn.LayerNorm inside
 *   timm ConvNeXtV2 / ViT and transformers SigLIP: model.py:96-100, 459-463, 553-557); biased variance, fp32.
 *   tokens_per_image == 0: y is [m, c] (may alias x); > 0: y is channels-first [m / tpi][c][tpi] (timm LayerNorm2d of the
 *   ConvNeXt stem; c <= 512, y != x).  c % 4 == 0, c <= 8192 (a row lives in one wavefront's registers).
 * mirx_patchify_nchw: non-overlapping patch x patch blocks of x [n, c, h, w] as rows
 *   out[((b * (h/patch) + py) * (w/patch) + px) * row_stride + (ch * patch + ky) * patch + kx], columns beyond
 *   c * patch * patch zeroed: a Conv2d(c, cout, kernel = stride = patch) is patchify + mirx_linear_split3 / _split2h with
 *   weight.flatten(1) (the ViT / SigLIP patch embedding, the ConvNeXt stem and downsample convolutions).  With
 *   ln_gamma / ln_beta every pixel is first normalised over its c channels (timm LayerNorm2d in front of the ConvNeXt
 *   downsample conv).
 * mirx_attention_small: softmax(scale q k^T) v for short query sets, one wavefront per (image, head, query), fp32:
 *   q[(b * n_queries + i) * q_row_stride + hd * head_dim + d], k / v likewise with kv_row_stride, key_mask[b * n_keys + j]
 *   != 0 keeps key j (NULL: all keys; a query whose keys are all masked gives zeros), out [batch, n_queries, heads *
 *   head_dim].  Used for the SigLIP text tower (64 tokens, padding mask: eval_medsiglip.py:164-186) and the SigLIP
 *   attention-pooling head (1 probe query).  head_dim 16 / 32 / 64 / 72.
 */
int mirx_layernorm(const float *x, int64_t m, int c, const float *gamma_or_null, const float *beta_or_null, float eps,
                   float *y, int tokens_per_image, void *stream);
int mirx_patchify_nchw(const float *x, int64_t n, int c, int h, int w, int patch, const float *ln_gamma_or_null,
                       const float *ln_beta_or_null, float eps, float *out, int row_stride, void *stream);
int mirx_attention_small(const float *q, int64_t q_row_stride, const float *k, const float *v, int64_t kv_row_stride,
                         const uint8_t *key_mask_or_null, int64_t batch, int heads, int head_dim, int n_queries, int n_keys,
                         float scale, float *out, void *stream);

/*
 * Linear layer of the token-major backbones (replaces the nn.Linear calls inside the timm / transformers
 * models the reference instantiates: model.py:448-494 DinoV2, model.py:87-118 ConvNeXtV2,
 * model.py:536-638 MedSigLIP vision tower), fp32-grade on the bf16 matrix pipe with three bf16 terms per operand:
 *     y[i, j] = epi( sum_k x[i, k] W[j, k] + bias[j] )
 *     act = 1: exact (erf) GELU;  residual != NULL:  y = residual + gamma[j] * v  (LayerScale + skip; gamma
 *     NULL = 1; y may alias residual).
 * x = device fp32 [m, k] row-major; w3 = device bf16 [ceil(n / 128)][k / 16][3][128][16] (the layout of
 * mirx_conv1x1_bn_relu_split3, mirx.model._split3_weights(W); weight rows beyond n are zero padding);
 * y = device fp32 [m, n].  k % 16 == 0, any n >= 1, any m >= 0.
 */
int mirx_linear_split3(const float *x, int64_t m, int k, const void *w3, const float *bias_or_null, int n, int act,
                       const float *residual_or_null, const float *gamma_or_null, float *y, void *stream);

/*
 * mirx_linear_split3 with TWO fp16 terms per operand (three MFMAs per product block instead of six; same measured
 * error, 1.7x the speed) for inputs whose range the caller can bound:
 *     y = epi( out_scale * sum_k (x[i, k] * x_scale) W2[j, k] + bias[j] ),   epilogues as mirx_linear_split3
 * w2 = device fp16 [ceil(n / 128)][k / 16][2][128][16]: the two terms of W * w_scale, w_scale a power of two
 * (mirx.model._linear_h2_weights); x_scale a power of two with |x * x_scale| <= 65504 for EVERY element (fp16
 * range: the caller's contract -- mirx.model uses this entry only behind a LayerNorm, whose output is bounded by
 * sqrt(C - 1) max|gamma| + max|beta|); out_scale = 1 / (x_scale * w_scale).  k % 16 == 0.
 */
int mirx_linear_split2h(const float *x, int64_t m, int k, const void *w2, const float *bias_or_null, int n, int act,
                        const float *residual_or_null, const float *gamma_or_null, float x_scale, float out_scale,
                        float *y, void *stream);

/*
 * The token-major Linear with BOTH operands pre-split ("terms rows"), the form the ViT / SigLIP towers run on: the same
 * arithmetic as mirx_linear_split2h (two fp16 terms per operand, three MFMAs per product block, fp32 accumulation), but the
 * activations arrive already split, so the kernel is a DMA-fed MFMA GEMM (k_linear_t2.hip).  Replaces nn.Linear inside timm
 * VisionTransformer blocks and transformers SiglipEncoderLayer (model.py:459-463, 553-557 of the reference build them).
 *
 * TERMS ROWS of a matrix a [rows][k] scaled by a power of two s: rows of ceil(k / 32) lines of 128 bytes,
 *     line g = fp16 hi(s a[32 g .. 32 g + 31]) | fp16 lo(..),   hi = fp16(s a), lo = fp16(s a - hi), zero beyond k
 * -- 4 bytes per element like fp32.  Contract: |s a| <= 65504 for every element (callers pass provable bounds).
 *
 * mirx_rows_to_terms:   xt = terms rows of `scale` * x, x = device fp32 [m][k] with `row_stride` floats between rows
 *                       (row_stride % 4 == 0, x 16-byte aligned).  xt: m * ceil32(k) * 4 bytes.
 * mirx_layernorm_terms: mirx_layernorm (token-major form) writing terms rows of `scale` * y instead of fp32.
 * mirx_linear_terms:    v = act( out_scale * sum_k xt[i, k] wt[j, k] + bias[j] ),   out_scale = 1 / (x scale * w scale)
 *                       act 0 none, 1 GELU (erf), 2 GELU (tanh);
 *                       y (fp32 [m][n]) = v, or residual + gamma[j] * v (act 0; gamma NULL = 1; y may alias residual);
 *                       or yt = terms rows of yt_scale * v (no residual) -- the next Linear's input, written in full lines.
 *                       wt = terms rows of W * w scale, ceil(n / 256) * 256 rows (zero beyond n).  n % 4 == 0.
 *                       workspace: a tile (256 tokens x 256 outputs) occupies one CU for its whole K loop, so a launch whose
 *                       tile count is not a multiple of the CU count would end in a mostly empty round.  With a device
 *                       buffer of mirx_linear_terms_workspace_bytes(m, k, n) bytes (0 = not needed; at most 64 MiB) the
 *                       tiles of that last round are cut along k into pieces that run side by side and are summed in piece
 *                       order by a second launch -- deterministic for a given (m, k, n).  NULL = whole tiles only.
 */
int mirx_rows_to_terms(const float *x, int64_t m, int k, int64_t row_stride, float scale, void *xt, void *stream);
/* LayerNorm over the channels of every pixel of channels-last maps x [n_img, h, w, c], written as the 2 x 2 patch rows of a
 * stride-2 convolution: y [n_img, h / 2, w / 2, 4 c] with feature order (ky, kx, channel) -- timm's LayerNorm2d + Conv2d(k = s = 2)
 * downsample of ConvNeXt becomes this + a Linear whose weight is conv.weight.permute(0, 2, 3, 1).reshape(cout, 4 c). */
int mirx_layernorm_patch2_nhwc(const float *x, int64_t n_img, int h, int w, int c, const float *gamma_or_null,
                               const float *beta_or_null, float eps, float *y, void *stream);
int mirx_layernorm_terms(const float *x, int64_t m, int c, const float *gamma_or_null, const float *beta_or_null, float eps,
                         float scale, void *yt, void *stream);
int mirx_linear_terms(const void *xt, int64_t m, int k, const void *wt, const float *bias_or_null, int n, int act,
                      const float *residual_or_null, const float *gamma_or_null, float out_scale, float *y_or_null,
                      void *yt_or_null, float yt_scale, void *workspace_or_null, int64_t workspace_bytes, void *stream);
int64_t mirx_linear_terms_workspace_bytes(int64_t m, int k, int n);

/*
 * Tail of a ConvNeXtV2 block (timm ConvNeXtBlock.forward, used by the reference's model.py:87-118): the second
 * point-wise Linear on the channels-last hidden map, written back channels-first with the block's skip added:
 *     y[b, j, p] = residual[b, j, p] + sum_k (x[b * tpi + p, k] * input_scale[b, k]) W[j, k] + bias[j]
 * x = device fp32 [n_img * tokens_per_image, k]; w3 as in mirx_linear_split3; residual / y = device fp32
 * [n_img, n, tokens_per_image] (NCHW); residual NULL = no skip; y may alias residual.
 * input_scale = device fp32 [n_img, k] or NULL: the GRN factor 1 + weight * gx / (mean gx + eps), applied while x
 * is staged (the GRN shift is constant per feature: the caller adds W . grn_bias to `bias`).
 */
int mirx_linear_split3_nchw(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w3,
                            const float *bias_or_null, int n, const float *residual_or_null,
                            const float *input_scale_or_null, float *y, void *stream);

/*
 * mirx_linear_split3_nchw on TWO fp16 terms per operand (mirx_linear_split2h's arithmetic) for inputs with a known bound:
 *   |x[i, j]| <= x_bound for every element (host scalar, e.g. the provable bound of a Linear fed by a LayerNorm, through GELU);
 *   input_scale (the GRN scale [n_img, k], multiplied into x while it is staged) comes with input_scale_max = device fp32[1]
 *   holding max |input_scale| -- it is computed per forward, so the kernel reads it and derives the power-of-two staging
 *   scale from x_bound * input_scale_max[0] itself (no host round trip; a non-finite bound makes every output NaN);
 *   w2 / w_inv = mirx.model._linear_h2_weights (the two fp16 terms of W * w_scale, and 1 / w_scale).
 * Reference: timm ConvNeXtBlock (mlp.fc2 after GRN, permute back, + shortcut) and the LayerNorm2d + 2x2/2 downsample conv,
 * as used by the reference's model.py:87-118.
 */
int mirx_linear_split2h_nchw(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w2,
                             const float *bias_or_null, int n, const float *residual_or_null,
                             const float *input_scale_or_null, float x_bound, const float *input_scale_max_or_null,
                             float w_inv, float *y, void *stream);
/* fc1 of a ConvNeXtV2 block with the global response norm's reduction folded in: y = gelu(mirx_linear_split2h(x)) (row-major
 * [n_img * tokens_per_image, n]) AND gx[b, j] = || y[b, :, j] ||_2 (what mirx_grn_norm_nhwc would compute from y in a pass of its
 * own): every workgroup returns the column sums of y^2 of its 128 token rows split by image in `partials` (device fp32,
 * ceil(n_img * tokens_per_image / 128) * 2 * n floats), a second small launch adds them in tile order.  tokens_per_image >= 128.
 * Bit-reproducible. */
int mirx_linear_split2h_gelu_grn(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w2,
                                 const float *bias_or_null, int n, float x_scale, float out_scale, float *y, float *partials,
                                 float *gx, void *stream);
/* The same block tail for a channels-last residual stream (the ConvNeXtV2 fast path): residual and y are row-major
 * [n_img * tokens_per_image, n] (y may alias the residual), input_scale / input_scale_max are required. */
int mirx_linear_split2h_grn_rows(const float *x, int64_t n_img, int tokens_per_image, int k, const void *w2,
                                 const float *bias_or_null, int n, const float *residual_or_null, const float *input_scale,
                                 float x_bound, const float *input_scale_max, float w_inv, float *y, void *stream);

/*
 * Global response normalisation of ConvNeXtV2 (timm GlobalResponseNorm, channels last) as two HBM passes:
 *   mirx_grn_norm_nhwc:  gx[b, c] = || x[b, :, c] ||_2              x = device fp32 [n, hw, c], gx = [n, c]
 * with scale = 1 + weight * gx / (mean_c gx + 1e-6) and shift = bias formed by the caller on [n, c].
 * n <= 65535.  Fixed summation order (bit-reproducible).
 */
int mirx_grn_norm_nhwc(const float *x, int64_t n, int hw, int c, float *gx, void *stream);
/* The GRN scale vector in one launch: scale[b, j] = 1 + weight[j] * gx[b, j] / (mean_j gx[b, :] + eps)  (timm
 * GlobalResponseNorm: x * (1 + weight * Nx) + bias with Nx = Gx / (mean Gx + eps), eps = 1e-6), and scale_max[0] = the largest
 * |scale| over the batch -- the device-side bound mirx_linear_split2h_nchw reads; combined by atomic max, so the caller ZEROES
 * scale_max[0] first. */
int mirx_grn_scale(const float *gx, const float *weight, int64_t n, int c, float eps, float *scale, float *scale_max,
                   void *stream);

/*
 * 3x3 convolution of a DenseNet dense layer (128 -> 32 channels, stride 1, pad 1, no bias): conv2 of
 * torchvision's _DenseLayer (model.py:53), as Winograd F(2x2,3x3) on fp32 MFMA.  x: device NCHW fp32
 * [n, 128, side, side] (packed), side = 56, 28, 14 or 7.  u: device fp32 [16 stages][16][8][32] = the
 * transformed weights U_xi[oc, c] = (G g G^T)_xi of the layer, stage s holding channels 8s .. 8s+7 as
 * [xi = 4i + j][c][oc] (mirx.model prepares it once per layer).  The 32 output channels of image b are
 * written at out + b * out_batch_stride as [32, side, side] -- i.e. directly into the layer's slice of
 * the dense-block buffer.  Other sizes: MIRX_EINVAL (use the library convolution).
 */
int mirx_conv3x3_winograd_nchw(const float *x, const float *u, int64_t n, int side, float *out,
                               int64_t out_batch_stride, void *stream);

/*
 * mirx_conv3x3_winograd_nchw with the 16 Winograd-domain channel GEMMs on three-term bf16 MFMAs (fp32-grade,
 * see mirx_conv1x1_bn_relu_split3): same x / out / out_batch_stride; u3 = device bf16
 * [cin / 16][ij = 4 i + j][3 terms][32 oc][16 channels], the split of U = G g G^T
 * (mirx.model._winograd_weights_split3).  side in {56, 28, 14}; the 7 x 7 maps use mirx_conv3x3_winograd_nchw.
 */
int mirx_conv3x3_winograd_split3_nchw(const float *x, const void *u3, int64_t n, int side, float *out,
                                      int64_t out_batch_stride, void *stream);

/*
 * The same convolution (conv2 of a dense layer: 128 -> 32 channels, 3x3, pad 1) as a DIRECT implicit GEMM on
 * three-term bf16 MFMAs (no Winograd transform: K = 9 taps x 128 channels; fp32-grade): same x / out /
 * out_batch_stride; w3 = device bf16 [8 stages][9 taps = 3 ky + kx][3 terms][32 oc][16 channels]
 * (mirx.model._conv3x3_weights_split3).  side in {56, 28, 14}.
 */
int mirx_conv3x3_direct_split3_nchw(const float *x, const void *w3, int64_t n, int side, float *out,
                                    int64_t out_batch_stride, void *stream);

/*
 * Multi-head self-attention of the ViT backbones, fp32: out = softmax(q k^T * scale) v per (image,
 * head), scores never materialised.  Replaces the attention of timm's `vit_base_patch14_dinov2`
 * blocks (model.py:459-463; nih_multilabel_retrieval.py:175-221).  qkv: device [batch, n_tokens, 3,
 * heads, head_dim] fp32, exactly the output of the block's qkv Linear; out: device [batch, n_tokens,
 * heads, head_dim] fp32 (= [batch, n_tokens, C], no head transpose).  head_dim in {32, 64, 72, 96}
 * (64: ViT-B / DINOv2; 72: the SigLIP-So400m tower of MedSigLIP, model.py:536-638).
 */
int mirx_attention_qkv_f32(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim,
                           float scale, float *out, void *stream);

/*
 * mirx_attention_qkv_f32 with both GEMMs on three-term bf16 MFMAs (Q, K, V and the probabilities each carried
 * as xh + xm + xl; fp32-grade, see mirx_conv1x1_bn_relu_split3): same arguments, result layout and head_dim set.
 * Like the two-fp16-term entry points below it reads K and V through 32-bit buffer offsets, so one image's qkv rows must
 * stay below 2 GiB: n_tokens * 3 * heads * head_dim * 4 < 2^31, else MIRX_EHIP (invalid value) before anything is launched.
 */
int mirx_attention_qkv_f32_split3(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim,
                                  float scale, float *out, void *stream);

/*
 * mirx_attention_qkv_f32 with both GEMMs on TWO fp16 terms per operand (three MFMAs per product block; see
 * mirx_linear_split2h).  qk_bound >= max |q|, |k| and v_bound >= max |v| over the packed projection are the caller's
 * contract (fp16 range; mirx.model derives them from the LayerNorm in front of the projection and its row norms);
 * the library turns them into exact power-of-two scales.  head_dim 64 (DINOv2 / ViT-B), or 32 / 72 / 96 through the
 * general kernel (72 = the SigLIP-So400m tower of MedSigLIP).
 */
int mirx_attention_qkv_f32_split2h(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim,
                                   float scale, float qk_bound, float v_bound, float *out, void *stream);
/* The same attention with the result written as terms rows of out_scale * out (include above: mirx_linear_terms), |out| <=
 * v_bound (a softmax-weighted average of V rows), so that the output projection reads it without a conversion pass.
 * out_terms: batch * n_tokens rows of ceil32(heads * head_dim) * 4 bytes. */
int mirx_attention_qkv_f32_split2h_terms(const float *qkv, int64_t batch, int n_tokens, int heads, int head_dim, float scale,
                                         float qk_bound, float v_bound, float out_scale, void *out_terms, void *stream);

/*
 * Metric tail over ranked lists, on the device: one pass per query over its
 * ranking `ranks[q, 0..n)` (gallery row ids, best first; rows `row_stride` apart) gives
 *   out_ap[q]      AP of the list: ap_kind 0 = the trapezoidal compute_ap of test.py:58-92 summed the
 *                  way compute_map does (test.py:95-146), ap_kind 1 = mean of precision at each relevant
 *                  rank (compute_map_multilabel test.py:941-985, fusion_eval/metrics.py:41-94);
 *                  NaN when the list holds no relevant id (the reference's "nempty" / skipped queries);
 *   out_cnt[q, j]  relevant ids within the first kappas[j] ranks (retrieval_accuracy test.py:38-54;
 *                  precision@kappa test.py:137-142; mP@k / R@k of fusion_eval/metrics.py:70-86);
 *   out_nrel[q]    relevant ids in the whole list; out_maxpos[q] largest 1-based relevant rank (0 = none).
 * Relevance of gallery row `id` for query q: rel_kind 0 -> gallery_labels[id] == query_labels[q];
 * rel_kind 1 -> labels are multi-hot bit masks (<= 64 classes) and
 * |a & b| / (|a | b| + 1e-8) > jaccard_threshold (test.py:956-965).  query_ids_or_null[q] is never
 * relevant (self-exclusion: binary_relevance[i] = 0, test.py:966).  Ids outside [0, n_labels) are
 * not relevant.  All pointers are device pointers except kappas (host, nk <= 8).
 */
int mirx_rank_metrics(const int64_t *ranks, int64_t nq, int64_t n, int64_t row_stride,
                      const int64_t *gallery_labels, int64_t n_labels, const int64_t *query_labels,
                      const int64_t *query_ids_or_null, int drop_self, int rel_kind,
                      double jaccard_threshold, int ap_kind, const int32_t *kappas, int nk,
                      double *out_ap, int64_t *out_cnt, int64_t *out_nrel, int64_t *out_maxpos,
                      void *stream);

/*
 * mirx_rank_metrics with a group taken out of every list (leave-group-out evaluation: a patient's other studies are neither
 * hits nor misses).  gallery_codes[id] (device [n_labels], indexed like gallery_labels) and query_codes[q] (device [nq]): entry
 * `id` is taken out of query q's list iff query_codes[q] >= 0 && 0 <= id < n_labels && gallery_codes[id] == query_codes[q].
 * Such an entry is treated exactly like the dropped self entry of drop_self: it has no position (later ranks move up), is never
 * relevant and counts in none of out_cnt, out_nrel, out_maxpos; the trapezoidal AP and the caller's kq = min(max(pos), kappa)
 * rule therefore apply to the list AFTER removal.  A negative query code leaves nothing out (all negative: mirx_rank_metrics'
 * outputs bit for bit); a negative gallery code is the field's null and is never left out.  out_ap is NaN when no relevant entry
 * remains.  Everything else, the MIRX_EINVAL cases included (null codes among them), is mirx_rank_metrics'.
 */
int mirx_rank_metrics_grouped(const int64_t *ranks, int64_t nq, int64_t n, int64_t row_stride,
                              const int64_t *gallery_labels, int64_t n_labels, const int64_t *query_labels,
                              const int64_t *query_ids_or_null, int drop_self, int rel_kind,
                              double jaccard_threshold, int ap_kind, const int32_t *kappas, int nk,
                              const int32_t *gallery_codes, const int32_t *query_codes,
                              double *out_ap, int64_t *out_cnt, int64_t *out_nrel, int64_t *out_maxpos,
                              void *stream);

/*
 * The full ranking of every query, evaluated without ever leaving the sort's workspace: per query the outputs are those of
 * mirx_index_rank_all(q, exclude_ids_or_null) followed by mirx_rank_metrics_grouped over that ranking (labels and codes mapped
 * from row order to ids) -- integer outputs equal, out_ap within 1e-12, NaN in the same places -- and no [nq, size] array exists
 * on either side of the call.  row_labels / row_codes_or_null: device [size] in ROW order (the order of the index's ids);
 * query_labels / query_codes_or_null: device [nq].  Both codes pointers or neither (MIRX_EINVAL).  self_kind says what the
 * excluded id is: 0 = an ordinary last entry (mirx_rank_metrics with query_ids = NULL), 1 = never relevant (query_ids = exclude,
 * drop_self = 0), 2 = also taken out of the list (drop_self = 1); 1 and 2 need exclude_ids.  rel_kind, jaccard_threshold,
 * ap_kind, kappas (host), nk <= 8 as in mirx_rank_metrics.  Batches, workspace (32 bytes per row and query of a batch, plus 20
 * bytes per 4096 rows) and the sort are mirx_index_rank_top's; there is no host wait.  A query's out_ap bits depend on the
 * gallery and the query alone, not on nq or its place in the call.  MIRX_ESTATE between mirx_index_search_begin and _end.
 */
int mirx_index_rank_metrics(mirx_index *ix, const float *q, int64_t nq, const int64_t *exclude_ids_or_null, int self_kind,
                            const int64_t *row_labels, const int64_t *query_labels,
                            const int32_t *row_codes_or_null, const int32_t *query_codes_or_null,
                            int rel_kind, double jaccard_threshold, int ap_kind, const int32_t *kappas, int nk,
                            double *out_ap, int64_t *out_cnt, int64_t *out_nrel, int64_t *out_maxpos, void *stream);

/*
 * Grouping search: the best hits PER GROUP instead of the best rows -- pymilvus' collection.search(..., group_by_field=..,
 * group_size=.., strict_group_size=True), which the reference's callers get from their Milvus service and its own scripts never
 * exercise ("the nearest case of every diagnosis", "ten different patients, not ten follow-ups of one").  The contract, per
 * query i, over the index's ranking (fp64 ranking score descending, equal scores by ascending id: mirx_index_rank_all's order):
 *   - a row is ELIGIBLE when its mask entry is non-zero (if a mask is given) and its id is not the query's excluded id;
 *   - every row carries an integer group code >= 0; c_i(g) = eligible rows of group g, G_i = groups with c_i(g) > 0,
 *     T_i = min(limit, G_i);
 *   - the result is the T_i groups whose best eligible row ranks highest, ordered by that row, each holding its first
 *     min(group_size, c_i(g)) eligible rows in ranking order -- a group is never short while it has rows left.
 *   Equivalently, walk the ranking of the eligible rows: a group opens at its first row while fewer than `limit` groups are
 *   open; a row is kept while its group is open and holds fewer than group_size rows.
 * Limits of every call below (MIRX_EINVAL, nothing launched): 1 <= limit <= MIRX_GROUP_MAX_LIMIT, 1 <= group_size <=
 * MIRX_GROUP_MAX_SIZE, limit * group_size <= MIRX_GROUP_MAX_HITS (Milvus' own top-k ceiling).  The three calls are the device
 * passes; which prefix to walk, which groups to fill and when to deepen is the caller's (mirx.index.FlatIndex.search_grouped).
 *
 * mirx_group_walk: that walk over a ranked PREFIX, one wavefront per query, 64 entries at a time (a free function over ranked
 * lists, like mirx_rank_metrics; all pointers device).
 *   ranks        [nq, row_stride >= depth] int64, best first: what mirx_index_search / _rank_top return with the excluded id and
 *                the masked rows left out; the first -1 ends the list (the prefix then IS the whole eligible ranking)
 *   table_index  laid out alike, or NULL: the index into group_of of each entry; NULL when the ranked id itself is that index
 *                (ids 0 .. n-1).  The ids written to out_ids are always those of `ranks`.
 *   scores       laid out alike, or NULL: the fp64 ranking scores, copied to out_scores beside each kept id
 *   group_of     [n_table] int64 group code per entry; an entry outside [0, n_table) or a code outside [0, n_groups) is skipped
 *   group_rows   [n_groups] int64 = c(g), the eligible rows per code regardless of the query (mirx_group_count)
 *   live_groups  the number of codes with group_rows > 0
 *   excl_group   [nq] int64 or NULL: the code of the query's excluded row when that row is otherwise eligible, else -1; that
 *                group counts one row less for the query and vanishes from G_i when it was its only one
 *   out_ids      [nq, limit, group_size] int64, -1 in empty slots; out_scores alike (fp64, -inf in empty slots) or NULL
 *   out_codes    [nq, limit] int64, -1 in empty slots; out_kept [nq, limit] int32 rows held per group slot
 *   out_state    [nq, 2] int32: [0] groups open; [1] bit 0 COMPLETE: T_i groups are open and each holds min(group_size, c_i(g))
 *                rows, or the list ended -- the outputs are the contract's answer; bit 1 GROUPS FINAL: T_i groups are open, so
 *                membership and order of the groups are decided and only rows are missing (set whenever bit 0 is)
 * The open groups live in a per-wave LDS hash table (power-of-two slots, >= 2 * limit; linear probing from code mod slots).
 * Inside a chunk the lanes whose row can no longer be kept (group open and full; group not open and no slot left -- both
 * absorbing) drop out at once, the others act in lane order, each looking its group up at its turn.  The walk stops, wave-
 * uniformly, once complete.  No atomics; the outputs do not depend on scheduling.
 *
 * mirx_group_count: out_counts[c] = rows r < n with groups[r] == c and allow_or_null[r] != 0 (NULL = every row), for c in
 * [0, n_groups), n_groups < 2^31; codes outside that range are skipped.  Device pointers; out_counts is zeroed by the call.
 * Integer atomics (the sums do not depend on their order).
 *
 * mirx_index_group_fill: completes groups that are final but short without ranking the gallery.  For each of n_pairs pairs
 * (pair_query, pair_slot) the member rows of the pair's group are members[pair_first .. pair_first + pair_len) -- row POSITIONS
 * of the index, eligible rows only, any order (pair_len <= max_members <= MIRX_GROUP_FILL_MAX; a longer span is cut).  The
 * call prepares the nq queries as the searches do; one workgroup per pair scores every
 * member with the ranking's own lane-tree fp64 score (the bits of mirx_index_search_f64), skips the excluded id and writes the
 * best group_size by (score descending, id ascending) to out_ids / out_rank_scores [nq, limit, group_size] at (query, slot);
 * slots past the members read (-1, -inf).  q: device [nq, dim]; every other pointer device int64.  Between
 * mirx_index_search_begin and mirx_index_search_end: MIRX_ESTATE.  Drops a pending range result like any search.
 *
 * mirx_index_get_ids: ids of rows [first, first + n) (device or host destination), without copying rows.
 */
#define MIRX_GROUP_MAX_LIMIT 1024
#define MIRX_GROUP_MAX_SIZE 64
#define MIRX_GROUP_MAX_HITS 16384
#define MIRX_GROUP_FILL_MAX 4096
int mirx_group_walk(const int64_t *ranks, const int64_t *table_index_or_null, const double *scores_or_null, int64_t nq,
                    int64_t depth, int64_t row_stride, const int64_t *group_of, int64_t n_table, const int64_t *group_rows,
                    int64_t n_groups, int64_t live_groups, const int64_t *excl_group_or_null, int limit, int group_size,
                    int64_t *out_ids, double *out_scores_or_null, int64_t *out_codes, int32_t *out_kept, int32_t *out_state,
                    void *stream);
int mirx_group_count(const int64_t *groups, const uint8_t *allow_or_null, int64_t n, int64_t n_groups, int64_t *out_counts,
                     void *stream);
int mirx_index_group_fill(mirx_index *ix, const float *q, int64_t nq, const int64_t *exclude_ids_or_null, int limit,
                          int group_size, const int64_t *pair_query, const int64_t *pair_slot, const int64_t *pair_first,
                          const int64_t *pair_len, int64_t n_pairs, const int64_t *members, int64_t n_members, int max_members,
                          int64_t *out_ids, double *out_rank_scores, void *stream);
int mirx_index_get_ids(const mirx_index *ix, int64_t first, int64_t n, int64_t *out_ids);

/*
 * Hybrid search: fuses the ranked lists of several search requests into one ranking per query -- pymilvus'
 * hybrid_search(reqs, rerank=RRFRanker() | WeightedRanker(..), limit).  The reference keeps one collection per backbone and
 * joins them on image_path (fusion_eval/, retrieval_analysis/); the caller (mirx.retriever.hybrid_search) turns every ranked id
 * into a DOCUMENT CODE, equal for rows of different collections that carry the same key.  A free function over ranked lists,
 * like mirx_rank_metrics.
 *   codes, distances   device [nq, row_stride >= m]: the lists of the n_requests requests side by side, request r in columns
 *                      [segment_offsets[r], segment_offsets[r + 1]), best first; m = segment_offsets[n_requests].  A code
 *                      outside [0, n_codes) marks an empty slot (-1 by convention).  distances: the fp32 value a hit reports
 *                      (similarity for COSINE / IP, Euclidean distance for L2), finite wherever the code is valid; read by the
 *                      weighted ranker only (may be NULL for MIRX_FUSE_RRF).
 *   segment_offsets    HOST int32 [n_requests + 1], 0 = offsets[0] < offsets[1] < .. (every list has at least one slot)
 *   ranker             MIRX_FUSE_RRF: an entry in slot s of its list (rank s + 1) contributes 1 / (rrf_k + rank), 0 < rrf_k < 16384.
 *                      MIRX_FUSE_WEIGHTED: it contributes weights[r] * n_r(d), d its distance widened to fp64, weights HOST
 *                      double [n_requests] in [0, 1], norms HOST int32 [n_requests]: MIRX_FUSE_NORM_RAW n = d, _COSINE n =
 *                      (1 + d) * 0.5, _IP n = 0.5 + atan(d) / pi, _L2 n = 1 - 2 * atan(d) / pi.  (weights / norms may be NULL
 *                      for MIRX_FUSE_RRF.)
 * A document's score is 0.0 plus its entries' contributions, added one by one in ascending position (hence ascending request),
 * every operation a separate correctly rounded fp64 operation (no fused multiply-add): a float64 restatement reproduces the bits
 * of the RRF, RAW and COSINE forms; the atan forms agree to the device's atan (a few ulp).  Per query the result is the
 * min(limit, distinct codes) documents with the highest score, equal scores by ascending code:
 *   out_codes   [nq, limit] int64, -1 past them;  out_scores [nq, limit] fp64, -inf past them
 *   out_request, out_slot  [nq, limit] int32: the request and the slot in its list of the document's first entry, -1 past them
 *   out_count   [nq] int32
 * One workgroup per query, two bitonic sorts in LDS (16 bytes per slot of the next power of two >= m: 64 KiB at the limit); no
 * atomics, one fixed order of additions: equal inputs give equal outputs, call after call.
 * Limits (MIRX_EINVAL before any device call): 1 <= n_requests <= MIRX_FUSE_MAX_REQUESTS, m <= MIRX_FUSE_MAX_ENTRIES,
 * 1 <= limit <= MIRX_FUSE_MAX_LIMIT, 0 <= n_codes < 2^31, 0 <= nq < 2^31.
 */
#define MIRX_FUSE_MAX_REQUESTS 8
#define MIRX_FUSE_MAX_ENTRIES 4096
#define MIRX_FUSE_MAX_LIMIT 1024
#define MIRX_FUSE_RRF 0
#define MIRX_FUSE_WEIGHTED 1
#define MIRX_FUSE_NORM_RAW 0
#define MIRX_FUSE_NORM_COSINE 1
#define MIRX_FUSE_NORM_IP 2
#define MIRX_FUSE_NORM_L2 3
int mirx_fuse_ranked(const int64_t *codes, const float *distances_or_null, int64_t nq, int64_t row_stride, int64_t n_codes,
                     const int32_t *segment_offsets, int n_requests, int ranker, double rrf_k, const double *weights_or_null,
                     const int32_t *norms_or_null, int limit, int64_t *out_codes, double *out_scores, int32_t *out_request,
                     int32_t *out_slot, int32_t *out_count, void *stream);

/*
 * x <- x / max(||x||_2, 1e-12) row-wise, in place.  Replaces F.normalize(x, dim=1)
 * (model.py:83,116,493,634; milvus_retrieval.py:63).  x: device [n, dim] fp32.
 */
int mirx_l2_normalize(float *x, int64_t n, int dim, void *stream);

/*
 * Embedding head: y[b, c] = mean_{hw} relu(x[b, c, h, w] * scale[c] + shift[c]), then the
 * optional L2 normalisation of each row.  Replaces norm5 -> relu -> AdaptiveAvgPool2d(1)
 * -> flatten -> F.normalize of model.py:59-60,73-74,83 in one pass over the feature map.
 * x: device NCHW fp32 [n, c, hw]; scale/shift: device [c] (folded eval BatchNorm) or NULL
 * for identity; y: device [n, c] fp32.
 */
int mirx_bn_relu_gap_l2norm(const float *x, const float *scale, const float *shift, int64_t n,
                            int c, int hw, int normalize, float *y, void *stream);

/*
 * y = relu(x * scale[c] + shift[c]) for the first c channels of an NCHW fp32 tensor whose
 * images are `x_batch_stride` floats apart (a channel-prefix view of a wider dense-block
 * buffer); y is packed [n, c, hw].  Replaces norm1 -> relu1 (and transition norm -> relu) of
 * torchvision's _DenseLayer / _Transition (model.py:53) in ONE pass instead of two.
 */
int mirx_bn_relu_nchw(const float *x, int64_t x_batch_stride, const float *scale, const float *shift,
                      int64_t n, int c, int hw, float *y, void *stream);

/*
 * Transition front half: y = avgpool2x2(relu(x * scale[c] + shift[c])), x as above with
 * h x w pixels (h, w even), y packed [n, c, h/2, w/2].  The 1x1 transition conv commutes with
 * the average pool, so the caller runs it on the pooled map (4x fewer pixels).
 */
int mirx_bn_relu_avgpool2(const float *x, int64_t x_batch_stride, const float *scale,
                          const float *shift, int64_t n, int c, int h, int w, float *y, int64_t x_plane_stride,
                          void *stream);    /* x_plane_stride: floats between channel planes of x (0 = h * w; else % 4 == 0) */
/* ... the same with y = [n, >= c, h/2, w/2]: images `y_batch_stride` floats apart (the first c channels of a wider pooled map
 * whose other channels mirx_conv3x3_direct_terms_nchw_pool writes) */
int mirx_bn_relu_avgpool2_into(const float *x, int64_t x_batch_stride, const float *scale, const float *shift,
                               int64_t n, int c, int h, int w, float *y, int64_t y_batch_stride, int64_t x_plane_stride,
                               void *stream);

/*
 * DenseNet stem: conv 7x7 stride 2 pad 3 (3 -> 64 channels) + folded BatchNorm + ReLU +
 * max-pool 3x3 stride 2 pad 1, NCHW fp32 in, NCHW fp32 out [n, 64, H/4, W/4].
 * Replaces features.conv0/norm0/relu0/pool0 of torchvision densenet121 (model.py:53).
 * w: device [64, 3, 7, 7]; scale/shift: device [64].  H, W multiples of 4.
 */
int mirx_stem_conv7_bn_relu_pool(const float *x, const float *w, const float *scale,
                                 const float *shift, int64_t n, int h, int wd, float *y,
                                 void *stream);

/*
 * The same stem with the implicit GEMM on three-term bf16 MFMAs (fp32-grade, see mirx_conv1x1_bn_relu_split3).
 * w3 = device bf16 [2 blocks of 32 oc][11 steps][3 terms][32 oc][16 k]: step s, k = 8 g + i is weight
 * (c, ky) = divmod(2 s + g, 7), kx = 2 i for i < 4, 2 (i - 4) + 1 for i >= 4 (kx = 7 and row 21 are zero)
 * -- mirx.model._stem_weights_split3(conv0.weight).  n <= 65535.
 */
int mirx_stem_conv7_bn_relu_pool_split3(const float *x, const void *w3, const float *scale, const float *shift,
                                        int64_t n, int h, int wd, float *y, void *stream);

/*
 * Fused 1x1 convolution of a DenseNet dense layer / transition (fp32 MFMA):
 *     y[b, o, p] = act_out( sum_k wt[k, o] * act_in(x[b, k, p]) + bias[o] )
 * act_in(v) = relu(v * scale[k] + shift[k]) when scale != NULL (norm1 + relu1), identity otherwise;
 * act_out = relu when relu_out != 0 (relu2; norm2 = bias + a scale folded into wt by the caller).
 * Replaces norm1 -> relu1 -> conv1 -> norm2 -> relu2 of torchvision's _DenseLayer (model.py:53) in one
 * pass over the concatenated features.  x: channel-prefix view, image stride x_batch_stride floats,
 * cin % 32 == 0; wt: device [cin, cout] (the conv weight TRANSPOSED), cout % 128 == 0; bias: device
 * [cout] or NULL; y: device packed NCHW [n, cout, hw].
 */
int mirx_conv1x1_bn_relu(const float *x, int64_t x_batch_stride, int cin, const float *scale, const float *shift,
                         const float *wt, const float *bias, int64_t n, int hw, int cout, int relu_out, float *y,
                         void *stream);

/*
 * ConvNeXt block front end: y = permute_NHWC(depthwise_conv7x7(x) + bias), pad 3, stride 1.
 * Replaces conv_dw + x.permute(0, 2, 3, 1) of timm's ConvNeXtBlock (the convnextv2_base backbone
 * of model.py:96-100).  x: device NCHW fp32 [n, c, h, w]; w: device [c, 1, 7, 7]; bias: device [c]
 * or NULL; y: device NHWC fp32 [n, h, w, c].
 */
int mirx_dwconv7x7_nchw_to_nhwc(const float *x, const float *w, const float *bias, int64_t n, int c, int h,
                                int wd, float *y, void *stream);
/* The same convolution on a channels-last map (the ConvNeXtV2 fast path keeps its residual stream NHWC): x, y = device NHWC fp32
 * [n, h, w, c] (y != x); w_taps_first = device [49][c] (conv_dw.weight.view(c, 49).t(), prepared once per layer); bias [c] or
 * NULL.  No LDS: a lane owns one channel and walks a strip of 3 output rows with a 7-column window in registers. */
int mirx_dwconv7x7_nhwc(const float *x, const float *w_taps_first, const float *bias, int64_t n, int c, int h, int wd, float *y,
                        void *stream);

/*
 * ResNet-50 on channels-last TERMS ROWS (layout: mirx_linear_terms above; image b of a map is n_pixels rows of c / 32 lines).
 * Every terms map travels with two device fp32 rows [n]: its SCALE row (the power of two image b was written with) and its
 * RANGE row (largest |value| of image b before the split, zeroed by the caller once per forward, folded in by unsigned atomic
 * max: mirx_device.h).  An image's arithmetic reads only its own rows, so its embedding does not depend on its batch mates and
 * a non-finite image makes only its own outputs NaN.  Replaces the torchvision Bottleneck convolutions the reference's
 * ResNet50 runs (model.py:9-39 there, models.resnet50 children [:-1]).
 *
 * mirx_conv_terms: y[b, oy, ox, o] = relu?( oscale[o] / x_scale[b] * sum_{ky, kx, c} x[b, s oy + ky - p, s ox + kx - p, c]
 *                  * W2[o, ky, kx, c] + bias[o] (+ res[b, oy, ox, o]) ),  p = (ksize - 1) / 2, ho = (h + 2 p - ksize) / s + 1
 *     as an implicit GEMM on two fp16 terms per operand (k_conv_t2.hip); padding taps read zeros.
 *     xt = terms rows [n, h, w, cin] with x_scale / x_range its scale and range rows; ksize 1 or 3, stride 1 or 2,
 *     cin and cout multiples of 32, any h and w.
 *     wt = terms rows of W2[o, :] = W[o, ky, kx, c] * ws[o] in K order (ky, kx, c) (W: conv weight with the eval BatchNorm
 *     folded in, ws a power of two per output channel putting max |W2[o, :]| in [2^13, 2^14)), rows padded with zeros to
 *     a multiple of 128; oscale = device fp32 [cout] = 1 / ws; bias = device fp32 [cout] (the folded BatchNorm shift).
 *     w_abs_sum = max_o sum |W[o, :]| and bias_abs_max = max |bias| (host constants of the layer).
 *     res_or_null = terms rows [n, ho, wo, cout] (the Bottleneck's identity or downsample branch) with its scale and
 *     range rows.  relu != 0: ReLU after the residual.
 *     Outputs (either or both): yt_or_null = terms rows [n, ho, wo, cout] of y_scale[b] * y, where
 *         y_scale[b] = 2^(14 - floor(log2 bound_b)),  bound_b = x_range[b] * w_abs_sum + bias_abs_max (+ res_range[b])
 *     (>= every |y| of the image; a function of rows complete before the launch, written into y_scale_or_null for the
 *     consumer); y_or_null = fp32 rows [n * ho * wo, cout].  out_range_or_null: range row of y.
 * mirx_nchw_to_terms: xt (terms rows [n, hw, c]) of the NCHW fp32 map x (images x_batch_stride floats apart: the stem's
 *     output, mirx_stem_conv7_bn_relu_pool_split2h_into / _u8_into) with image b scaled by 2^(14 - floor(log2 range_row[b]))
 *     (range_row = the stem's output range), written into scale_row[b].  c % 32 == 0.
 * mirx_gap_nhwc_l2norm: y[b, :] = mean over the hw pixels of x[b, p, :] (fp32 rows [n, hw, c], c % 4 == 0), then, with
 *     normalize, y[b] / max(||y[b]||_2, 1e-12): AdaptiveAvgPool2d(1) + flatten + F.normalize of the reference's ResNet50
 *     (model.py:26-38 there); the channels-last form of mirx_bn_relu_gap_l2norm without norm and ReLU.
 * Buffers 16-byte aligned.
 */
int mirx_conv_terms(const void *xt, const float *x_scale, const float *x_range, int64_t n, int h, int w, int cin, int ksize,
                    int stride, const void *wt, const float *oscale, const float *bias, int cout, float w_abs_sum,
                    float bias_abs_max, const void *res_or_null, const float *res_scale, const float *res_range, int relu,
                    void *yt_or_null, float *y_scale_or_null, float *y_or_null, float *out_range_or_null, void *stream);
int mirx_nchw_to_terms(const float *x, int64_t x_batch_stride, int64_t n, int c, int hw, const float *range_row,
                       float *scale_row, void *xt, void *stream);
int mirx_gap_nhwc_l2norm(const float *x, int64_t n, int hw, int c, int normalize, float *y, void *stream);

/*
 * SwinV2 (timm 0.9.7 swinv2_base_window12to24_192to384, the backbone of the reference's SwinV2, model.py:418-446 there) on
 * fp32 raster rows [n, side, side, c] (c = heads * head_dim).  Replace torch.roll + window_partition + WindowAttention +
 * window_reverse + roll back (one mirx_window_attention_split2h), `x + norm1(..)` / `x + norm2(..)` (mirx_swin_postnorm) and
 * PatchMerging's reshape / permute / flatten (mirx_patch_merge_terms) of SwinTransformerV2Block and its stages.
 *
 * mirx_window_attention_split2h: qkv = the qkv Linear's output rows [n * side * side, 3 c] (bias cat(q_bias, 0, v_bias) included;
 *     q, k, v of head h at columns h * 32, c + h * 32, 2 c + h * 32).  For every window of the map shifted by `shift` (token
 *     (ty, tx) of window (wy, wx) is pixel ((wy window + ty + shift) mod side, (wx window + tx + shift) mod side)):
 *         out[pixel(t), h * 32 + d] = sum_u softmax_u(cos(q_t, k_u) ls[h] + bias_table[h, rel(t, u)] + mask(t, u)) v_u[d],
 *     rel(t, u) = (ty - uy + window - 1) (2 window - 1) + (tx - ux + window - 1), mask = -100 where t and u lie in different
 *     regions of timm's shifted-window mask (slices [0, side - window), [side - window, side - shift), [side - shift, side) per
 *     axis; no mask for shift 0); cos from F.normalize(.., eps 1e-12) in fp32.  bias_table = device fp32 [heads, (2 window -
 *     1)^2] (16 sigmoid(cpb_mlp(relative_coords_table)) transposed); logit_scale = device fp32 [heads], exp(min(logit_scale,
 *     ln 100)).  Both GEMMs on two fp16 terms per operand (k_attention_win.hip); v staged at a power of two from the largest
 *     |v| of its own (image, window, head).  head_dim 32, window 12 or 24, side a multiple of window, 0 <= shift < window.
 *     Outputs (either or both): out_or_null fp32 rows [n * side * side, c]; out_terms_or_null terms rows (mirx_linear_terms) of
 *     out_scale * out.
 * mirx_swin_postnorm: out = x + LayerNorm(y) over rows of c (x_or_null NULL: out = LayerNorm(y)); out may be x, not y.  gamma,
 *     beta device [c].  out_terms_or_null: out also written as terms rows of terms_scale * out.  c % 32 == 0, c <= 1024.
 * mirx_patch_merge_terms: terms rows [n, h / 2, w / 2, 4 c] of scale * x, x = fp32 rows [n, h, w, c]: row (b, i, j) holds the
 *     pixels (2 i, 2 j), (2 i + 1, 2 j), (2 i, 2 j + 1), (2 i + 1, 2 j + 1) in that order (timm PatchMerging).  c % 8 == 0.
 * Buffers 16-byte aligned.
 */
int mirx_window_attention_split2h(const float *qkv, int64_t n, int side, int window, int shift, int heads, int head_dim,
                                  const float *bias_table, const float *logit_scale, float *out_or_null, void *out_terms_or_null,
                                  float out_scale, void *stream);
int mirx_swin_postnorm(const float *x_or_null, const float *y, int64_t m, int c, const float *gamma, const float *beta, float eps,
                       float *out, void *out_terms_or_null, float terms_scale, void *stream);
int mirx_patch_merge_terms(const float *x, int64_t n, int h, int w, int c, float scale, void *out_terms, void *stream);

/*
 * Attention-pooling heads of the reference's ConvNeXtV2_SRA / ConvNeXtV2_PCAM (model.py:120-278 there: SRA.forward and
 * PCAMPool.forward after convnext.forward_features) on the backbone's final channels-last residual stream x = fp32 rows
 * [n, hw, c] (image b's pixel p at row b * hw + p).  LN(v) = LayerNorm over c with device affine gamma, beta [c] and eps (the
 * shared convnext.head.norm).  One workgroup per image with one fixed reduction order, so an image's output bits depend only on
 * its own rows and the weights; non-finite rows reach only their own image's output.  fp32 arithmetic throughout.
 *
 * mirx_sra_head_nhwc: w_att device [K, c] (conv_att, no bias).
 *     g = LN(mean_p x[p]);  a[k, p] = softmax_p(w_att[k] . x[p]) (max-subtracted);  s = LN(sum_p ((1 / K) sum_k a[k, p]) x[p]);
 *     y[b] = g + lam s, divided by max(||.||_2, 1e-12) when normalize != 0 (F.normalize).
 * mirx_pcam_head_nhwc: w_cls device [K, c], b_cls device [K] (classifier).
 *     g = LN(mean_p x[p]);  z[p] = LN(x[p]);  q[k, p] = sigmoid(w_cls[k] . z[p] + b_cls[k]) / (sum_p sigmoid(..) + 1e-8);
 *     P[k] = sum_p q[k, p] z[p];  logit[k] = P[k] . w_cls[k] + b_cls[k];  feat[b] = g + lam sum_k softmax_k(logit)[k] P[k],
 *     normalised as above when normalize != 0 (the reference normalises after its optional fc: pass 0 when an fc follows).
 *     class_logits_or_null: device [n, K] <- logit.
 * Limits (MIRX_EINVAL with a message, nothing launched, outside them): c % 4 == 0, 4 <= c <= 8192; 1 <= K <= 64; hw >= 1 and
 * (K + 3) * hw <= 16384 (the per-pixel weights live in 64 KiB of LDS: K = 8 allows hw <= 1489, K = 64 allows hw <= 244);
 * n < 2^31; x, w, gamma, beta and the output 16-byte aligned.
 */
#define MIRX_ATTNPOOL_MAX_C 8192
#define MIRX_ATTNPOOL_MAX_K 64
#define MIRX_ATTNPOOL_LDS_FLOATS 16384
int mirx_sra_head_nhwc(const float *x, int64_t n, int hw, int c, const float *w_att, int K, const float *gamma, const float *beta,
                       float eps, float lam, int normalize, float *y, void *stream);
int mirx_pcam_head_nhwc(const float *x, int64_t n, int hw, int c, const float *w_cls, const float *b_cls, int K, const float *gamma,
                        const float *beta, float eps, float lam, int normalize, float *feat, float *class_logits_or_null,
                        void *stream);

/*
 * Binary-code retrieval of the reference's ATH path (test_ath.py / train_ath.py there: pairwise_distance on 0/1 codes + argsort).
 *
 * mirx_hamming_words: the words per packed row for `bits` (ceil(bits / 32) rounded up to a power of two: 1, 2, 4, ..., 32).
 * mirx_hamming_pack: src = device [rows, bits] contiguous, dtype MIRX_BITS_F32 (float32) or MIRX_BITS_U8 (uint8 / bool bytes) ->
 *     dst = device uint32 [rows, mirx_hamming_words(bits)], bit j of a row in bit j % 32 of word j / 32, padding bits 0.  Any value
 *     other than 0 or 1 (NaN included) stores 1 into the device int *bad_flag (which the caller zeroes first and reads after).
 * mirx_hamming_topk: exact top-k by Hamming distance of packed queries [nq, words] against packed rows [n, words]:
 *     ranking = (distance ascending, row ascending); exclude_or_null = device int64 [nq], that row never appears for that query.
 *     out_dist = device int32 [nq, k] distances, out_ids = device int64 [nq, k] rows; when fewer than k rows remain (an excluded row
 *     and k = n) the tail holds -1 in both.  The result is a function of the query, the rows, k and the exclusion alone (the same
 *     bits on every run and in every batch).  workspace = device, >= mirx_hamming_workspace_bytes(nq, n, bits, k) bytes, 16-byte
 *     aligned; its size is bounded by nq, n, k and bits, whatever the distances are.  Limits (MIRX_EINVAL, nothing launched):
 *     1 <= bits <= 1024, 1 <= k <= 1024, k <= n < 2^31, 0 <= nq <= 2^24; packed buffers 16-byte aligned.
 */
#define MIRX_HAMMING_MAX_BITS 1024
#define MIRX_HAMMING_MAX_K 1024
#define MIRX_HAMMING_MAX_Q (1 << 24)
#define MIRX_BITS_F32 0
#define MIRX_BITS_U8 1
int mirx_hamming_words(int bits);
int mirx_hamming_pack(const void *src, int dtype, int64_t rows, int bits, uint32_t *dst, int *bad_flag, void *stream);
int64_t mirx_hamming_workspace_bytes(int64_t nq, int64_t n, int bits, int k);
int mirx_hamming_topk(const uint32_t *q_packed, int64_t nq, const uint32_t *g_packed, int64_t n, int bits, int k,
                      const int64_t *exclude_or_null, void *workspace, int64_t workspace_bytes, int *out_dist, int64_t *out_ids,
                      void *stream);

/*
 * The forward of the reference's ATHNet (ath_model.py there) in fp32: x = device fp32 [n, 3, size, size] (NCHW) ->
 * hash_out [n, hash_size], logits_out [n, num_classes].  params = device fp32, the eval-mode BatchNorms folded into their
 * convolutions (w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)), at the offsets below (conv weights [out, in, 3, 3]):
 *     W11/B11 net1.0.net.0+1   W12/B12 net1.0.net.3+4   W1D/B1D net1.0.downsample   WSA sa.conv [1, 2, 3, 3]
 *     W21..B2D net2.0 (16 -> 8)   W31..B3D dense (8 -> 1)
 *     HEADS: hashlayer.weight [hash_size, f], hashlayer.bias, typelayer.weight [num_classes, f], typelayer.bias; f = (size / 8)^2.
 * Each output is a fixed-order fp32 sum over its own image (k_ath.hip), so an image's bits do not depend on its batch mates.
 * workspace = device fp32, >= mirx_ath_workspace_floats(n, size).  Limits (MIRX_EINVAL, nothing launched): size % 8 == 0,
 * 8 <= size <= 1024, n <= 65536, hash_size, num_classes >= 1; x, params, workspace 16-byte aligned.
 */
#define MIRX_ATH_MAX_SIZE 1024
#define MIRX_ATH_MAX_BATCH 65536
#define MIRX_ATH_P_W11 0
#define MIRX_ATH_P_B11 432
#define MIRX_ATH_P_W12 448
#define MIRX_ATH_P_B12 2752
#define MIRX_ATH_P_W1D 2768
#define MIRX_ATH_P_B1D 3200
#define MIRX_ATH_P_WSA 3216
#define MIRX_ATH_P_W21 3234
#define MIRX_ATH_P_B21 4386
#define MIRX_ATH_P_W22 4394
#define MIRX_ATH_P_B22 4970
#define MIRX_ATH_P_W2D 4978
#define MIRX_ATH_P_B2D 6130
#define MIRX_ATH_P_W31 6138
#define MIRX_ATH_P_B31 6210
#define MIRX_ATH_P_W32 6211
#define MIRX_ATH_P_B32 6220
#define MIRX_ATH_P_W3D 6221
#define MIRX_ATH_P_B3D 6293
#define MIRX_ATH_P_HEADS 6296
int64_t mirx_ath_workspace_floats(int64_t n, int size);
int mirx_ath_forward(const float *x, int64_t n, int size, const float *params, int hash_size, int num_classes, float *workspace,
                     int64_t workspace_floats, float *hash_out, float *logits_out, void *stream);

/* ---- SimCAM similarity saliency (k_simcam.hip) -------------------------------------------------------------------------
 * The reference's explanations.py SimCAM / SimCAM_MedSigLIP / SimCAM_Densenet121 on channels-last fp32 token rows.
 * q: [h * w, c] query rows; r: P retrieved row blocks, block p at r + p * pair_stride, each [h * w, c] (row-major, any c).
 * Per pair D_p = q r_p^T in f32 (a fixed-order reduction on the f32 matrix pipe), s_p = max(D_p) + eps (NaN kept),
 *   map 0 (query)     decom_1[i] = sum_j relu(D_p[i, j] / s_p)
 *   map 1 (retrieved) decom_2[j] = sum_i relu(D_p[i, j] / s_p), or with point != NULL (double[2], point[0] along H) the
 *                     reference's Point_Specific: the bilinear blend of the rows relu(D_p[i*, :] / s_p) at the point on the
 *                     replicate-padded query grid, clamped at 0,
 * each bilinearly upsampled to H x W (align_corners=False) into out: maps = MIRX_SIMCAM_MAPS_BOTH -> [P, 2, H, W] (map 0, map 1),
 * MIRX_SIMCAM_MAPS_RETRIEVED -> [P, H, W] (map 1).  s_p == 0 or a NaN in D_p gives NaN maps for pair p only.  Every output of
 * pair p is a fixed-order function of q and r_p: bit-identical whatever P is.
 * workspace = device fp32, >= mirx_simcam_workspace_floats(P, h * w).  Limits (MIRX_EINVAL, nothing launched): 1 <= h * w <= 1024,
 * 1 <= c <= 16384, 0 <= P <= 65535, pair_stride >= h * w * c, 1 <= H, W <= 8192, eps finite >= 0, point inside [0, H) x [0, W).
 *
 * mirx_bn_relu_rows: out[b, i, ch] = relu(x[b, ch, i] * scale[ch] + shift[ch]) -- an NCHW map [b, c, hw] as channels-last rows.
 */
#define MIRX_SIMCAM_MAX_HW 1024
#define MIRX_SIMCAM_MAX_C 16384
#define MIRX_SIMCAM_MAX_PAIRS 65535
#define MIRX_SIMCAM_MAX_SIZE 8192
#define MIRX_SIMCAM_MAPS_BOTH 0
#define MIRX_SIMCAM_MAPS_RETRIEVED 1
int64_t mirx_simcam_workspace_floats(int64_t pairs, int64_t hw);
int mirx_simcam(const float *q, const float *r, int64_t pairs, int64_t pair_stride, int h, int w, int64_t c, float eps, int maps,
                const double *point, int H, int W, float *workspace, int64_t workspace_floats, float *out, void *stream);
int mirx_bn_relu_rows(const float *x, int64_t b, int64_t c, int64_t hw, const float *scale, const float *shift, float *out,
                      void *stream);

/* ---- Attention rollout (k_rollout.hip) ---------------------------------------------------------------------------------
 * The reference's explanations.py AttentionRolloutMedSigLIP, from the packed qkv [b, n, 3c] (q | k | v, c = heads * head_dim,
 * head h at columns h * head_dim) of each encoder layer.
 * mirx_rollout_layer: A_l[b] = normalise(discard(fuse_h softmax((q_h k_h^T) * scale)) + I) into workspace slot `layer`:
 *   scores in f32 on the matrix pipe (fixed-order reductions), the exact softmax per row, the heads fused in ascending order
 *   (fusion: MIRX_ROLLOUT_FUSE_MEAN sum / heads, _MAX, _MIN; NaN kept; up to 4 splits of consecutive heads, a function of
 *   the head count alone, combined in split order), then the row stage of mirx_rollout_rows.
 * mirx_rollout_rows: in place on a [rows, n] fp32 matrix, per row: k > 0 -> thr = the k-th smallest value, a = a * (a > thr)
 *   (ties at thr dropped); then a[row % n] += 1 and a = a / (sum(a) + 1e-8).  k = 0: no discard.
 * mirx_rollout_finish: v = 1/n, v <- v^T A_l for l = layers - 1 .. 0 (fixed order), v *= clamp(patches[b, j] . query, 0) when
 *   patches ([b, n, e]) and query ([e]) are given (both or neither), then the h x w map (n = h * w) bilinearly upsampled
 *   (align_corners=False) into out [b, H, W].  It reads the `layers` slots mirx_rollout_layer filled.
 * Every output of image b is a fixed-order function of image b's inputs alone: bit-identical whatever b is.  A NaN in image b's
 * qkv makes its map NaN.  workspace = device fp32, >= mirx_rollout_workspace_floats(layers, b, n) ((layers + 4) b n^2 + 17 b n).
 * Limits (MIRX_EINVAL, nothing launched): 1 <= layers <= 256, 0 <= b <= 65535, 1 <= n <= 1024, 1 <= heads <= 256,
 * head_dim % 4 == 0 in [4, 128], 0 <= k <= n, scale finite, qkv 16-byte aligned, 0 <= rows <= 2^26, 1 <= H, W <= 8192,
 * 1 <= e <= 65536.
 */
#define MIRX_ROLLOUT_MAX_N 1024
#define MIRX_ROLLOUT_MAX_HEAD_DIM 128
#define MIRX_ROLLOUT_MAX_HEADS 256
#define MIRX_ROLLOUT_MAX_LAYERS 256
#define MIRX_ROLLOUT_MAX_IMAGES 65535
#define MIRX_ROLLOUT_MAX_ROWS (1LL << 26)
#define MIRX_ROLLOUT_MAX_SIZE 8192
#define MIRX_ROLLOUT_MAX_EMBED 65536
#define MIRX_ROLLOUT_FUSE_MEAN 0
#define MIRX_ROLLOUT_FUSE_MAX 1
#define MIRX_ROLLOUT_FUSE_MIN 2
int64_t mirx_rollout_workspace_floats(int layers, int64_t b, int64_t n);
int mirx_rollout_layer(const float *qkv, int64_t b, int n, int heads, int head_dim, float scale, int fusion, int k, int layer, int layers,
                       float *workspace, int64_t workspace_floats, void *stream);
int mirx_rollout_rows(float *a, int64_t rows, int n, int k, void *stream);
int mirx_rollout_finish(float *workspace, int64_t workspace_floats, int layers, int64_t b, int h, int w, const float *patches,
                        const float *query, int64_t e, int H, int W, float *out, void *stream);

/* ---- Grad-CAM retrieval saliency (k_gradcam.hip) ------------------------------------------------------------------------
 * The reference's medsiglip_saliency.py _compute_single_gradcam for a SigLIP tower, from the last encoder layer's tokens
 * x [b, n, d] (before post_layernorm, LayerNorm gamma / beta / eps), heads of width d / heads; see DESIGN 21.
 * mirx_gradcam_pool: y = LN(x); S[t, h] = y_t . u[h] + c[h] (u [heads, d], c [heads]: the probe query folded into the keys);
 *   P = softmax over t per head (exact, NaN kept); ybar [b, heads, d] = sum_t P[t, h] y_t.  Stats and P stay in the workspace.
 * mirx_gradcam_tokens: dP[t, h] = y_t . w[b, h] + e[b, h] (w [b, heads, d], e [b, heads]: the gradient at the value
 *   projection), dS = P (dP - sum_t P dP), g_y = sum_h dS u_h + P w_h, the LayerNorm backward g_x, summed over blocks of
 *   MIRX_GRADCAM_TOKENS_PER_BLOCK tokens into the workspace.  Needs the workspace mirx_gradcam_pool filled.
 * mirx_gradcam_finish: wbar = (1/n) sum_t g_x[t] (block partials in order), cam_t = relu(x_t . wbar), the sqrt(n)^2 grid
 *   bilinearly upsampled (align_corners=False, ATen's source index) into out [b, H, W], then per image numpy's float32 rule:
 *   max - min > 1e-8 -> (v - min) / (max - min), else 0.  A NaN anywhere in an image's map therefore gives it an all-zero map.
 * mirx_gradcam_gemv: out[i * os + j] = sum_t A[(j % rmod) * lda + (j / mg) * acol + t] * x[i * xs + (j / mg) * xg + t]
 *   (+ bias[j]) (+ res[i * rs + j]), t < k, j < m, i < b (plain GEMV: mg = rmod = m); a wave per output.
 * mirx_gradcam_layernorm: rows of len, out = LN(v) (relu != 0: then ReLU, NaN kept), stats [b, 2] = (mean, 1 / std).
 * mirx_gradcam_layernorm_bwd: out = LN backward of g (times (after > 0) when after is given) (+ res), from v and stats.
 * mirx_gradcam_gelu: mode 0 out = tanh-GELU(h); mode 1 out = g * tanh-GELU'(h), as ATen writes both.
 * mirx_gradcam_cosine_bwd: out [b, e] = d/dp sum_r cosine_similarity(normalize(p), q_r) for q [bq, e].
 * Every output of image b is a fixed-order function of image b's inputs alone (no atomics): bit-identical whatever b is and
 * however the images are chunked.  workspace = device fp32, >= mirx_gradcam_workspace_floats(b, n, d, heads).
 * Workspace of one image, in floats and in this order (image i's slot starts at i times the total):
 *   stats [2 n] (mean, 1 / std per token) | P [n * heads] | dP [n * heads] | dsum [16] (sum_t P dP per head) |
 *   partials [ceil(n / 4) * d] (the column sum of g_x per block of MIRX_GRADCAM_TOKENS_PER_BLOCK tokens) | wbar [d] | cam [n] |
 *   minmax [1024] (a (min, max) pair per 16 output rows); the total is rounded up to a multiple of 4.
 *   pool writes stats and P; tokens reads them and writes dP, dsum and partials; finish reads partials and writes the rest.
 * Limits (MIRX_EINVAL, nothing launched): 0 <= b <= 65535, 1 <= n <= 1024 (a square for finish), 1 <= heads <= 16,
 * 1 <= d <= 8192 with d % heads == 0, eps finite >= 0, buffers 4-byte aligned, 1 <= H, W <= 8192, 1 <= len, e <= 8192,
 * 1 <= bq <= 65535, gemv m, k, mg, rmod >= 1 and strides >= 0.
 */
#define MIRX_GRADCAM_MAX_N 1024
#define MIRX_GRADCAM_MAX_HEADS 16
#define MIRX_GRADCAM_MAX_WIDTH 8192
#define MIRX_GRADCAM_MAX_IMAGES 65535
#define MIRX_GRADCAM_MAX_SIZE 8192
#define MIRX_GRADCAM_MAX_EMBED 8192
#define MIRX_GRADCAM_TOKENS_PER_BLOCK 4
int64_t mirx_gradcam_workspace_floats(int64_t b, int n, int d, int heads);
int mirx_gradcam_pool(const float *x, int64_t b, int n, int d, int heads, const float *gamma, const float *beta, float eps, const float *u,
                      const float *c, float *workspace, int64_t workspace_floats, float *ybar, void *stream);
int mirx_gradcam_tokens(const float *x, int64_t b, int n, int d, int heads, const float *gamma, const float *beta, const float *u,
                        const float *w, const float *e, float *workspace, int64_t workspace_floats, void *stream);
int mirx_gradcam_finish(const float *x, int64_t b, int n, int d, int heads, float *workspace, int64_t workspace_floats, int H, int W,
                        float *out, void *stream);
int mirx_gradcam_gemv(const float *A, int64_t lda, const float *x, int64_t xs, const float *bias, const float *res, int64_t rs, float *out,
                      int64_t os, int64_t b, int m, int k, int mg, int rmod, int64_t acol, int64_t xg, void *stream);
int mirx_gradcam_layernorm(const float *v, int64_t b, int len, const float *gamma, const float *beta, float eps, int relu, float *out,
                           float *stats, void *stream);
int mirx_gradcam_layernorm_bwd(const float *g, const float *after, const float *v, const float *stats, const float *gamma, int64_t b,
                               int len, const float *res, float *out, void *stream);
int mirx_gradcam_gelu(const float *h, const float *g, int64_t count, int mode, float *out, void *stream);
int mirx_gradcam_cosine_bwd(const float *p, int64_t b, int e, const float *q, int64_t bq, float *out, void *stream);

/* ---- ChestMIR lesion-aware re-ranking (k_rerank.hip) -------------------------------------------------------------------
 * The reference's ChestMIR/chestmir_eval.py rerank_with_specific_lesion / rerank_with_adaptive_lesion for every stage of a
 * dataset in one launch (grid: query x stage); see DESIGN 22.
 * base_ids: device [n, n] int64, row q = the full base ranking of query q (mirx_index_rank_all with the query excluded: q
 *   itself last).  Base score of (q, id): base_sim_or_null[q * n + id] (device fp64 [n, n]) when given, otherwise the fp64 dot
 *   of rows q and id of gvec_or_null (device fp32 [n, d]).
 * Region store, a CSR over images: row_ptr [n + 1] int64, region_lesion [n_regions] int32 (index into the caller's lesion
 *   name list), region_vec [n_regions, dr] fp32, the regions of an image in stored order.
 * q_lesion [n_stages, n] int32 and q_region [n_stages, n] int64: per (stage, query) the lesion to match and the region index
 *   of the query vector (-1, or anything outside the store: no vector).
 * For each (stage s, query q): every one of the first topk ids c of the base row gets region = max over c's regions of that
 *   lesion of <q vector, region> (fp64; -1.0 without such a region) and combined = global_weight * base + (1 - global_weight)
 *   * region; out_matched[s, q] = number of candidates with region >= 0.  Without a query vector or with out_matched == 0 the
 *   base row is copied and out_reranked[s, q] = 0; otherwise the first topk ids are sorted on (combined desc, base desc, base
 *   position asc), the rest of the base row follows unchanged, and out_reranked[s, q] = 1.
 * out_ids: device [n_stages, n, n] int64, so that stage s is the ranks argument of mirx_rank_metrics at out_ids + s * n * n
 *   with row_stride n (or all stages at once with nq = n_stages * n).
 * All sums run in a fixed order (k_rerank.hip): a result does not depend on n_stages, on the other stages or on other queries.
 * Limits (MIRX_EINVAL, nothing launched): 2 <= n <= 65536, 1 <= dr <= 4096, 1 <= topk <= min(1024, n - 1),
 * 0 <= n_stages <= 65535, 0 <= global_weight <= 1, 0 <= n_regions < 2^31, 1 <= d <= 65536 when base_sim is null, 8-byte
 * aligned int64 / fp64 buffers, 4-byte aligned int32 / fp32 buffers.  The region store may be null when n_regions == 0.
 */
#define MIRX_RERANK_MAX_N 65536
#define MIRX_RERANK_MAX_DR 4096
#define MIRX_RERANK_MAX_D 65536
#define MIRX_RERANK_MAX_TOPK 1024
#define MIRX_RERANK_MAX_STAGES 65535
#define MIRX_RERANK_MAX_REGIONS 2147483647
int mirx_lesion_rerank(const int64_t *base_ids, int64_t n, const double *base_sim_or_null, const float *gvec_or_null, int d,
                       const int64_t *row_ptr, const int32_t *region_lesion, const float *region_vec, int64_t n_regions, int dr,
                       const int32_t *q_lesion, const int64_t *q_region, int n_stages, int topk, double global_weight, int64_t *out_ids,
                       int32_t *out_matched, int32_t *out_reranked, void *stream);

/* ---- SimAtt similarity-attention saliency (k_simatt.hip) ---------------------------------------------------------------
 * The reference's explanations.py SimAtt in closed form for a model whose tail after the target feature map is
 * average pool -> optional fc.  rows: device fp32 [b, h * w, c], the channels-last rows of that map, image 0 the query.
 * fc_weight [d, c] / fc_bias [d] (row-major; bias may be null); no fc: fc_weight = fc_bias = null and d = 0 (the embedding is
 * the pooled vector, width c).  With x_i = fc(mean over positions of rows[i]) and xn_i = x_i / max(|x_i|, 1e-12):
 *   wt[e]   = product over the non-query images j of |xn_0[e] - xn_j[e]|, the FIRST factor replaced by 1 - itself when
 *             positive = 1
 *   g_i[ch] = sum_e W[e, ch] * sign(x_i[e]) * wt[e] / (h * w)        (W = identity without fc, sign(0) = 0)
 *   map_i   = relu(sum_ch g_i[ch] * rows[i, :, ch]) as an h x w grid, bilinearly upsampled (align_corners=False) to H x W
 * mode MIRX_SIMATT_GROUP: one wt over the images 1 .. b - 1; out [b, H, W].
 * mode MIRX_SIMATT_PAIRS: retrieval k = image k + 1 alone against the query (wt_k has the single factor of image k + 1, flipped
 *   when positive = 1); out [b - 1, 2, H, W]: the query's map under pair k, then retrieval k's.
 * Two launches whatever b is, no host synchronisation.  Every sum runs in an order fixed by h * w, c and d: x_i depends on image
 * i only and a pairs-mode map on the query and its retrieval only, bit-identical whatever b is.  relu keeps NaN; a NaN in image j
 * makes every map NaN in group mode and pair j - 1's two maps (every pair's when j = 0) in pairs mode.
 * Cost: pairs mode is linear in b.  In group mode every map's workgroup rebuilds the b norms and wt itself (two launches, no
 * hand-off between workgroups), b * b * d operations in all: nothing at the handful of images the explainer is called with, an
 * estimated several seconds of one launch at b = 65535 with d = 16384 (not measured).  Use pairs mode for large batches.
 * workspace = device fp32, >= mirx_simatt_workspace_floats(b, c, d, mode).  Limits (MIRX_EINVAL, nothing launched):
 * 1 <= h * w <= 1024, 1 <= c <= 16384, 1 <= d <= 16384 (or 0: no fc), 2 <= b <= 65535, 1 <= H, W <= 8192, positive 0 or 1.
 */
#define MIRX_SIMATT_MAX_HW 1024
#define MIRX_SIMATT_MAX_C 16384
#define MIRX_SIMATT_MAX_D 16384
#define MIRX_SIMATT_MAX_B 65535
#define MIRX_SIMATT_MAX_SIZE 8192
#define MIRX_SIMATT_GROUP 0
#define MIRX_SIMATT_PAIRS 1
int64_t mirx_simatt_workspace_floats(int64_t b, int64_t c, int64_t d, int mode);
int mirx_simatt(const float *rows, int64_t b, int h, int w, int64_t c, const float *fc_weight, const float *fc_bias, int64_t d,
                int mode, int positive, int H, int W, float *workspace, int64_t workspace_floats, float *out, void *stream);

/* ---- Anomaly evaluation (k_anomaly.hip) --------------------------------------------------------------------------------
 * The reference's anomaly/test_anomaly.py + anomaly/anomaly.py on the device: class centroids of an embedding set,
 * every row's distance to its nearest centroid, and the binary ranking measures and curve points of score segments.
 *
 * mirx_class_centroids: rows = device fp32 [n, d], labels = device int64 [n], classes = HOST int64 [k] (read during the call).
 *   centroids = device fp64 [k, d]: the mean of the rows whose label is classes[j] (the first such j when classes repeat a value;
 *   rows whose label is in no class are left out), counts = device int64 [k].  Sums are fp64, added per chunk of consecutive rows
 *   in row order and then in chunk order; the chunking depends on n and d alone and there is no floating atomic, so the bits are
 *   the same on every call.  The mean is NOT rounded to fp32.  A class without rows gives a NaN centroid, count 0 and
 *   MIRX_ANOMALY_BAD_EMPTY_CLASS in *bad_flag.  workspace = device, >= mirx_class_centroids_workspace_bytes(n, d, k), 256-byte
 *   aligned.
 * mirx_centroid_min_dist: dist[i] = min over j of sqrt(sum_e (rows[i, e] - centroids[j, e])^2) in fp64 (device fp64 [n]),
 *   nearest[i] = the lowest j that attains it (device int32 [n]), max_out = device fp64 [1], the largest dist.  A NaN in row i
 *   or in ANY centroid makes dist[i] NaN (nearest[i] = the first class whose distance is NaN) and max_out NaN: a NaN class is
 *   never skipped in favour of a finite minimum.  The result does not depend on launch order or batch size.
 * mirx_binary_rank_metrics: scores = device fp64 [s, n], positive = device uint8 [s, n] (non-zero = positive); norm_or_null =
 *   device fp64 [s], segment i is ranked on scores / norm[i] (null: on the scores).  Per segment, with the distinct scores in
 *   descending order: out_t[i] = T, their number, thresholds[i, 0..T) the values ranked on (score / norm[i] when a norm is
 *   given, -0.0 as +0.0), tps / fps[i, 0..T) the positives / negatives
 *   at or above each (device fp64 / int64 / int64 [s, n], the tail past T is not written); out_auroc = the trapezoid area under
 *   (fps, tps) from (0, 0), an int64 sum divided once by 2 P Nneg; out_aupr = sum over t of (tps[t] - tps[t - 1]) / P *
 *   tps[t] / (tps[t] + fps[t]); out_fpr = fps[c] / Nneg at the record c <= (the first with tps == P) whose |tps / P -
 *   recall_level| is smallest, the later one on a tie (the reference's fpr_and_fdr_at_recall).  Every output is a function of the
 *   groups of equal scores: nothing depends on the order of equal scores, and a segment's outputs do not depend on s.
 *   workspace = device, >= mirx_binary_rank_metrics_workspace_bytes(s, n), 256-byte aligned.
 * *bad_flag (device int, zeroed by the caller, read after): the OR of MIRX_ANOMALY_BAD_SCORE (a NaN or infinite score),
 *   _BAD_NORM (a norm that is 0, negative, NaN or infinite), _BAD_ONE_CLASS (a segment without positives or without negatives:
 *   its three measures are NaN), _BAD_EMPTY_CLASS.  A flagged call still completes.
 * One stream, no host synchronisation.  Limits (MIRX_EINVAL, nothing launched): 1 <= n <= 2^30, 1 <= s <= 65535, 1 <= k <= 64,
 * 1 <= d <= 16384, recall_level in [0, 1], 8-byte aligned int64 / fp64 buffers, 4-byte aligned fp32 / int32 buffers.
 */
#define MIRX_ANOMALY_MAX_N (1LL << 30)
#define MIRX_ANOMALY_MAX_SEGMENTS 65535
#define MIRX_ANOMALY_MAX_K 64
#define MIRX_ANOMALY_MAX_D 16384
#define MIRX_ANOMALY_BAD_SCORE 1
#define MIRX_ANOMALY_BAD_NORM 2
#define MIRX_ANOMALY_BAD_ONE_CLASS 4
#define MIRX_ANOMALY_BAD_EMPTY_CLASS 8
int64_t mirx_class_centroids_workspace_bytes(int64_t n, int d, int k);
int mirx_class_centroids(const float *rows, int64_t n, int d, const int64_t *labels, const int64_t *classes, int k, void *workspace,
                         int64_t workspace_bytes, double *centroids, int64_t *counts, int *bad_flag, void *stream);
int mirx_centroid_min_dist(const float *rows, int64_t n, int d, const double *centroids, int k, double *dist, int32_t *nearest,
                           double *max_out, void *stream);
int64_t mirx_binary_rank_metrics_workspace_bytes(int64_t s, int64_t n);
int mirx_binary_rank_metrics(const double *scores, const uint8_t *positive, int64_t s, int64_t n, const double *norm_or_null,
                             double recall_level, void *workspace, int64_t workspace_bytes, double *thresholds, int64_t *tps,
                             int64_t *fps, int64_t *out_t, double *out_auroc, double *out_aupr, double *out_fpr, int *bad_flag,
                             void *stream);

/* ---- Insertion / deletion curves (k_insdel.hip) ---------------------------------------------------------------------------
 * The insertion / deletion game of the reference's drivers (evaluation.py CausalMetric, evaluate_saliency.py InsDel) with every
 * curve of one query as one device job.  A job has n_curves curves of n_steps + 1 images each; flat image g is step
 * s = g % (n_steps + 1) of curve j = g / (n_steps + 1).
 *
 * mirx_insdel_steps: sal = device fp32 [k, hw] -> t = device int32 [k, hw], t[p] = rank(p) / step, where rank is the position
 *   of p in np.flip(np.argsort(sal_k, kind="stable")): saliency descending, equal values by DESCENDING flat index, -0.0 equal to
 *   +0.0, every NaN before +inf.  A segmented stable radix sort (k_ranksort.hip) on a 32-bit key; workspace = device, >=
 *   mirx_insdel_steps_workspace_bytes(k, hw), 256-byte aligned.  Limits: 1 <= hw <= 2^20, 1 <= step, 1 <= k <= 65535.
 * mirx_blur2d_same: y[n, c, h, w] = the zero-padded cross-correlation of every plane of x with kernel [klen, klen] (device fp32),
 *   padding klen / 2 -- F.conv2d(x, gkern(klen, nsig), padding=klen // 2) without the zero off-diagonal channel blocks.  Taps are
 *   added in (ky, kx) order in fp64 and rounded once: a pixel's bits depend on its plane alone.  The kernel need not be separable.
 *   x and y must not overlap.  Limits: klen odd, 1 <= klen <= 63; 1 <= h, w <= 16384; 0 <= n * c; at most 2^31 - 1 workgroups
 *   (n * c * ceil(h / 32) * ceil(w / 32)).
 * mirx_insdel_compose: images [g0, g0 + n) of the job -> out = device fp32 [n, 3, hw]:
 *     out[c, p] = t[row[j]][p] < s ? bank[finish[j]][c, p] : bank[start[j]][c, p]
 *   t = device int32 [n_rows, hw], bank = device fp32 [n_bank, 3, hw], start / finish / row = device int32 [n_curves]; a bank index
 *   of -1 is the all-zero image.  A select on the 32-bit patterns: no arithmetic, a NaN payload passes through.  16-byte loads and
 *   stores when hw % 4 == 0 and t, bank and out are 16-byte aligned.  A chunk may span curves.  An index outside [-1, n_bank) or a
 *   row outside [0, n_rows) gives the all-zero image (nothing is read out of bounds).  Limits: 1 <= hw <= 2^20, n_rows, n_bank,
 *   n_curves >= 1, 1 <= n_steps <= 2^20, 0 <= g0, 0 <= n, g0 + n <= n_curves * (n_steps + 1).
 * mirx_insdel_curves: q_feat = device fp32 [1, d], r_feats = device fp32 [n_curves * (n_steps + 1), d].  Per curve: scores =
 *   device fp64 [n_curves, n_steps + 1], the cosine in fp64 of the fp32 rows with each norm clamped at 1e-8 (F.cosine_similarity);
 *   negative values are counted in zero_counter (device int64 [n_curves]) and set to 0, values above 1 and NaNs are kept
 *   (single_run's rule); auc = (sum of scores - scores[0] / 2 - scores[n_steps] / 2) / n_steps, summed in index order (device fp64
 *   [n_curves]).  Limits: 1 <= d <= 2^20, 1 <= n_curves, 1 <= n_steps, n_curves * (n_steps + 1) <= 2^30.
 * One stream, no host synchronisation, no floating atomic.  Outside the limits: MIRX_EINVAL with a message, nothing launched.
 */
#define MIRX_INSDEL_MAX_HW (1 << 20)
#define MIRX_INSDEL_MAX_K 65535
#define MIRX_BLUR_MAX_KLEN 63
int64_t mirx_insdel_steps_workspace_bytes(int64_t k, int64_t hw);
int mirx_insdel_steps(const float *sal, int64_t k, int64_t hw, int64_t step, void *workspace, int64_t workspace_bytes, int32_t *t,
                      void *stream);
int mirx_blur2d_same(const float *x, int64_t n, int c, int h, int w, const float *kernel, int klen, float *y, void *stream);
int mirx_insdel_compose(const int32_t *t, int64_t n_rows, int64_t hw, const float *bank, int64_t n_bank, const int32_t *start,
                        const int32_t *finish, const int32_t *row, int64_t n_curves, int64_t n_steps, int64_t g0, int64_t n,
                        float *out, void *stream);
int mirx_insdel_curves(const float *q_feat, const float *r_feats, int64_t n_curves, int64_t n_steps, int d, double *scores,
                       double *auc, int64_t *zero_counter, void *stream);

/* ---- SBSM occlusion saliency without materialised masks (k_sbsm.hip) ---------------------------------------------------------
 * The sliding-window occlusion saliency of the reference's drivers (explanations.py SBSMBatch, `--explainer sbsm`).
 * A window set is two device int32 arrays of clipped half-open intervals, row_iv [nr, 2] and col_iv [nc, 2]: mask n = i * nc + j
 * zeroes the pixels row_iv[i] x col_iv[j] and keeps the rest, N = nr * nc masks.  A job applies every mask to each of b images;
 * its flat image g = n * b + k is mask n on image k (the reference's stack order).  The interval arrays stay on the device and
 * the entry points never read them: an interval is expected inside the image and non-empty (mirx.sbsm.check_intervals verifies
 * that on the host), and the kernels only compare coordinates against them, so any content stays in bounds.
 *
 * mirx_sbsm_compose: x = device fp32 [b, c, h, w] -> out = device fp32 [n, c, h, w], images [g0, g0 + n) of the job.  Every value
 *   is the IEEE product x * (inside ? 0.0f : 1.0f): the bits of torch's mask.float() * x, including -0.0 and the NaN of inf * 0.
 *   16-byte loads and stores when c * h * w % 4 == 0 and x and out are 16-byte aligned, single floats otherwise (h * w odd).
 *   x and out must not overlap.  n = 0 launches nothing.  Limits: 1 <= h * w <= 2^20, c * h * w <= 2^30, 1 <= b, 1 <= nr, nc <=
 *   4096, 0 <= g0, 0 <= n < 2^31, g0 + n <= nr * nc * b.
 * mirx_sbsm_gain: e_q = device fp32 [q, d], e_m = device fp32 [n_masks * b, d] (row n * b + k), e_r = device fp32 [b, d] or null
 *   -> gain = device fp64 [rows, n_masks].
 *     e_r null (self-similarity, needs q == b; rows = b):   gain[k, n] = |e_q[k] - e_m[n * b + k]|
 *     otherwise (pairs; rows = q * b):          gain[p * b + k, n] = max(|e_q[p] - e_m[n * b + k]| - |e_q[p] - e_r[k]|, 0)
 *   |.| is the Euclidean norm; differences, squares, sums and the root are fp64 (one wave per value: lane-strided fma, then the
 *   butterfly of the other kernels).  The clamp keeps a NaN, like torch's clamp(min=0).  Limits: 1 <= d <= 16384, 1 <= q, b,
 *   n_masks, rows * n_masks <= 2^30, n_masks * b <= 2^30.
 * mirx_sbsm_accumulate: gain = device fp64 [rows, nr * nc] -> sal = device fp32 [rows, h, w]:
 *     sal[r, y, x] = fp32((sum over i with y in row_iv[i] of sum over j with x in col_iv[j] of gain[r, i * nc + j]) / (cr[y] * cc[x]))
 *   cr[y] / cc[x] = the number of row / column intervals that hold y / x: the weighted_avg of the reference.  A pixel no window
 *   covers is 0 / 0 = NaN, as there.  fp64 sums in a fixed order: per (r, i) the columns j ascending into the workspace [rows,
 *   nr, w], then the rows i ascending; one division, one rounding.  A gain is added where its window covers and not touched where
 *   it does not (the reference multiplies by 0 there, which spreads a non-finite gain over the whole map).  workspace = device,
 *   >= mirx_sbsm_workspace_bytes(rows, nr, w), 8-byte aligned.  Limits: 1 <= h * w <= 2^20, 1 <= nr, nc <= 4096, 1 <= rows,
 *   rows * nr * nc <= 2^30, nr * w <= 2^30, rows * nr * w <= 2^40.
 * One stream, no host synchronisation, no atomic: repeated calls are bit-identical.  Outside the limits: MIRX_EINVAL with a
 * message, nothing launched.
 */
#define MIRX_SBSM_MAX_HW (1 << 20)
#define MIRX_SBSM_MAX_WINDOWS 4096 /* nr and nc, each */
#define MIRX_SBSM_MAX_D 16384
int mirx_sbsm_compose(const float *x, int64_t b, int c, int h, int w, const int32_t *row_iv, int nr, const int32_t *col_iv, int nc,
                      int64_t g0, int64_t n, float *out, void *stream);
int mirx_sbsm_gain(const float *e_q, int64_t q, const float *e_m, int64_t n_masks, int64_t b, const float *e_r_or_null, int d,
                   double *gain, void *stream);
int64_t mirx_sbsm_workspace_bytes(int64_t rows, int nr, int w);
int mirx_sbsm_accumulate(const double *gain, int64_t rows, const int32_t *row_iv, int nr, const int32_t *col_iv, int nc, int h, int w,
                         void *workspace, int64_t workspace_bytes, float *sal, void *stream);

/* ---- Batched Resize + CenterCrop of 8-bit images (k_resample.hip) ---------------------------------------------------------------
 * The transforms.Resize(int) + CenterCrop of the reference's inference transforms on PIL images, as they come out of Pillow's
 * BILINEAR for 8-bit images, to the bit: milvus/milvus_retrieval.py:176-198, test.py:1286-1332,
 * ingest_embeddings.py:112-122, nih_multilabel_retrieval.py:64-66 (mirx.retriever.default_transform restates them on the host;
 * mirx.preprocess drives these entry points).  Tested for sources that are "RGB" (3 interleaved channels) or "L" (1 channel,
 * written to all three planes); nothing is claimed for other modes.
 *
 * One axis, resized from in_size to out_size pixels: scale = in_size / out_size, fs = max(scale, 1); output i has the taps
 * [xmin, xmax) = [max(0, (int)(c - fs + 0.5)), min(in_size, (int)(c + fs + 0.5))) around c = (i + 0.5) * scale, weights
 * max(0, 1 - |(x - c + 0.5) * (1 / fs)|) summed in tap order and divided by the sum (double), coefficients (int)(w * 2^22 + 0.5);
 * out = clip((2^21 + sum pixel * coeff) >> 22, 0, 255) in 32-bit integers.  Horizontal pass first into 8 bits, then vertical.
 *
 * mirx_resample_taps: the coefficient slots per output of such an axis, (int)ceil(fs) * 2 + 1.  Host only, no HIP call.
 * mirx_resample_plan: fills `table` (HOST int32 [4 + 2 n + n * taps]) for the outputs [first, first + n) of the axis, the crop
 *   window: {taps, n, in_size, 0}, bounds [n][2] = (first tap, tap count), coefficients [n][taps] (zero past the count).  Host
 *   only, no HIP call; double arithmetic in the order above, compiled without contraction.
 * mirx_resample_taps_filter, mirx_resample_plan_filter: the same two for a named filter.  Pillow computes every
 *   filter F of support `sup` the same way: support = sup * fs, taps [max(0, (int)(c - support + 0.5)), min(in_size,
 *   (int)(c + support + 0.5))), weights F((x - c + 0.5) * (1 / fs)) summed in tap order and divided by the sum, coefficients
 *   (int)(0.5 + w * 2^22) for w >= 0 and (int)(-0.5 + w * 2^22) for w < 0, (int)ceil(support) * 2 + 1 slots per output.
 *   MIRX_RESAMPLE_BILINEAR: sup = 1, the triangle above; its tables equal mirx_resample_plan's byte for byte (header word 3 = 0).
 *   MIRX_RESAMPLE_BICUBIC: sup = 2, a = -0.5, x = |x|: x < 1: ((a + 2) x - (a + 3)) x x + 1; x < 2: (((x - 5) x + 8) x - 4) a;
 *   else 0, in this association, one operation per statement; header word 3 = 1.  With first = 0, n = out_size and one call
 *   per axis, each with its own sizes, the tables describe Resize((s, s)) without a crop.  taps <= MIRX_RESAMPLE_MAX_TAPS
 *   stops bicubic at a scale of 16.  Any other filter: MIRX_EINVAL.
 * mirx_resample_batch: one launch for b images of any mix of sizes -> out = device [b, 3, s, s], uint8 (MIRX_RESAMPLE_OUT_U8:
 *   the pixels a model that normalises 8-bit input itself takes) or fp32 (MIRX_RESAMPLE_OUT_F32: (u / 255 - mean[c]) / std[c],
 *   IEEE fp32, correctly rounded division; mean3 / std3 = HOST float [3], unused for uint8).  Everything the kernel reads is one
 *   byte buffer, given twice: blob_host (what the caller filled; read here, on the host) and blob_dev (its device copy, which the
 *   caller has enqueued on `stream` before this call; 16-byte aligned).  Layout: b descriptors of MIRX_RESAMPLE_DESC_WORDS int64
 *   at offset 0: {source offset, w, h, row pitch in bytes, channels (1 or 3, interleaved), x table offset, y table offset, 0};
 *   offsets are bytes from the start of the buffer, multiples of 16, behind the descriptors.  Images of one size may share tables.
 *   Checked BEFORE any HIP call, from blob_host: every image inside the buffer, every table inside the buffer and planned for
 *   this s and this image's side, every tap range inside [0, w) or [0, h), every coefficient >= 0 and every run's sum <= 2^23
 *   (so the 32-bit sums cannot overflow), the LDS of the largest tile (x coefficients + the source rows a 16-row tile taps, 32
 *   columns, 8 bits) <= MIRX_RESAMPLE_MAX_LDS.  Output alignment: 4 elements when s % 4 == 0 (vector stores), 1 otherwise.
 *   out must not overlap blob_dev.  A table names its filter in header word 3: for MIRX_RESAMPLE_BICUBIC coefficients may be
 *   negative and the rule on a run is sum |coeff| <= 2^23 (255 * 2^23 + 2^21 < 2^31 either way); any other value than the two
 *   filters, or an image whose x and y tables name different filters, is refused.
 * Caps: source side <= MIRX_RESAMPLE_MAX_SIDE, taps <= MIRX_RESAMPLE_MAX_TAPS (scale <= 32: an 8192-pixel side at resize 256), s
 * <= MIRX_RESAMPLE_MAX_OUT, b <= MIRX_RESAMPLE_MAX_BATCH.  Anything over a cap, or failing a check: MIRX_EINVAL with a message,
 * nothing launched.  One stream, no host synchronisation, no atomic.
 */
#define MIRX_RESAMPLE_MAX_SIDE 8192
#define MIRX_RESAMPLE_MAX_TAPS 65
#define MIRX_RESAMPLE_MAX_OUT 1024
#define MIRX_RESAMPLE_MAX_BATCH 65536
#define MIRX_RESAMPLE_MAX_RESIZED (1 << 24)
#define MIRX_RESAMPLE_MAX_BYTES (1LL << 40)
#define MIRX_RESAMPLE_MAX_LDS 65536
#define MIRX_RESAMPLE_TILE_W 32
#define MIRX_RESAMPLE_TILE_H 16
#define MIRX_RESAMPLE_DESC_WORDS 8
#define MIRX_RESAMPLE_OUT_U8 0
#define MIRX_RESAMPLE_OUT_F32 1
#define MIRX_RESAMPLE_BILINEAR 0
#define MIRX_RESAMPLE_BICUBIC 1
int mirx_resample_taps(int in_size, int out_size);
int mirx_resample_plan(int in_size, int out_size, int first, int n, int32_t *table, int64_t table_words);
int mirx_resample_taps_filter(int in_size, int out_size, int filter);
int mirx_resample_plan_filter(int in_size, int out_size, int first, int n, int filter, int32_t *table, int64_t table_words);
int mirx_resample_batch(const void *blob_host, const void *blob_dev, int64_t blob_bytes, int64_t b, int s, int out_kind,
                        const float *mean3, const float *std3, void *out, void *stream);

/*
 * The IVF_FLAT index: the reference's own index type -- every driver creates its collection with index_params = {"index_type":
 * "IVF_FLAT", "params": {"nlist": 1024}} (milvus/milvus_setup.py:191-213, nih_zilliz_utils.py) and searches it with
 * {"metric_type": "COSINE", "params": {"nprobe": 10}} (milvus/milvus_retrieval.py:69-86, query_nih_zilliz.py:56-63).  The rows are
 * partitioned into nlist lists by their nearest of nlist centroids; a search scans the lists of the query's nprobe nearest
 * centroids only.  The project's rule holds: no hit is decided from an approximate score.  An answer is THE EXACT TOP-K OF THE ROWS
 * IN THE PROBED LISTS -- fp64 lane-tree scores, ties to the lowest id, bit for bit what mirx_index_search_masked returns under
 * the mask "the row's list is probed" -- and the only approximation is which lists are probed: nprobe >= nlist is
 * mirx_index_search's answer to the bit.  "Nearest" is the metric's own ranking (fp64 lane-tree score, ties to the lowest list
 * number): mirx_index_search over an internal flat index of the centroids, k = 1 for an assignment, k = nprobe for the probes.
 * An ivf is not re-entrant; every call below is synchronous in the host sense unless stated.
 *
 * mirx_ivf_create   1 <= nlist <= 65536; 1 <= dim <= 2048; the metrics of mirx_index_create; MIRX_EINVAL before any device call.
 * mirx_ivf_train    Lloyd's k-means over rows [n, dim] (host or device), n >= nlist (else MIRX_EINVAL); fixes the centroids.
 *     start       centroid j = rows[init_positions[j]] (host, nlist int64 in [0, n)); NULL: init_positions[j] = floor(j n / nlist)
 *     assignment  every row to its nearest centroid, as above
 *     update      per list and column ONE fp64 accumulator over the list's rows in ascending row order, divided by the count and
 *                 rounded once to fp32; with MIRX_METRIC_IP the fp32 mean is then normalised as mirx_l2_normalize does it
 *                 (spherical k-means); an empty list keeps its centroid.  No floating atomics: two calls give equal bits.
 *     stopping    after `iters` (>= 0) updates, or earlier when an assignment pass changes no row's list
 *   One assignment per iteration travels to the host (8 bytes per row), which orders the rows by list for the update.  An ivf that
 *   already holds rows re-assigns them to the new centroids (as mirx_ivf_set_centroids).
 * mirx_ivf_set_centroids / _get_centroids   [nlist, dim] fp32, host or device: a caller's own quantiser, and the tests' way to
 *   force list sizes.  Set on an ivf that holds rows re-assigns them (insertion order inside each list is kept).
 * mirx_ivf_add      rows [n, dim] (host or device), ids as for mirx_index_add (NULL = auto ids, which go on past the largest auto
 *   id handed out).  Before the centroids are fixed: MIRX_ESTATE.  The fp32 master is kept LIST-MAJOR (a list's rows contiguous, in
 *   insertion order) with offsets[nlist + 1] and the ids.  Cost: the new rows' assignment (n x nlist fp64 scores) and a rebuild of
 *   the whole layout into a second allocation -- every resident row moves once per call, so add in large batches.
 * mirx_ivf_remove_ids   the semantics of mirx_index_remove_ids (duplicates count once, absent ids are ignored, every row of a
 *   repeated id goes, auto ids are not reused); the lists stay contiguous and ordered.  The request and the ids meet on the host;
 *   the survivors move once.
 * mirx_ivf_size / _list_sizes (host, nlist int64) / _assign (rows device [n, dim] -> out_lists device [n] int64, the list each
 *   row would be added to; enqueued on `stream`).
 * mirx_ivf_search   the exact top-k of the probed lists.
 *     q              device [nq, dim] fp32;  1 <= k <= 1024;  nprobe >= 1, clamped to nlist
 *     exclude_ids    device, nq int64 or NULL, as for mirx_index_search
 *     out_values / out_f64 / out_ids   device [nq, k]: fp32 reported values and / or fp64 ranking scores (either may be NULL, not
 *                    both), ids; ordered (score desc, id asc), the excluded id skipped, (-1, -inf) past the eligible rows
 *     out_probes     device [nq, nprobe (clamped)] int32 or NULL: the lists probed, nearest first
 *   Work per internal batch of queries: the centroid search; the [nq, nprobe] table inverted into list order on the device
 *   (histogram, scan, scatter: integer atomics hand out slots, each pair owns its slot and no result depends on their order); ONE
 *   launch that scores every (query, probed list) pair -- a work item is (a list, mirx_ivf_row_block() of its rows, up to
 *   mirx_ivf_query_tile(dim) of the queries probing it), the queries in LDS as doubles, the rows streamed once per query group,
 *   scores from the transposed lane tree of the exact tier -- into a compact row per query (its probed lists concatenated in probe
 *   order); then the exact tier's selection over that row with the ids of the lists.  A batch is as many queries as a 1 GiB score
 *   workspace holds rows of `the nprobe largest lists` doubles (MIRX_IVF_OPT_SCORE_BYTES lowers it for tests).  No floating atomics.
 * mirx_ivf_last_stats   waits for `stream`, then copies the counters of the last search.
 * mirx_ivf_query_tile / _row_block   the list scan's block sizes (tests reach their edges); no device touched.
 */
typedef struct mirx_ivf mirx_ivf;
typedef struct mirx_ivf_stats {
    int64_t nq;            /* queries in the call                                   */
    int64_t rows_scored;   /* (query, row) pairs scored in fp64                     */
    int64_t pairs;         /* (query, probed list) pairs                            */
    int64_t work_items;    /* work items of the list scan, summed over its batches  */
    int64_t batches;       /* internal batches                                      */
} mirx_ivf_stats;
#define MIRX_IVF_MAX_NLIST 65536
#define MIRX_IVF_MAX_DIM 2048
#define MIRX_IVF_OPT_SCORE_BYTES 1   /* test hook: the score workspace's budget in bytes; 0 = default (1 GiB) */
int mirx_ivf_create(int dim, int metric, int nlist, int device, mirx_ivf **out);
void mirx_ivf_destroy(mirx_ivf *ivf);
int mirx_ivf_train(mirx_ivf *ivf, const float *rows, int64_t n, const int64_t *init_positions_or_null, int iters, void *stream);
int mirx_ivf_set_centroids(mirx_ivf *ivf, const float *centroids);
int mirx_ivf_get_centroids(const mirx_ivf *ivf, float *out_centroids);
int mirx_ivf_add(mirx_ivf *ivf, const float *rows, int64_t n, const int64_t *ids_or_null);
int mirx_ivf_remove_ids(mirx_ivf *ivf, const int64_t *ids, int64_t n, int64_t *out_removed_or_null, void *stream);
int64_t mirx_ivf_size(const mirx_ivf *ivf);
int mirx_ivf_list_sizes(const mirx_ivf *ivf, int64_t *out_sizes);
int mirx_ivf_assign(mirx_ivf *ivf, const float *rows, int64_t n, int64_t *out_lists, void *stream);
int mirx_ivf_search(mirx_ivf *ivf, const float *q, int64_t nq, int k, int nprobe, const int64_t *exclude_ids_or_null,
                    float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids, int32_t *out_probes_or_null,
                    void *stream);
int mirx_ivf_last_stats(mirx_ivf *ivf, void *stream, mirx_ivf_stats *out);
int mirx_ivf_set_option(mirx_ivf *ivf, int option, int64_t value);
int mirx_ivf_query_tile(int dim);
int mirx_ivf_row_block(void);

/*
 * IVF_SQ8: the same lists, probes, work items and top-k with the master kept as 8-bit codes, a quarter of the fp32 master (the
 * reference's create_index documents the type: 'IVF_FLAT', 'IVF_SQ8', 'IVF_PQ', 'HNSW', 'FLAT', milvus/milvus_setup.py:191-213).
 * The rule is bent in one declared place: AN IVF_SQ8 ANSWER IS THE IVF_FLAT ANSWER OVER THE DECODED ROWS -- per query the exact
 * fp64 top-k over the decoded rows of its probed lists, bit for bit what mirx_index_search_masked returns on a flat index that
 * holds the decoded fp32 rows under the same ids; nprobe >= nlist is mirx_index_search over the decoded rows.  The approximations
 * are the choice of lists and the quantiser, and both are defined exactly.
 *
 * Quantiser: per column, global (not per list, not residual); vmin[dim], scale[dim] fp32.
 *     train    vmin[d] / vmax[d] = min / max of column d over the training rows (NaN ignored; a zero minimum is stored as +0; a
 *              column without a number gets vmin = scale = 0), scale[d] = (float)(((double)vmax[d] - (double)vmin[d]) / 255.0).
 *              Partials per workgroup folded in a fixed order, no floating atomics: two calls give equal bits.
 *     encode   t = ((double)x - (double)vmin[d]) / (double)scale[d]; code = (uint8)min(255.0, max(0.0, floor(t + 0.5))), t + 0.5
 *              one IEEE double addition; scale[d] == 0 -> 0; NaN, -inf -> 0; +inf -> 255; rows outside the range clamp.
 *     decode   xhat = (float)((double)vmin[d] + (double)code * (double)scale[d]): the product is exact in double, one rounding to
 *              double, one to float.
 *   A row's list is chosen from its ORIGINAL fp32 values, then the row is encoded; the originals are not kept.
 *
 * mirx_ivf_create_typed   mirx_ivf_create with kind = MIRX_IVF_FLAT (what mirx_ivf_create means) or MIRX_IVF_SQ8; any other kind:
 *   MIRX_EINVAL before any device call.  mirx_ivf_kind: the kind, -1 for NULL.
 * mirx_ivf_sq8_train (rows [n, dim], n >= 1, host or device) / _sq8_set_range / _sq8_get_range (vmin, scale: dim fp32 each, host or
 *   device) fix or read the range.  mirx_ivf_get_codes (out_codes [size, dim] uint8, ids, list numbers) and mirx_ivf_reconstruct
 *   (out_rows [size, dim] fp32 decoded, ids): device arrays in list-major order, the order of the master; the _or_null ones may be
 *   NULL.  All of these on a MIRX_IVF_FLAT handle: MIRX_EINVAL.
 * State, MIRX_IVF_SQ8 (MIRX_ESTATE, nothing changed): mirx_ivf_add before both the centroids and the range are fixed;
 *   mirx_ivf_sq8_train / _sq8_set_range while rows are resident (they were encoded with the old range); mirx_ivf_train /
 *   _set_centroids while rows are resident (IVF_FLAT re-assigns its rows; there are no originals to re-assign here).  Every other
 *   mirx_ivf_* call keeps its contract; mirx_ivf_search reads the codes: a lane loads four codes where it loaded four floats,
 *   decodes them once per row group with its columns' (double) vmin and scale held in registers, and goes on as for fp32 rows.
 * mirx_sq8_encode / mirx_sq8_decode   the quantiser over device arrays (rows [n, dim] fp32, codes [n, dim] uint8, vmin / scale
 *   [dim]), without an index; encode waits for its work, decode is enqueued on `stream`.
 */
#define MIRX_IVF_FLAT 0
#define MIRX_IVF_SQ8 1
int mirx_ivf_create_typed(int dim, int metric, int nlist, int kind, int device, mirx_ivf **out);
int mirx_ivf_kind(const mirx_ivf *ivf);
int mirx_ivf_sq8_train(mirx_ivf *ivf, const float *rows, int64_t n, void *stream);
int mirx_ivf_sq8_set_range(mirx_ivf *ivf, const float *vmin, const float *scale);
int mirx_ivf_sq8_get_range(const mirx_ivf *ivf, float *out_vmin, float *out_scale);
int mirx_ivf_get_codes(const mirx_ivf *ivf, uint8_t *out_codes, int64_t *out_ids_or_null, int64_t *out_lists_or_null);
int mirx_ivf_reconstruct(const mirx_ivf *ivf, float *out_rows, int64_t *out_ids_or_null);
int mirx_sq8_encode(const float *rows, int64_t n, int dim, const float *vmin, const float *scale, uint8_t *out_codes, void *stream);
int mirx_sq8_decode(const uint8_t *codes, int64_t n, int dim, const float *vmin, const float *scale, float *out_rows, void *stream);

/*
 * IVF_PQ: the same lists and probes with the master kept as m codeword numbers per row (m bytes; the third IVF type of the
 * reference's create_index, milvus/milvus_setup.py:191-213).  The rule is bent in one declared place: AN IVF_PQ ANSWER IS THE
 * EXACT TOP-K, UNDER (score desc, id asc), OF THE ASYMMETRIC-DISTANCE (ADC) SCORE DEFINED BELOW, OVER THE ROWS OF THE PROBED LISTS.
 * It is not a search over mirx_ivf_reconstruct's rows: the ADC sum associates differently from the lane tree, so the two differ
 * in bits.  Every step is defined to the bit.
 *
 * Parameters: m sub-quantisers of 256 codewords (nbits = 8), dsub = dim / m; m % 4 == 0, 4 <= m <= 64, dim % (4 m) == 0.  Codes
 *   encode the raw row (not a residual, not per list); mirx_ivf_create_pq_ex below adds the residual form.
 * Codebooks cb[m][256][dsub] fp32.
 *     train    sub-space j's codebook is mirx_ivf_train's loop on columns [j dsub, (j+1) dsub) with 256 lists and ALWAYS the L2
 *              metric (no normalisation): start rows[floor(c n / 256)], one fp64 accumulator per codeword and column in ascending
 *              row order, an unused codeword keeps its bits, at most `iters` updates, stop when nothing moves.  n >= 256.
 *     encode   code[j] = the nearest codeword of sub-vector j under the L2 ranking score, ties to the lowest code:
 *              mirx_index_search(k = 1) over the 256 codewords with ids 0 .. 255 -- list assignment's own rule, not restated.
 *     decode   the row's m codewords concatenated: exact fp32 copies.
 *   A row's list is chosen from its ORIGINAL fp32 values, then the row is encoded; the originals are not kept.
 * Tables, per query, fp64: T[j][c], j < m, c < 256 = ONE sequential accumulator from 0.0 over e = 0 .. dsub-1 ascending;
 *     IP   acc = acc + (double)q[j dsub + e] * (double)cb[j][c][e]                (the product is exact in double)
 *     L2   d = (double)q[..] - (double)cb[..]; acc = acc + d * d, the product ROUNDED to double before the addition (no fma)
 * Score of a row: s = 0.0; for j ascending: s = s + T[j][code[j]].  The ranking score is s (IP) or -s (L2); reported fp32 values,
 *   the excluded id, (-1, -inf) past the eligible rows and the order of the results are mirx_ivf_search's.  nprobe >= nlist ranks
 *   every row by the same scores.
 *
 * mirx_ivf_create_pq   the only way to a MIRX_IVF_PQ handle (mirx_ivf_kind: 2); mirx_ivf_create's limits and the ones above,
 *   nbits == 8: MIRX_EINVAL before any device call.  mirx_ivf_create_typed(kind = MIRX_IVF_PQ) stays MIRX_EINVAL: it has no m.
 * mirx_ivf_pq_train (rows [n, dim], n >= 256, host or device) / _pq_set_codebooks / _pq_get_codebooks ([m][256][dsub] fp32, host
 *   or device) fix or read the codebooks.  mirx_ivf_pq_m: m, -1 for another kind.  mirx_ivf_get_codes returns m bytes per row,
 *   mirx_ivf_reconstruct the decoded rows.  The PQ calls on a FLAT or SQ8 handle, the SQ8 calls on a PQ handle: MIRX_EINVAL.
 * State (MIRX_ESTATE, nothing changed): mirx_ivf_add before both the centroids and the codebooks are fixed; mirx_ivf_train,
 *   _set_centroids, _pq_train and _pq_set_codebooks while rows are resident.
 * mirx_ivf_search on a PQ handle, per internal batch: the probes; k_pq_tables writes every query's table into the workspace (a
 *   query costs its compact row of doubles plus m x 2 KiB of the budget); ONE scan launch whose work item is (a query,
 *   mirx_ivf_pq_item_rows() consecutive entries of its compact row) -- the workgroup holds the query's table in LDS, a thread owns
 *   an entry, loads the row's m code bytes as words and adds the m table entries; then mirx_ivf_search's top-k.  In
 *   mirx_ivf_stats work_items counts these items: the sum over the queries of ceil(entries / item_rows).  No floating atomics.
 * mirx_pq_encode / _pq_decode / _pq_tables   the quantiser and the tables over device arrays (rows [n, dim] fp32, codes [n, m]
 *   uint8, codebooks [m][256][dsub], out_tables_f64 [nq, m, 256]), without an index; encode waits for its work (m searches per
 *   call: it is not a hot path), the other two are enqueued on `stream`.
 */
#define MIRX_IVF_PQ 2
int mirx_ivf_create_pq(int dim, int metric, int nlist, int m, int nbits, int device, mirx_ivf **out);
int mirx_ivf_pq_train(mirx_ivf *ivf, const float *rows, int64_t n, int iters, void *stream);
int mirx_ivf_pq_set_codebooks(mirx_ivf *ivf, const float *codebooks);
int mirx_ivf_pq_get_codebooks(const mirx_ivf *ivf, float *out_codebooks);
int mirx_ivf_pq_m(const mirx_ivf *ivf);
int mirx_ivf_pq_item_rows(void);
int mirx_pq_encode(const float *rows, int64_t n, int dim, int m, const float *codebooks, uint8_t *out_codes, void *stream);
int mirx_pq_decode(const uint8_t *codes, int64_t n, int dim, int m, const float *codebooks, float *out_rows, void *stream);
int mirx_pq_tables(const float *q, int64_t nq, int dim, int m, int metric, const float *codebooks, double *out_tables_f64,
                   void *stream);

/*
 * IVF_PQ with residual coding (opt-in: mirx_ivf_create_pq_ex(by_residual = 1); a handle from mirx_ivf_create_pq, or with
 * by_residual = 0, is the raw form above in every bit).  The codes encode the row minus the centroid of its list, so the 256
 * codewords of a sub-space describe the spread inside a list instead of telling the lists apart.  c_l = the centroid of list l.
 *     residual   r_e = x_e - c_{l,e} in fp32, one rounding; l = the row's list from its ORIGINAL values, as mirx_ivf_add assigns it.
 *     codebooks  `train` above on the residual sub-vectors of the training rows (always L2); codes = `encode` above of the residuals.
 *     base       of a (query, probed list): B[q][l] = sum over j ascending of P_j, P_j ONE sequential fp64 accumulator from 0.0 over
 *                the columns of sub-space j ascending, each step + (double)q_e * (double)c_{l,e} (the product is exact).
 *     tables     the IP tables T[j][c] above of the residual codebooks, one table per query, for BOTH metrics.
 *     ip         of an entry: ip = B[q][l]; for j ascending: ip = ip + T[j][code[j]].
 *     IP         ranking score = ip.
 *     L2         QQ[q] = the two-level sum (as B) of (double)q_e * (double)q_e.  N2[row] = the two-level sum of xh_e * xh_e with
 *                xh_e = (double)c_{l,e} + (double)cb[j][code_j][e], each product rounded to double and then added; computed once,
 *                when the row is added, and kept beside its id (8 bytes a row, L2 handles only).
 *                ranking score = -((QQ + N2) - 2.0 * ip), each operation rounded in that order (2.0 * ip is exact).  The expanded
 *                distance may come out slightly negative; the reported value clamps it as mirx_ivf_search's does.
 *   Selection, the excluded id, the padding and the reported values are mirx_ivf_search's.  mirx_ivf_reconstruct returns
 *   (float)(c_{l,e} + codeword_e), one fp32 rounding per column; mirx_ivf_get_codes is unchanged.
 * mirx_ivf_create_pq_ex   mirx_ivf_create_pq with the flag; by_residual other than 0 / 1: MIRX_EINVAL.  mirx_ivf_pq_by_residual:
 *   the flag, -1 for another kind.
 * State: on a residual handle mirx_ivf_pq_train needs fixed centroids (MIRX_ESTATE otherwise): it assigns its rows, forms their
 *   residuals and trains on them.  The other state rules are the raw form's.
 * mirx_ivf_get_norms   N2 of the resident rows in list-major order (the order of mirx_ivf_get_codes), to a device array; MIRX_EINVAL
 *   unless the handle is residual and L2.
 * mirx_pq_residuals / mirx_pq_bases   the kernels over device arrays, without an index, enqueued on `stream`: out [n, dim] fp32
 *   residuals of rows under lists [n] (int64) and centroids [nlist, dim]; out_base_f64 [nq, nprobe] and out_qq_f64_or_null [nq] for
 *   queries, list numbers lists [nq, nprobe] (int32) and centroids.  A list number outside 0 .. nlist-1 reads nothing: its
 *   residual row is NaN, its base 0.0.
 * mirx_ivf_search's workspace budget counts 8 nprobe + 8 more bytes per query on a residual handle.
 */
int mirx_ivf_create_pq_ex(int dim, int metric, int nlist, int m, int nbits, int by_residual, int device, mirx_ivf **out);
int mirx_ivf_pq_by_residual(const mirx_ivf *ivf);
int mirx_ivf_get_norms(const mirx_ivf *ivf, double *out_norms_f64);
int mirx_pq_residuals(const float *rows, int64_t n, int dim, const int64_t *lists, const float *centroids, int nlist,
                      float *out_rows, void *stream);
int mirx_pq_bases(const float *q, int64_t nq, int dim, int m, const int32_t *lists, int nprobe, const float *centroids, int nlist,
                  double *out_base_f64, double *out_qq_f64_or_null, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIRX_H */
