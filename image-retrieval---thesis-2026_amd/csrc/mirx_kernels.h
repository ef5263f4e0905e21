// mirx_kernels.h -- launch wrappers implemented in the k_*.hip files (internal, not ABI).
#pragma once
#include "mirx_common.h"

namespace mirx {

// ---- the search's routing constants: defined in mirx_api.hip, where the tests read their values; used in mirx_index.hip ----
extern const int64_t QUERY_BATCH;
extern const int64_t TIER1_MIN_ROWS;
extern const int TIER1_MAX_K;

// ---- k_prep.hip -------------------------------------------------------------------------
// Rows [n, dim] fp32 (device) -> padded fp32 master, bf16 copy, per-row bias (metric 1:
// -0.5*||g||^2, metric 0: 0) and an atomic running maximum of ||g|| (upper bound, fp32 bits).
hipError_t launch_ingest(const float *src, int64_t n, int dim, int dimp, float *g32,
                         uint16_t *g16, float *gbias, unsigned *gnorm_max_bits, int metric,
                         hipStream_t st);
// Queries [nq, dim] fp32 -> padded fp32 [nq_pad, dimp], bf16 [nq_pad, dimp], upper bound of
// ||q|| per query; rows nq..nq_pad-1 are zero.
hipError_t launch_prep_queries(const float *q, int64_t nq, int64_t nq_pad, int dim, int dimp,
                               float *q32p, uint16_t *q16, float *qnorm, hipStream_t st);
hipError_t launch_l2_normalize(float *x, int64_t n, int dim, hipStream_t st);
hipError_t launch_bn_relu_gap_l2norm(const float *x, const float *scale, const float *shift,
                                     int64_t n, int c, int hw, int normalize, float *y,
                                     hipStream_t st);
hipError_t launch_bn_relu_nchw(const float *x, int64_t x_batch_stride, const float *scale,
                               const float *shift, int64_t n, int c, int hw, float *y, hipStream_t st);
hipError_t launch_bn_relu_avgpool2(const float *x, int64_t x_batch_stride, const float *scale,
                                   const float *shift, int64_t n, int c, int h, int w, float *y,
                                   int64_t x_plane_stride, hipStream_t st, int64_t y_batch_stride = 0);
hipError_t launch_stem(const float *x, const float *w, const float *scale, const float *shift,
                       int64_t n, int h, int wd, float *y, hipStream_t st);
// k_stem_s3.hip: the same stem on three-term bf16 MFMAs; w3 = pre-split weights [2][11][3][32][16] bf16
// y_bs = output batch stride in floats (64 * (h/4) * (wd/4) for a packed tensor); out_range: range slots or null
hipError_t launch_stem_s3(const float *x, const uint16_t *w3, const float *scale, const float *shift, int64_t n, int h,
                          int wd, float *y, int64_t y_bs, float *out_range, hipStream_t st);

// k_stem_h2.hip: the stem on two fp16 terms (w2 = [2][11][2][32][16] fp16, per-output-channel scales in oscale[64];
// in_range = range slots of the input images) and the pass that fills such slots with the largest |x|
hipError_t launch_stem_h2(const float *x, const uint16_t *w2, const float *oscale, const float *scale, const float *shift,
                          int64_t n, int h, int wd, float *y, int64_t y_bs, const float *in_range, float *out_range,
                          hipStream_t st);
hipError_t launch_range_absmax(const float *x, int64_t per_image, int64_t n, float *row, hipStream_t st);
// raw 8-bit images, ToTensor + Normalize applied while staging (bit-identical to the fp32 path on the normalised tensor)
hipError_t launch_stem_h2_u8(const uint8_t *x, const float *mean, const float *stdv, const uint16_t *w2, const float *oscale,
                             const float *scale, const float *shift, int64_t n, int h, int wd, float *y, int64_t y_bs,
                             const float *in_range, float *out_range, hipStream_t st);
hipError_t launch_range_absmax_u8(const uint8_t *x, int64_t hw, int64_t n, const float *mean, const float *stdv, float *row,
                                  hipStream_t st);

// ---- k_conv1x1.hip ----------------------------------------------------------------------
hipError_t launch_conv1x1(const float *x, int64_t xbs, int cin, const float *scale, const float *shift,
                          const float *wt, const float *bias, int64_t n, int hw, int cout, int relu_out, float *y,
                          hipStream_t st);

// ---- k_convnext.hip ---------------------------------------------------------------------
hipError_t launch_dwconv7_nhwc(const float *x, const float *wt, const float *bias, int64_t n, int c, int h, int wd, float *y,
                               hipStream_t st);
hipError_t launch_dwconv7(const float *x, const float *w, const float *bias, int64_t n, int c, int h, int wd,
                          float *y, hipStream_t st);
// gx[b][c] = sqrt(sum over the hw positions of x[b][p][c]^2)       (x = [n][hw][c], channels last)
hipError_t launch_grn_norm(const float *x, int64_t n, int hw, int c, float *gx, hipStream_t st);
hipError_t launch_grn_scale(const float *gx, const float *weight, int64_t n, int c, float eps, float *scale, float *smax,
                            hipStream_t st);
// x[b][p][c] = x[b][p][c] * scale[b][c] + shift[c], in place

// ---- k_exact.hip ------------------------------------------------------------------------
// out[i*ld + j] = fp64 ranking score of query qlist[i] (or i when qlist == null) vs row j.
hipError_t launch_scores_f64(const float *q32p, const int32_t *qlist, int nq, const float *g32,
                             int64_t n, int dimp, int metric, double *out, int64_t ld,
                             hipStream_t st);
// Per query row of `scores` [nq, ld]: top-k by (score desc, id asc), skipping exclude ids.
// Writes out_f64 / out_ids / out_val at row qlist[i] (or i) of the [*, k] outputs.
hipError_t launch_row_topk(const double *scores, int64_t ld, int64_t n, const int64_t *ids,
                           const int32_t *qlist, int nq, const int64_t *exclude, int k,
                           int metric, double *out_f64, int64_t *out_ids, float *out_val,
                           hipStream_t st);
// Full sort of every row: hits [nq, np2] (np2 = power of two >= n) built from scores, sorted.
hipError_t launch_rank_rows(const double *scores, int64_t ld, int64_t n, const int64_t *ids,
                            const int64_t *exclude, int nq, Hit *work, int64_t np2, int metric,
                            int64_t *out_ids, float *out_val, hipStream_t st);
hipError_t launch_topk_merge(const double *in_scores, const int64_t *in_ids, int nshard,
                             int64_t nq, int k, int metric, double *out_f64, float *out_val,
                             int64_t *out_ids, hipStream_t st);

// ---- k_ranksort.hip: segmented stable LSD radix sort of (64-bit key, int32 row) pairs, the ranking past 65536 rows ----------
int64_t rank_sort_tiles(int64_t n);              // RANK_TILE-element tiles of an n-element segment
// keys[i*n + j], pay[i*n + j] of query i: position j holds row r = perm ? perm[j] : j (perm = the rows in (id, row) order, null
// when that is the identity) with rank_key(scores[i*ld + r]); rows whose id is exclude[i] get the key of -inf, or with
// drop_excluded the key after every score's.
hipError_t launch_rank_sort_build(const double *scores, int64_t ld, int64_t n, const int64_t *ids, const int32_t *perm,
                                  const int64_t *exclude, int drop_excluded, int nq, uint64_t *keys, int32_t *pay, hipStream_t st);
// one segment that sorts into (id, row) order: key = id ^ sign bit, payload = row
hipError_t launch_rank_sort_build_ids(const int64_t *ids, int64_t n, uint64_t *keys, int32_t *pay, hipStream_t st);
// nseg segments of n pairs, ascending by key, equal keys in their input order; in / out = keys_a, pay_a; keys_b, pay_b = scratch of
// the same size; hist = nseg * 256 * rank_sort_tiles(n) words.  No workgroup waits for another: three launches per 8-bit digit.
// key_bits (a multiple of 16, <= 64): keys that agree above their low key_bits bits need only those digits sorted.
hipError_t launch_rank_sort(uint64_t *keys_a, int32_t *pay_a, uint64_t *keys_b, int32_t *pay_b, unsigned *hist, int64_t n,
                            int nseg, hipStream_t st, int key_bits = 64);
// ranks 0 .. kout-1 of every query from the sorted payload: ids, fp32 reported values and / or fp64 scores ([nq, kout] each).  The
// excluded id reads -inf; with drop_excluded its slot reads id -1 (those rows are last, see launch_rank_sort_build).
hipError_t launch_rank_sort_write(const int32_t *pay, int64_t n, int64_t kout, const double *scores, int64_t ld,
                                  const int64_t *ids, const int64_t *exclude, int drop_excluded, int metric, int nq,
                                  int64_t *out_ids, float *out_val, double *out_f64, hipStream_t st);

// ---- k_compact.hip: order-preserving removal of rows (mirx_index_remove_ids) -------------------------------------------------
int64_t compact_tiles(int64_t n);                // COMPACT_TILE-row tiles of an n-row gallery
size_t compact_scratch_bytes(int64_t chunk_rows, int dimp);
// pos[r] (n + 1 entries) = rows in front of row r whose id is not in the request; pos[n] = the survivors.  req[0 .. nreq) = the
// requested ids as keys id ^ sign bit, ascending as unsigned (launch_rank_sort_build_ids + launch_rank_sort), duplicates allowed.
// part = compact_tiles(n) words.  Three launches: mark + tile sums, scan of the tile sums, apply.
hipError_t launch_compact_scan(const int64_t *ids, int64_t n, const uint64_t *req, int64_t nreq, int32_t *pos, int32_t *part,
                               hipStream_t st);
// the same from keep flags: pos[r] = 0 / 1 for r < n and part[tile] = the flags' sum over each COMPACT_TILE rows on entry (what the
// mark launch leaves, or k_mask.hip's pass); the two scan launches
hipError_t launch_compact_scan_flags(int32_t *pos, int64_t n, int32_t *part, hipStream_t st);
// the kept rows of [0, n), pos[n] < n of them, in order: fp32 row r -> s32 row pos[r], its id -> sid[pos[r]] (one gather launch;
// the gallery is only read)
hipError_t launch_compact_gather(const float *g32, const int64_t *ids, const int32_t *pos, int64_t n, int dimp, float *s32,
                                 int64_t *sid, hipStream_t st);
// the survivors of source rows [c0, c1), c1 - c0 <= chunk_rows, to rows pos[c0] .. of g32 / g16 / ids / gbias through `scratch`
// (compact_scratch_bytes): a gather launch, then a place launch.  Chunks must be issued in ascending order.
hipError_t launch_compact_chunk(float *g32, uint16_t *g16, int64_t *ids, float *gbias, void *scratch, int64_t chunk_rows,
                                const int32_t *pos, int64_t c0, int64_t c1, int dimp, hipStream_t st);

// ---- k_mask.hip: a search under a row mask (mirx_index_search_masked / mirx_index_rank_top_masked) ---------------------------
// One pass over allow[0 .. n) (device, non-zero = eligible): bias[r] for r < cap (gbias[r], or 0 without gbias, for allowed rows
// and the rows past n; -inf for masked rows), and for r < n the keep flag pos[r], mids[r] = the id or INT64_MAX, and the flags'
// sums per COMPACT_TILE rows in part[] -- ready for launch_compact_scan_flags.
hipError_t launch_mask_pass(const uint8_t *allow, int64_t n, int64_t cap, const float *gbias, const int64_t *ids, float *bias,
                            int64_t *mids, int32_t *pos, int32_t *part, hipStream_t st);
// scores [nq, ld]: the entries of masked rows -> -inf; pos = the scanned positions (n + 1 entries; row r is masked iff
// pos[r + 1] == pos[r])
hipError_t launch_mask_scores(double *scores, int64_t ld, int64_t n, const int32_t *pos, int nq, hipStream_t st);
// leave-group-out (mirx_index_search_leave_out).  scores [nq, ld] of the queries qlist[0 .. nq) (or 0 .. nq-1 without a list): the
// entry of row r becomes NaN where query_codes[q] >= 0 and row_codes[r] == query_codes[q].  A masked entry is (-inf, INT64_MAX)
// because its id is masked with it; a left-out row keeps its id (the id vector serves every query), and (-inf, id) would rank
// before an empty slot.  NaN ranks before nothing (hit_before compares with > and ==), so k_row_topk never takes the entry.
hipError_t launch_leave_out_scores(double *scores, int64_t ld, int64_t n, const int32_t *row_codes, const int32_t *query_codes,
                                   const int32_t *qlist, int nq, hipStream_t st);
// codes of the kept rows in the gather's order: out[pos[r]] = row_codes[r] for every row r < n that the scanned positions keep
hipError_t launch_mask_gather_codes(const int32_t *row_codes, const int32_t *pos, int64_t n, int32_t *out, hipStream_t st);
// The radix ranking (rank_top under a mask, the range search's exact route) takes the allow bytes themselves: masked iff allow[r] == 0.
// keys / pay [nq, n] as launch_rank_sort_build leaves them: a masked row's key -> RANK_KEY_LAST
hipError_t launch_mask_rank_keys(uint64_t *keys, const int32_t *pay, int64_t n, const uint8_t *allow, int nq, hipStream_t st);
// after launch_rank_sort_write: output slots whose row is masked -> (-1, -inf)
hipError_t launch_mask_rank_tail(const int32_t *pay, int64_t n, int64_t kout, const uint8_t *allow, int nq, int64_t *out_ids,
                                 float *out_val, double *out_f64, hipStream_t st);

// ---- k_anomaly.hip: class centroids, nearest-centroid distances, segmented binary ranking metrics (include/mirx.h) -----------
int64_t an_chunk_rows(int64_t n, int d);          // rows per chunk of the centroid sums: a function of n and d alone
int64_t class_centroids_workspace_bytes(int64_t n, int d, int k);
hipError_t launch_class_centroids(const float *rows, int64_t n, int d, const int64_t *labels, const int64_t *classes_host, int k,
                                  void *workspace, double *centroids, int64_t *counts, int *bad, hipStream_t st);
hipError_t launch_centroid_min_dist(const float *rows, int64_t n, int d, const double *centroids, int k, double *dist,
                                    int32_t *nearest, double *max_out, hipStream_t st);
int64_t binary_rank_metrics_workspace_bytes(int64_t nseg, int64_t n);
hipError_t launch_binary_rank_metrics(const double *scores, const uint8_t *positive, int64_t nseg, int64_t n, const double *norm,
                                      double level, void *workspace, double *thresholds, int64_t *tps, int64_t *fps, int64_t *out_t,
                                      double *out_auroc, double *out_aupr, double *out_fpr, int *bad, hipStream_t st);

// ---- k_insdel.hip: the insertion / deletion game's step maps, blur substrate, step images and curve scores (include/mirx.h) ----
int64_t insdel_steps_workspace_bytes(int64_t k, int64_t hw);
hipError_t launch_insdel_steps(const float *sal, int64_t k, int64_t hw, int64_t step, void *workspace, int32_t *t, hipStream_t st);
int64_t blur2d_blocks(int64_t planes, int h, int w);      // workgroups of the blur's launch
hipError_t launch_blur2d_same(const float *x, int64_t planes, int h, int w, const float *kern, int klen, float *y, hipStream_t st);
hipError_t launch_insdel_compose(const int32_t *t, int64_t n_rows, int64_t hw, const float *bank, int64_t n_bank, const int32_t *start,
                                 const int32_t *finish, const int32_t *row, int64_t n_steps, int64_t g0, int64_t n, float *out,
                                 hipStream_t st);
hipError_t launch_insdel_curves(const float *q, const float *r, int64_t n_curves, int64_t n_steps, int d, double *scores, double *auc,
                                int64_t *zero_counter, hipStream_t st);

// ---- k_sbsm.hip: SBSM occlusion saliency on interval-described window sets: masked images, gains, the saliency map (include/mirx.h) ----
hipError_t launch_sbsm_compose(const float *x, int64_t b, int c, int h, int w, const int32_t *row_iv, const int32_t *col_iv, int nc,
                               int64_t g0, int64_t n, float *out, hipStream_t st);
hipError_t launch_sbsm_gain(const float *e_q, const float *e_m, const float *e_r, int64_t rows, int64_t n_masks, int64_t b, int d,
                            double *gain, hipStream_t st);
int64_t sbsm_workspace_bytes(int64_t rows, int nr, int w);
hipError_t launch_sbsm_accumulate(const double *gain, int64_t rows, const int32_t *row_iv, int nr, const int32_t *col_iv, int nc, int h,
                                  int w, void *workspace, float *sal, hipStream_t st);

// ---- k_resample.hip: batched Resize + CenterCrop of 8-bit images, bit-equal to Pillow's BILINEAR / BICUBIC (include/mirx.h) ----
// filter = MIRX_RESAMPLE_BILINEAR or MIRX_RESAMPLE_BICUBIC (checked by the caller)
int resample_taps(int in_size, int out_size, int filter);                                          // host only
void resample_plan(int in_size, int out_size, int first, int n, int filter, int32_t *table);       // host only; taps <= MIRX_RESAMPLE_MAX_TAPS
const char *resample_check(const void *blob_host, int64_t blob_bytes, int64_t b, int s, int64_t *lds);   // host only; null = fine
hipError_t launch_resample(const void *blob_dev, int64_t b, int s, int out_f32, const float *mean3, const float *std3, void *out,
                           int64_t lds, hipStream_t st);

// ---- k_conv1x1_s3.hip --------------------------------------------------------------------
hipError_t launch_conv1x1_s3(const float *x, int64_t xbs, int cin, const float *scale, const float *shift,
                             const uint16_t *w3, const float *bias, int64_t n, int hw, int cout, int relu_out,
                             float *y, int64_t ybs, hipStream_t st);

// ---- k_conv1x1_h2.hip: the same convolution on two fp16 terms per operand; ranges travel in 64 "range slots" ----
hipError_t launch_conv1x1_h2(const float *x, int64_t xbs, int cin, const float *scale, const float *shift,
                             const uint16_t *w2, const float *oscale, const float *bias, int64_t n, int hw, int cout,
                             int relu_out, float *y, int64_t ybs, const float *in_amax, float in_ks, float in_kb,
                             float *out_amax, float y_ks, float y_kb, float *y_inv_out, int64_t xps, int64_t yps,
                             hipStream_t st);

void set_conv1x1_small_max_wg(int v);      // mirx_set_tuning(MIRX_TUNE_CONV1X1_SMALL_MAX_WG)
void set_conv1x1_ring(int v);             // mirx_set_tuning(MIRX_TUNE_CONV1X1_RING)
// k_conv1x1_h2s.hip: the same contract for small launches (one wave per 32 x 32 tile, no LDS); bit-identical results
hipError_t launch_conv1x1_h2_small(const float *x, int64_t xbs, int cin, const float *scale, const float *shift,
                                   const uint16_t *w2, const float *oscale, const float *bias, int64_t n, int hw, int cout,
                                   int relu_out, float *y, int64_t ybs, const float *in_amax, float in_ks, float in_kb,
                                   float *out_amax, float y_ks, float y_kb, float *y_inv_out, int64_t xps, int64_t yps,
                                   hipStream_t st);

// ---- k_linear_split.hip: the token-major Linear, fp32 operands split into 16-bit terms while they are staged ----
// two fp16 terms per operand (3 MFMAs per product block); the caller supplies the power-of-two range scales
hipError_t launch_linear_h2(const float *x, int64_t m, int k, const uint16_t *w2, const float *bias, int n, int act,
                            const float *res, const float *gamma, float x_scale, float out_scale, float *y,
                            int tokens_per_image, const float *xb_dev, hipStream_t st, bool rows_out = false,
                            float *sq_out = nullptr);
hipError_t launch_grn_norm_partials(const float *part, int tpi, int64_t n_img, int c, float *gx, hipStream_t st);

// three bf16 terms per operand (6 MFMAs per product block), the same kernel template
// tokens_per_image == 0: y / res are [m][n]; > 0: token t is pixel t % tpi of image t / tpi and y / res are NCHW
hipError_t launch_linear_s3(const float *x, int64_t m, int k, const uint16_t *w3, const float *bias, int n, int act,
                            const float *res, const float *gamma, float *y, int tokens_per_image, hipStream_t st);

// ---- k_conv3x3.hip ----------------------------------------------------------------------
hipError_t launch_conv3x3_wino(const float *x, const float *u, int64_t n, int side, float *out, int64_t out_bs,
                               float *out_range, hipStream_t st);
// ---- k_conv3x3_s3.hip: the same convolution on three-term bf16 MFMAs (side 56 / 28 / 14) ----------
hipError_t launch_conv3x3_wino_s3(const float *x, const uint16_t *u3, int64_t n, int side, float *out, int64_t out_bs,
                                  hipStream_t st);
// ---- k_conv3x3_d3.hip: the same convolution as a direct implicit GEMM on three-term bf16 MFMAs ------
// w3 = [8 stages][9 taps][3 terms][32 oc][16 c] bf16
hipError_t launch_conv3x3_d3(const float *x, const uint16_t *w3, int64_t n, int side, float *out, int64_t out_bs,
                             hipStream_t st);

// ---- k_dense_fused.hip: a whole dense layer of the 14 x 14 / 7 x 7 maps, bottleneck resident in LDS --------------------
hipError_t launch_dense_fused(float *buf, int64_t bs, int cin, const float *scale, const float *shift, const uint16_t *w2,
                              const float *oscale, const float *bias, const uint16_t *w3, const float *c3osc, int64_t n,
                              int side, float *range_row, float in_ks, float in_kb, float y_ks, float y_kb, hipStream_t st);

// ---- k_norm.hip: LayerNorm over rows, patchify (+ LayerNorm2d), attention for short query sets ------------------
hipError_t launch_layernorm_rows(const float *x, int64_t m, int c, const float *gamma, const float *beta, float eps,
                                 float *y, int tokens_per_image, hipStream_t st, void *yt = nullptr, float scale = 1.f,
                                 int patch_w = 0, int patch_h = 0);
// k_linear_t2.hip: the DMA-fed two-fp16-term Linear on "terms rows" and the fp32 -> terms conversion
hipError_t launch_rows_to_terms(const float *x, int64_t m, int k, int64_t ldx, float scale, void *xt, hipStream_t st);
hipError_t launch_linear_t2(const void *xt, int64_t m, int k, const void *wt, const float *bias, int n, int act,
                            const float *res, const float *gamma, float out_scale, float *y, void *yt, float y_scale,
                            void *workspace, size_t workspace_bytes, hipStream_t st);
size_t linear_t2_workspace_bytes(int64_t m, int k, int n);
hipError_t launch_patchify(const float *x, int64_t n, int c, int h, int w, int p, const float *gamma, const float *beta,
                           float eps, float *out, int kpad, hipStream_t st);
hipError_t launch_attention_small(const float *q, int64_t q_rs, const float *k, const float *v, int64_t kv_rs,
                                  const uint8_t *key_mask, int64_t batch, int heads, int head_dim, int nq, int nk,
                                  float scale, float *out, hipStream_t st);

// k_conv3x3_d2h.hip, second kernel: the input already split into fp16 terms by launch_conv1x1_h2(.., y_inv_out != null)
// pool_out != nullptr (sides 56 / 28 / 14, strip kernel only -- ask conv3x3_takes_small first): the launch also writes
// avgpool2x2(relu(v * pool_sc[oc] + pool_sh[oc])) of its 32 output channels to pool_out[image * pool_bs + oc * (side/2)^2 + ..]
hipError_t launch_conv3x3_d2p(const uint16_t *yt, const uint16_t *w2, const float *oscale, int64_t n, int side, float *out,
                              int64_t out_bs, const float *in_inv, float *out_range, int64_t out_ps, hipStream_t st,
                              const float *pool_sc = nullptr, const float *pool_sh = nullptr, float *pool_out = nullptr,
                              int64_t pool_bs = 0);
bool conv3x3_takes_small(int64_t n, int side);

// k_conv3x3_d2s.hip: the same contract for small launches (one wave per 32 output pixels, no LDS); bit-identical results
hipError_t launch_conv3x3_d2s(const uint16_t *yt, const uint16_t *w2, const float *oscale, int64_t n, int side, float *out,
                              int64_t out_bs, const float *in_inv, float *out_range, int64_t out_ps, hipStream_t st);
void set_conv3x3_small_max_wg(int v);      // mirx_set_tuning(MIRX_TUNE_CONV3X3_SMALL_MAX_WG)
int conv3x3_small_max_wg();

// ---- k_attention.hip --------------------------------------------------------------------
hipError_t launch_attention(const float *qkv, int64_t batch, int n, int heads, int head_dim, float scale, float *out,
                            hipStream_t st);
// ---- k_attention_split.hip: the same attention on 16-bit MFMA terms, one kernel template for both schemes (head_dim 32 / 64 /
// 72 / 96; one image's qkv rows below 2 GiB) -- _s3: three bf16 terms per operand
hipError_t launch_attention_s3(const float *qkv, int64_t batch, int n, int heads, int head_dim, float scale, float *out,
                               hipStream_t st);
// _h2: two fp16 terms per operand (caller-supplied bounds), fp32 rows or terms rows out
hipError_t launch_attention_h2(const float *qkv, int64_t batch, int n, int heads, int head_dim, float scale,
                               float qk_bound, float v_bound, float *out, hipStream_t st, void *out_terms = nullptr, float terms_scale = 1.f);

// ---- k_metrics.hip ----------------------------------------------------------------------
constexpr int MIRX_MAX_KAPPAS = 8;
struct RankMetricsArgs {
    const int64_t *ranks;          // [nq, row_stride >= n] gallery row ids, best first
    int64_t nq, n, row_stride;
    const int64_t *gallery_labels; // [n_labels] class id, or multi-hot bit mask (rel_kind 1)
    int64_t n_labels;
    const int64_t *query_labels;   // [nq]
    const int64_t *query_ids;      // [nq] id that is never relevant for the query, or null
    int drop_self;                 // 1: that entry is also taken out of the list (later ranks move up)
    double jaccard_threshold;
    int32_t kappas[MIRX_MAX_KAPPAS];
    int nk;
    double *out_ap;                // [nq]
    int64_t *out_cnt;              // [nq, nk]
    int64_t *out_nrel, *out_maxpos;
    // leave-group-out (mirx_rank_metrics_grouped): read by the CODES instantiations only, which launch_rank_metrics picks when
    // gallery_codes is set.  An entry whose id carries the query's code leaves the list like a dropped self entry.
    const int32_t *gallery_codes;  // [n_labels] by id, or null
    const int32_t *query_codes;    // [nq]; negative = the query leaves nothing out
};
hipError_t launch_rank_metrics(const RankMetricsArgs &a, int rel_kind, int ap_kind, hipStream_t st);

// The same walk over the radix ranking's row payload (mirx_index_rank_metrics), parallel along the list: every query's list of
// n rows is cut into segments of rank_walk_segment(n) entries, a multiple of 4096 that keeps the segments at or below 1024.
// launch_rank_walk runs three passes:
//   count    per (query, segment): entries taken out and relevant entries                                -> seg_cnt
//   terms    per (query, segment): the AP terms, the per-kappa hits and the last relevant position of the segment, from the
//            counts of the segments before it                                                            -> seg_ap, seg_max, out_cnt
//   finish   one wavefront per query adds the segments' partials in a fixed order                        -> out_ap, out_nrel, out_maxpos
// Every floating-point sum's order depends on n alone; out_cnt is zeroed first and added to with integer atomics.
struct RankWalkArgs {
    const int32_t *pay;            // [nq, n] rows, best first (RadixBatch::pa)
    int64_t n;                     // rows per list
    int nq;                        // lists of this batch
    const int64_t *ids;            // [n] id of a row
    const int64_t *exclude;        // [nq] or null
    int self_kind;                 // 0: the excluded row is an ordinary entry, 1: never relevant, 2: also taken out
    const int64_t *row_labels;     // [n] by row
    const int64_t *query_labels;   // [nq]
    const int32_t *row_codes;      // [n] by row, or null
    const int32_t *query_codes;    // [nq], or null
    double jaccard_threshold;
    int32_t kappas[MIRX_MAX_KAPPAS];
    int nk;
    int64_t seg_len;               // rank_walk_segment(n)
    int nseg;                      // ceil(n / seg_len)
    int32_t *seg_cnt;              // [nq, nseg, 2] taken out, relevant
    double *seg_ap;                // [nq, nseg]
    int64_t *seg_max;              // [nq, nseg] largest 1-based relevant position of the segment, 0 = none
    double *out_ap;                // [nq]
    unsigned long long *out_cnt;   // [nq, nk]
    int64_t *out_nrel, *out_maxpos;
};
int64_t rank_walk_segment(int64_t n);
size_t rank_walk_workspace_bytes(int64_t per, int64_t n);   // seg_cnt, seg_ap, seg_max of `per` lists, each 256-byte aligned
void rank_walk_carve(RankWalkArgs &a, void *workspace, int64_t per);   // fills seg_len, nseg and the three pointers from a.n
hipError_t launch_rank_walk(const RankWalkArgs &a, int rel_kind, int ap_kind, hipStream_t st);

// ---- k_gemm.hip -------------------------------------------------------------------------
// The per-query candidate lists the filter GEMM fills and the finalize kernels (k_finalize.hip, k_range.hip) read through
// gather_cands (mirx_device.h).  The readers' argument structs embed it and take it from GemmArgs::lists().
struct CandLists {
    int regions, slots;    // producer regions per query (<= DEEP_MAX_REGIONS) and slots per region (gemm_plan / gemm_plan_deep)
    const int *region_cnt; // [nq_pad, regions]  rows that passed, per region
    const Cand *cand;      // [nq_pad, regions, slots]
    const int *ovf_cnt;    // [nq_pad]
    const Cand *ovf;       // [nq_pad, CAND_OVF]
};
// The GEMM keeps the six fields as its own members, where they have always been: embedding CandLists moved them in the kernel
// arguments, k_gemm16 was compiled to other registers and its filter pass measured 1.2 % slower (profiles/r31).
struct GemmArgs {
    const uint16_t *g16;   // gallery bf16 [rows, dimp]
    const uint16_t *q16;   // queries bf16 [nq_pad, dimp]
    const float *gbias;    // per-row bias (metric 1) or null
    int64_t n_rows;        // valid gallery rows (filter mode) / sampled rows (group-max mode)
    int64_t row_stride;    // gallery row step between consecutive tile rows (1 = dense)
    int64_t nq_pad;        // multiple of the query tile
    int dimp;
    // filter mode: every (query, producer wave) owns a private region of `slots` entries, so
    // the epilogue appends with plain stores; rows beyond a region go to a shared overflow list
    const float *tau;      // [nq_pad]
    int regions, slots;    // producer regions per query and slots per region (from gemm_plan)
    int nph;               // phases per query tile (filled by the launcher)
    int *region_cnt;       // [nq_pad, regions]  rows that passed, per region (zeroed per search)
    Cand *cand;            // [nq_pad, regions, slots]
    int *ovf_cnt;          // [nq_pad]           (zeroed per search)
    Cand *ovf;             // [nq_pad, CAND_OVF]
    void *spill;           // gemm_spill_bytes(): per-wave overflow area of the 256-query kernel's candidate rings
    // group-max mode
    float *groupmax;       // [nq_pad, ngroups]
    int ngroups;
    CandLists lists() const { return CandLists{regions, slots, region_cnt, cand, ovf_cnt, ovf}; }
};
int gemm_query_tile(int64_t nq);                 // query-tile width chosen for nq (64/128/256)
// Producer regions per query and slots per region of the filter GEMM for this problem.
void gemm_plan(int64_t n_rows, int64_t nq_pad, int bn, int *regions, int *slots);
// The deep route's plan: the same regions with about 2 * DEEP_CAP slots per query (at least DEEP_MIN_SLOTS per region).  The
// launcher accepts either plan's (regions, slots) pair; the kernels read the slots at run time.
void gemm_plan_deep(int64_t n_rows, int64_t nq_pad, int bn, int *regions, int *slots);
size_t gemm_spill_bytes();                       // workspace the filter GEMM needs behind GemmArgs::spill
int gemm_groups_per_tile(int bn);                // group-max groups per 256-row gallery tile
hipError_t launch_gemm_filter(const GemmArgs &a, int bn, hipStream_t st);
hipError_t launch_gemm_groupmax(const GemmArgs &a, int bn, hipStream_t st);

// ---- k_finalize.hip ---------------------------------------------------------------------
struct FinalizeArgs {
    const float *q32p;       // [nq, dimp]
    const float *qnorm;      // [nq]
    const float *g32;        // [rows, dimp]
    const int64_t *ids;      // [rows]
    const unsigned *gnorm_max_bits;
    const float *tau;
    CandLists lists;
    const int64_t *exclude;  // or null
    int64_t n_rows;
    int dimp, k, metric, nq;
    double *out_f64;         // [nq, k]
    int64_t *out_ids;        // [nq, k]
    float *out_val;          // [nq, k]
    int32_t *fail_list;      // [nq]   queries for the exact scan (original query numbers)
    int *fail_count;         // [2]    [0] exact list length, [1] retry list length
    // second chance (pass 1 only; null in the retry pass): a query whose guard failed only because
    // tau was too high is re-filtered with tau2 = kth(s~) - 2*eps, which is complete by construction
    int32_t *retry_list;     // [nq]
    float *tau2;             // [nq]
    // retry pass: slot i of the candidate buffers / tau belongs to original query qmap[i]
    const int32_t *qmap;     // or null (identity)
    mirx_search_stats *stats;  // device copy
    // leave-group-out (mirx_index_search_leave_out): read by the CODES instantiations only, which launch_finalize picks when
    // row_codes is set
    const int32_t *row_codes;    // [rows], or null
    const int32_t *query_codes;  // [nq] by original query number
};
// q16r[i] = q16[list[i]] for i < n, zero rows and tau = +inf up to n_pad (retry pass input).
hipError_t launch_gather_queries(const uint16_t *q16, const float *tau2, const int32_t *list, int n,
                                 int64_t n_pad, int dimp, uint16_t *q16r, float *taur, hipStream_t st);
hipError_t launch_select_tau(const float *groupmax, int ngroups, int64_t nq, int64_t nq_pad,
                             int rank_j, float *tau, hipStream_t st);
// One kernel, two capacities: up to CAND_CAP candidates per query on 256 threads, or with `deep` (the deep route's candidate
// buffers, gemm_plan_deep) up to DEEP_CAP on 1024.  1 <= regions <= DEEP_MAX_REGIONS, slots >= 1, 1 <= k <= MAX_K.
hipError_t launch_finalize(const FinalizeArgs &a, bool deep, hipStream_t st);

// ---- k_range.hip: range search (mirx_index_range_search): every row with lo < s <= hi, per query, best first -------------------
constexpr int RANGE_CAP = CAND_CAP + CAND_OVF;   // most candidates the filter route re-scores per query; more -> exact route
// tau[q] of the filter GEMM from the lower bound: below lo' - eps, rounded down; +inf for the padding queries
hipError_t launch_range_tau(const float *q32p, const float *qnorm, const unsigned *gnorm_max_bits, double lo, int dimp, int metric,
                            int64_t nq, int64_t nq_pad, float *tau, hipStream_t st);
struct RangeFinalizeArgs {
    const float *q32p;       // [nq, dimp]
    const float *g32;        // [rows, dimp]
    const int64_t *ids;      // [rows]
    CandLists lists;         // the filter GEMM's candidate buffers, as in FinalizeArgs
    const int64_t *exclude;  // [nq] or null
    const uint8_t *allow;    // [rows] or null
    int64_t n_rows;
    int dimp, metric, nq;
    double lo, hi;
    Hit *stage;              // [nq, RANGE_CAP]   the query's hits, best first
    int32_t *count;          // [nq]              hits of the query (0 for a failed query)
    int32_t *fail_list;      // [nq]              queries whose candidates overflowed: the exact route answers them
    int *fail_count;         // [1]
    unsigned long long *stats;   // [2]           queries answered here, candidates gathered
};
hipError_t launch_range_finalize(const RangeFinalizeArgs &a, hipStream_t st);
// out[i] = exclude[list[i]]
hipError_t launch_range_gather_exclude(const int64_t *exclude, const int32_t *list, int n, int64_t *out, hipStream_t st);
// sorted keys [nq, n]: segment i's hits are the positions [first[i], first[i] + count[qx]) whose score s has lo < s <= hi;
// qx = list ? list[i] : q_first + i in this and the two below
hipError_t launch_range_cut(const uint64_t *keys, int64_t n, int nq, double lo, double hi, const int32_t *list, int64_t q_first,
                            int32_t *first, int32_t *count, hipStream_t st);
// exclusive scan of count[qx], i < m: off[qx] = base + the sum in front of i; tail_or_null[0] = total_out[0] = base + the sum
hipError_t launch_range_scan(const int32_t *count, const int32_t *list, int64_t q_first, int m, int64_t base, int64_t *off,
                             int64_t *tail_or_null, int64_t *total_out, hipStream_t st);
// the cut's hits as (score, id) records at seg + off[qx], in sorted order
hipError_t launch_range_emit(const int32_t *pay, int64_t n, const double *scores, int64_t ld, const int64_t *ids, int nq,
                             const int32_t *list, int64_t q_first, const int32_t *first, const int32_t *count, const int64_t *off,
                             Hit *seg, hipStream_t st);
// CSR assembly: query i's count[i] records -> out + lims[i], from seg + xoff[i] when xoff[i] >= 0, else from its staging row
hipError_t launch_range_compact(const Hit *stage, const Hit *seg, const int64_t *xoff, const int32_t *count, const int64_t *lims,
                                int nq, Hit *out, hipStream_t st);
// the records as the caller's arrays: fp32 reported values and / or fp64 ranking scores, ids
hipError_t launch_range_fetch(const Hit *res, int64_t total, int metric, float *out_val, double *out_f64, int64_t *out_ids,
                              hipStream_t st);

// ---- k_group.hip: grouping search (mirx_group_walk / mirx_group_count / mirx_index_group_fill) -----------------------------
struct GroupWalkArgs {
    const int64_t *ranks;        // [nq, row_stride >= depth] ranked ids, best first; a -1 ends the ranking
    const int64_t *table_index;  // laid out alike: the entry's index into group_of, or null when the id is that index
    const double *scores;        // laid out alike, or null
    int64_t nq, depth, row_stride;
    const int64_t *group_of;     // [n_table] group code per entry
    int64_t n_table;
    const int64_t *group_rows;   // [n_groups] eligible rows per code
    int64_t n_groups, live_groups;
    const int64_t *excl_group;   // [nq] code of the query's excluded row or -1; or null
    int limit, group_size;
    int table;                   // slots of the hash table (filled by the launcher: group_walk_table(limit))
    int64_t *out_ids;            // [nq, limit, group_size]
    double *out_scores;          // alike, or null
    int64_t *out_codes;          // [nq, limit]
    int32_t *out_kept;           // [nq, limit]
    int32_t *out_state;          // [nq, 2]: groups open; bit 0 complete, bit 1 groups final
};
// why mirx_group_walk / mirx_index_group_fill refuse (limit, group_size), or null
inline const char *group_limits(int limit, int group_size) {
    if (limit < 1 || limit > MIRX_GROUP_MAX_LIMIT) return "limit must be in [1, 1024]";
    if (group_size < 1 || group_size > MIRX_GROUP_MAX_SIZE) return "group_size must be in [1, 64]";
    if ((int64_t)limit * group_size > MIRX_GROUP_MAX_HITS) return "limit * group_size must not exceed 16384";
    return nullptr;
}
int group_walk_table(int limit);                 // power of two >= max(64, 2 * limit)
hipError_t launch_group_walk(const GroupWalkArgs &a, hipStream_t st);
// counts[c] += the rows r < n with groups[r] == c and allow[r] != 0 (allow null = every row); codes outside [0, n_groups) are skipped
hipError_t launch_group_count(const int64_t *groups, const uint8_t *allow, int64_t n, int64_t n_groups, int64_t *counts, hipStream_t st);
struct GroupFillArgs {
    const float *q32p;           // [nq, dimp] prepared queries
    const float *g32;            // [n_rows, dimp]
    const int64_t *ids;          // [n_rows]
    const int64_t *exclude;      // [nq] or null
    int64_t nq, n_rows;
    int dimp, limit, group_size;
    const int64_t *pair_query, *pair_slot, *pair_first, *pair_len;   // [n_pairs]: members[first .. first + len) are the group's rows
    int64_t n_pairs;
    const int64_t *members;      // [n_members] row positions
    int64_t n_members;
    int max_members;             // >= every pair_len (sizes the LDS; a longer span is cut to it)
    int64_t *out_ids;            // [nq, limit, group_size]
    double *out_f64;             // alike
};
hipError_t launch_group_fill(const GroupFillArgs &a, int metric, hipStream_t st);

// ---- k_ivf.hip: the IVF_FLAT index (mirx_ivf_*): layout moves, the k-means update, the inverted probe table, the list scan --------
constexpr int IVF_ROWS = 256;                    // rows of a list per work item of the list scan (64 per wave, 4 waves)
constexpr int IVF_LDS_BYTES = 64 * 1024;         // the item's queries as doubles: two workgroups fit a CU's 160 KiB
int ivf_query_tile(int dimp);                    // queries per work item: min(16, IVF_LDS_BYTES / (8 dimp))
// dst row (dst_pos ? dst_pos[i] : i) = the first `cols` floats of src row (src_pos ? src_pos[i] : i), zeros up to dst_ld; a negative
// dst_pos drops the row.  src and dst must not overlap.
hipError_t launch_ivf_place(const float *src, int64_t n, int src_ld, int cols, const int64_t *src_pos, const int64_t *dst_pos,
                            float *dst, int dst_ld, hipStream_t st);
hipError_t launch_ivf_place_ids(const int64_t *src, int64_t n, const int64_t *dst_pos, int64_t *dst, hipStream_t st);
// the same move for IVF_SQ8's code rows of ld bytes (a multiple of 4): dst row dst_pos[i] = src row i, a negative dst_pos drops it
hipError_t launch_ivf_place_codes(const uint8_t *src, int64_t n, int ld, const int64_t *dst_pos, uint8_t *dst, hipStream_t st);
// IVF_SQ8's quantiser (include/mirx.h).  range: vmin / scale [dimp] from rows [n, dim], n >= 1, part = scratch of
// sq8_minmax_parts(n) * 2 * dim floats; encode_place: rows [n, cols] -> code rows of dst_ld bytes (a multiple of 4, zero codes
// past cols) at dst row (dst_pos ? dst_pos[i] : i); decode: code rows of src_ld bytes -> fp32 [n, cols].
int sq8_minmax_parts(int64_t n);
hipError_t launch_sq8_range(const float *rows, int64_t n, int dim, int dimp, float *part, float *vmin, float *scale,
                            hipStream_t st);
hipError_t launch_sq8_encode_place(const float *src, int64_t n, int cols, const float *vmin, const float *scale,
                                   const int64_t *dst_pos, uint8_t *dst, int dst_ld, hipStream_t st);
hipError_t launch_sq8_decode(const uint8_t *src, int64_t n, int src_ld, int cols, const float *vmin, const float *scale,
                             float *dst, hipStream_t st);
// One Lloyd update.  order = the training rows sorted by list (stable), loff[nlist + 1] = where each list starts in it.  cent[l] =
// fp32(sum in fp64, ascending row order / count), then normalised as launch_l2_normalize does when `normalize`; an empty list keeps
// its centroid.  upd = scratch [nlist, dim].
hipError_t launch_ivf_update(const float *rows, int dim, const int32_t *order, const int64_t *loff, int nlist, float *cent,
                             float *upd, bool normalize, hipStream_t st);
// pids [nq, nprobe] (the centroid index's search result) -> probes (int32, also to out_probes when set), qoff [nq, nprobe + 1] =
// each probed list's offset in the query's compact score row, and the table in list order: list l's pairs are the slots
// pairoff[l] .. pairoff[l + 1] of pair_q (the query) / pair_off (its qoff entry), its work items itemoff[l] .. itemoff[l + 1].
// cnt_cursor = 2 nlist ints of scratch; stats[0..2] += rows scored, pairs, work items.
hipError_t launch_ivf_invert(const int64_t *pids, int nq, int nprobe, const int64_t *offsets, int nlist, int qt, int32_t *probes,
                             int32_t *out_probes, int32_t *qoff, int *cnt_cursor, int32_t *pairoff, int32_t *itemoff,
                             int32_t *pair_q, int32_t *pair_off, unsigned long long *stats, hipStream_t st);
struct IvfScoreArgs {
    const float *q32p;           // [nq, dimp] the batch's queries, zero padded
    const void *rows;            // [size, dimp] list-major: fp32, or 8-bit codes when vmin is set
    const float *vmin, *scale;   // [dimp] IVF_SQ8's range, zero in the padding; both null for fp32 rows
    int dimp, nlist, qt;
    const int64_t *offsets;      // [nlist + 1]
    const int32_t *pairoff, *itemoff, *pair_q, *pair_off;   // launch_ivf_invert's
    double *out;                 // [nq, ld] compact score rows
    int64_t ld;
};
hipError_t launch_ivf_scores(const IvfScoreArgs &a, int metric, hipStream_t st);
// per query: the best k of its compact row by (score desc, id asc), ids taken from the probed lists, exclude[i] skipped
hipError_t launch_ivf_topk(const double *scores, int64_t ld, const int32_t *probes, const int32_t *qoff, int nq, int nprobe,
                           const int64_t *offsets, const int64_t *ids, const int64_t *exclude, int k, int metric, double *out_f64,
                           int64_t *out_ids, float *out_val, hipStream_t st);
// launch_ivf_invert's first step alone: probes, out_probes and qoff as there, cnt[nlist] = how many of the nq queries probe each list
hipError_t launch_ivf_probes(const int64_t *pids, int nq, int nprobe, const int64_t *offsets, int nlist, int32_t *probes,
                             int32_t *out_probes, int32_t *qoff, int *cnt, hipStream_t st);

// ---- k_ivf_pq.hip: IVF_PQ (mirx_ivf_create_pq): a query's ADC tables, the scan of the probed lists' code rows, code moves ------
constexpr int PQ_MAX_M = 64;                     // sub-quantisers: a query's table is m x 256 doubles, 128 KiB of LDS at 64
constexpr int PQ_MAX_DSUB = 512;                 // columns of a sub-space: MIRX_IVF_MAX_DIM / 4
constexpr int PQ_ITEM_ROWS = 1024;               // entries of a compact score row per work item of the scan: one per thread
constexpr int PQ_CU_LDS_BYTES = 160 * 1024;
// out[q][j][c] (fp64) = the score of q's sub-vector j against codeword c of cb [m][256][dim / m]: one sequential accumulator over
// the columns, IP: + q * c (exact product); L2: d = q - c, + (d * d) with the product rounded before the addition
hipError_t launch_pq_tables(const float *q, int64_t nq, int dim, int m, int metric, const float *cb, double *out, hipStream_t st);
// itemoff[nq + 1] = exclusive scan of ceil(qoff[q][nprobe] / PQ_ITEM_ROWS); stats[0..2] += entries, sum of cnt[nlist], items
hipError_t launch_pq_items(const int32_t *qoff, int nq, int nprobe, const int *cnt, int nlist, int32_t *itemoff,
                           unsigned long long *stats, hipStream_t st);
struct PqScanArgs {
    const double *tables;        // [nq, m, 256] launch_pq_tables'
    const uint8_t *codes;        // [size, m] list-major code rows
    int m, nq, nprobe;
    const int32_t *probes, *qoff;   // launch_ivf_probes'
    const int64_t *offsets;      // [nlist + 1]
    const int32_t *itemoff;      // launch_pq_items'
    double *out;                 // [nq, ld] compact score rows: entry e of query q = sum over j ascending of T[q][j][code[j]], negated for L2
    int64_t ld;
    // residual coding (mirx_ivf_create_pq_ex, by_residual = 1), all null otherwise: tables are then the IP tables of the residual
    // codebooks for BOTH metrics, an entry's sum starts from base[q * nprobe + slot], and L2 ranks by -((qq[q] + n2[pos]) - 2 ip)
    const double *base;          // [nq, nprobe] launch_pq_base's
    const double *qq;            // [nq] launch_pq_base's (L2)
    const double *n2;            // [size] list-major, launch_pq_norms' (L2)
};
hipError_t launch_pq_scan(const PqScanArgs &a, int metric, hipStream_t st);
// codes[i * m + j] = (uint8)found[i]: the codeword search of sub-space j written into the code rows
hipError_t launch_pq_pack(const int64_t *found, int64_t n, int m, int j, uint8_t *codes, hipStream_t st);
// dst [n, dim] = each row's m codewords, concatenated
hipError_t launch_pq_decode(const uint8_t *codes, int64_t n, int dim, int m, const float *cb, float *dst, hipStream_t st);
// residual coding.  residual: dst[i * dst_ld + e] = rows[i * dim + col0 + e] - cent[lists[i] * dim + col0 + e], e < cols, one fp32
// rounding; a list outside 0 .. nlist-1 gives NaN and reads nothing
hipError_t launch_pq_residual(const float *rows, int64_t n, int dim, int col0, int cols, const int64_t *lists, const float *cent,
                              int nlist, float *dst, int dst_ld, hipStream_t st);
// base[q][s] = sum over j ascending of P_j, P_j one sequential fp64 accumulator of (double)q_e * (double)c_e over sub-space j's
// columns of centroid lists[q][s] (a list outside 0 .. nlist-1: 0.0); qq_or_null[q] = the same two-level sum of q_e * q_e
hipError_t launch_pq_base(const float *q, int64_t nq, int dim, int m, const int32_t *lists, int nprobe, const float *cent, int nlist,
                          double *base, double *qq_or_null, hipStream_t st);
// n2[i] = the two-level sum of xh_e * xh_e (product rounded, then added), xh_e = (double)cent[lists[i]][e] + (double)codeword_e
hipError_t launch_pq_norms(const uint8_t *codes, int64_t n, int dim, int m, const int64_t *lists, const float *cent, int nlist,
                           const float *cb, double *n2, hipStream_t st);
// dst [n, dim] = (float)(centroid of the row's list + its codewords), one fp32 rounding per column; lists [n] as
// launch_pq_residual's (outside 0 .. nlist-1: NaN)
hipError_t launch_pq_decode_residual(const uint8_t *codes, int64_t n, int dim, int m, const float *cb, const int64_t *lists,
                                     const float *cent, int nlist, float *dst, hipStream_t st);

// ---- k_fuse.hip: hybrid search's rank / score fusion (mirx_fuse_ranked) ------------------------------------------------------
struct FuseArgs {
    const int64_t *codes;        // [nq, row_stride >= m] document codes of the concatenated lists, -1 = empty slot
    const float *distances;      // laid out alike
    int64_t nq, row_stride, n_codes;
    int m, n_requests;           // m = offsets[n_requests] <= MIRX_FUSE_MAX_ENTRIES
    int offsets[MIRX_FUSE_MAX_REQUESTS + 1];   // request r owns positions [offsets[r], offsets[r + 1])
    int ranker;                  // MIRX_FUSE_RRF / MIRX_FUSE_WEIGHTED
    int limit;
    double rrf_k;
    double weights[MIRX_FUSE_MAX_REQUESTS];
    int norms[MIRX_FUSE_MAX_REQUESTS];         // MIRX_FUSE_NORM_* per request
    int64_t *out_codes;          // [nq, limit], -1 past the documents
    double *out_scores;          // [nq, limit], -inf past the documents
    int32_t *out_request;        // [nq, limit] request and slot of the document's first entry, -1 past the documents
    int32_t *out_slot;
    int32_t *out_count;          // [nq] = min(limit, distinct documents)
};
int fuse_sort_width(int m);                      // power of two >= m: the slots of the LDS sorts, 16 bytes each
hipError_t launch_fuse_ranked(const FuseArgs &a, hipStream_t st);

// ---- k_conv_t2.hip: ResNet-50's convolutions on channels-last terms rows (mirx_conv_terms) and their glue ------------------
hipError_t launch_conv_t2(const void *xt, const float *x_scale, const float *x_range, int64_t n, int h, int w, int cin, int ksz,
                          int stride, const void *wt, const float *oscale, const float *bias, int cout, float w_abs_sum,
                          float bias_abs_max, const void *rt, const float *r_scale, const float *r_range, int relu, void *yt,
                          float *y_scale, float *y, float *out_range, hipStream_t st);
hipError_t launch_nchw_to_terms(const float *x, int64_t xbs, int64_t n, int c, int hw, const float *range, float *scale_row,
                                void *xt, hipStream_t st);
hipError_t launch_gap_nhwc(const float *x, int64_t n, int hw, int c, int normalize, float *y, hipStream_t st);

// ---- k_attention_win.hip / k_swin.hip: SwinV2's shifted-window cosine attention and its res-post-norm / merge glue ----------
hipError_t launch_attention_win(const float *qkv, int64_t n, int side, int window, int shift, int heads, const float *bias_tab,
                                const float *lscale, float *out, void *out_t, float t_scale, hipStream_t st);
hipError_t launch_postnorm_rows(const float *x, const float *y, int64_t m, int c, const float *gamma, const float *beta, float eps,
                                float *out, void *out_t, float scale, hipStream_t st);
hipError_t launch_patch_merge(const float *x, int64_t n, int h, int w, int c, float scale, void *out_t, hipStream_t st);

// ---- k_attnpool.hip: the SRA / PCAM attention-pooling heads on channels-last rows, one workgroup per image ------------------
hipError_t launch_sra_head(const float *x, int64_t n, int hw, int c, const float *w, int K, const float *gamma, const float *beta,
                           float eps, float lam, int normalize, float *y, hipStream_t st);
hipError_t launch_pcam_head(const float *x, int64_t n, int hw, int c, const float *w, const float *b, int K, const float *gamma,
                            const float *beta, float eps, float lam, int normalize, float *feat, float *logits, hipStream_t st);

}  // namespace mirx
