// mirx_api.hip -- the stateless half of the C ABI (include/mirx.h): the error plumbing and the one-launch wrappers, which check
// their arguments and call one launcher each.  The index object and every mirx_index_* entry point are in mirx_index.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mirx_kernels.h"

namespace mirx {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// The routing constants of the search in mirx_index.hip (declared in mirx_kernels.h).  They are defined here because the tests
// follow the library's capacities by reading `constexpr <type> NAME = <value>;` out of this file.
constexpr int64_t QUERY_BATCH = 8192;          // queries per internal pass
constexpr int64_t TIER1_MIN_ROWS = 32768;      // below this the exact scan answers directly
constexpr int TIER1_MAX_K = 64;                // the most k (+ 1 with excluded ids) the candidate lists answer

}  // namespace mirx

using namespace mirx;

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

int mirx_compact_tile(void) { return COMPACT_TILE; }
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

// mirx_rank_metrics and mirx_rank_metrics_grouped: codes = true checks and passes the two code arrays.
static int rank_metrics_impl(const char *who, const int64_t *ranks, int64_t nq, int64_t n, int64_t row_stride,
                             const int64_t *gallery_labels, int64_t n_labels, const int64_t *query_labels,
                             const int64_t *query_ids_or_null, int drop_self, int rel_kind, double jaccard_threshold,
                             int ap_kind, const int32_t *kappas, int nk, bool codes, const int32_t *gallery_codes,
                             const int32_t *query_codes, double *out_ap, int64_t *out_cnt, int64_t *out_nrel,
                             int64_t *out_maxpos, void *stream) {
    const std::string w(who);
    MIRX_CHECK(nq >= 0 && n >= 0 && row_stride >= n && n_labels >= 0, w + ": bad sizes");
    MIRX_CHECK(nq == 0 || (ranks && gallery_labels && query_labels && out_ap && out_nrel && out_maxpos), w + ": null buffer");
    MIRX_CHECK(!codes || (gallery_codes && query_codes), w + ": null codes");
    MIRX_CHECK(nk >= 0 && nk <= MIRX_MAX_KAPPAS && (nk == 0 || (kappas && out_cnt)), w + ": 0 <= nk <= 8");
    MIRX_CHECK((rel_kind == 0 || rel_kind == 1) && (ap_kind == 0 || ap_kind == 1), w + ": bad kind");
    RankMetricsArgs a{};
    a.ranks = ranks; a.nq = nq; a.n = n; a.row_stride = row_stride;
    a.gallery_labels = gallery_labels; a.n_labels = n_labels; a.query_labels = query_labels;
    a.query_ids = query_ids_or_null; a.drop_self = (drop_self && query_ids_or_null) ? 1 : 0;
    a.jaccard_threshold = jaccard_threshold; a.nk = nk;
    for (int j = 0; j < nk; ++j) {
        MIRX_CHECK(kappas[j] >= 1, w + ": kappa must be >= 1");
        a.kappas[j] = kappas[j];
    }
    a.out_ap = out_ap; a.out_cnt = out_cnt; a.out_nrel = out_nrel; a.out_maxpos = out_maxpos;
    if (codes) { a.gallery_codes = gallery_codes; a.query_codes = query_codes; }
    MIRX_HIP(launch_rank_metrics(a, rel_kind, ap_kind, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

int mirx_rank_metrics(const int64_t *ranks, int64_t nq, int64_t n, int64_t row_stride,
                      const int64_t *gallery_labels, int64_t n_labels, const int64_t *query_labels,
                      const int64_t *query_ids_or_null, int drop_self, int rel_kind, double jaccard_threshold,
                      int ap_kind,
                      const int32_t *kappas, int nk, double *out_ap, int64_t *out_cnt, int64_t *out_nrel,
                      int64_t *out_maxpos, void *stream) {
    return rank_metrics_impl("rank_metrics", ranks, nq, n, row_stride, gallery_labels, n_labels, query_labels, query_ids_or_null,
                             drop_self, rel_kind, jaccard_threshold, ap_kind, kappas, nk, false, nullptr, nullptr, out_ap, out_cnt,
                             out_nrel, out_maxpos, stream);
}

int mirx_rank_metrics_grouped(const int64_t *ranks, int64_t nq, int64_t n, int64_t row_stride,
                              const int64_t *gallery_labels, int64_t n_labels, const int64_t *query_labels,
                              const int64_t *query_ids_or_null, int drop_self, int rel_kind, double jaccard_threshold,
                              int ap_kind, const int32_t *kappas, int nk, const int32_t *gallery_codes,
                              const int32_t *query_codes, double *out_ap, int64_t *out_cnt, int64_t *out_nrel,
                              int64_t *out_maxpos, void *stream) {
    return rank_metrics_impl("rank_metrics_grouped", ranks, nq, n, row_stride, gallery_labels, n_labels, query_labels,
                             query_ids_or_null, drop_self, rel_kind, jaccard_threshold, ap_kind, kappas, nk, true, gallery_codes,
                             query_codes, out_ap, out_cnt, out_nrel, out_maxpos, stream);
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
