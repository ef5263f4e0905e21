// k_simatt.hip -- SimAtt similarity-attention saliency (the reference's explanations.py SimAtt) in closed form, on the
// channels-last fp32 rows [B, hw, C] of the LAST feature map of a model whose tail is average pool -> optional fc.  Image 0 is
// the query.  With x_b = fc(mean_pos rows[b]) (the pooled vector itself without fc) and xn_b = x_b / max(|x_b|, 1e-12):
//     wt[d]  = prod over the non-query images j of |xn_0[d] - xn_j[d]|, the first factor replaced by 1 - itself when `positive`
//     g_b[c] = sum_d W[d, c] * sign(x_b[d]) * wt[d] / hw            (W = identity without fc; sign(0) = 0)
//     M_b    = bilinear(relu(sum_c g_b[c] * rows[b, :, c]))         -> [H, W], F.interpolate(align_corners=False)
// g_b / hw is what the reference's autograd.grad of s_b = sum_d |x_b[d]| wt[d] gives at EVERY position of the feature map, so
// no backward pass is needed.  group mode: one wt over all non-query images, out [B, H, W].  pairs mode: retrieval k alone
// against the query (wt_k over image k + 1 only), out [K = B - 1, 2, H, W]: the query's map under pair k, then retrieval k's.
//
//   k_simatt_embed   x_b.  Without fc a thread per channel sums the positions in order.  With fc a workgroup owns 64 embedding
//                    components of one image: the pooled channels are staged through LDS 2048 at a time, a wave owns 16
//                    components, its lanes stride the channels and a butterfly adds the 64 lane sums.
//   k_simatt_maps    one workgroup of 1024 threads per map: the norms (a wave per image, lanes stride D, butterfly), wt (a thread
//                    per component, the images in order), s = sign(x) * wt, g = W^T s (a thread per channel, eight interleaved
//                    partial sums over D), the h x w map (a wave per position, lanes stride C, butterfly) kept in LDS with NaN
//                    passing the clamp, the bilinear upsample straight into the caller's output.
//
// Every sum has an order fixed by C, D and hw alone: x_b depends on image b only, a pairs-mode map on the query and its
// retrieval only, so neither changes with B, K or the place in the batch.  A NaN in image j reaches xn_j, hence every wt that has
// j as a factor: all maps in group mode, pair j - 1's two maps in pairs mode.
#include <cmath>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int SA_ETHREADS = 256;                         // k_simatt_embed: 4 waves
constexpr int SA_DSLICE = 64;                            // embedding components per workgroup
constexpr int SA_DWAVE = SA_DSLICE / (SA_ETHREADS / 64); // ... per wave
constexpr int SA_CCHUNK = 2048;                          // pooled channels staged in LDS at a time
constexpr int SA_MTHREADS = 1024;                        // k_simatt_maps: 16 waves
constexpr int SA_MWAVES = SA_MTHREADS / 64;
constexpr int SA_WT = MIRX_SIMATT_MAX_D / SA_MTHREADS;   // wt components a thread carries
constexpr float SA_NORM_EPS = 1e-12f;                    // F.normalize's eps
static_assert(MIRX_SIMATT_MAX_C <= MIRX_SIMATT_MAX_D, "without fc the embedding is the pooled vector: D = C");

// torch.sign (abs' backward): 0 at 0
__device__ inline float sign0(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }

struct EmbedArgs {
    const float *rows;       // [B, hw, c]
    int64_t hw, c, dx;       // dx: embedding width (d with fc, c without)
    const float *fcw, *fcb;  // [dx, c], [dx]; fcw null = no fc, fcb may be null
    float *x;                // [B, dx]
};

__global__ __launch_bounds__(SA_ETHREADS) void k_simatt_embed(EmbedArgs a) {
    __shared__ float pooled[SA_CCHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.y;
    const float *rb = a.rows + b * a.hw * a.c;
    const float n = (float)a.hw;
    if (!a.fcw) {
        const int64_t ch = (int64_t)blockIdx.x * SA_ETHREADS + tid;
        if (ch < a.c) {
            float sum = 0.f;
            for (int64_t pos = 0; pos < a.hw; ++pos) sum += rb[pos * a.c + ch];
            a.x[b * a.dx + ch] = sum / n;
        }
        return;
    }
    const int64_t d0 = (int64_t)blockIdx.x * SA_DSLICE + wave * SA_DWAVE;
    float acc[SA_DWAVE];
#pragma unroll
    for (int u = 0; u < SA_DWAVE; ++u) acc[u] = 0.f;
    for (int64_t c0 = 0; c0 < a.c; c0 += SA_CCHUNK) {
        const int nc = a.c - c0 < SA_CCHUNK ? (int)(a.c - c0) : SA_CCHUNK;
        for (int i = tid; i < nc; i += SA_ETHREADS) {
            float sum = 0.f;
            for (int64_t pos = 0; pos < a.hw; ++pos) sum += rb[pos * a.c + c0 + i];
            pooled[i] = sum / n;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SA_DWAVE; ++u) {
            if (d0 + u < a.dx) {                                    // wave-uniform
                const float *wrow = a.fcw + (d0 + u) * a.c + c0;
                for (int i = lane; i < nc; i += 64) acc[u] = fmaf(wrow[i], pooled[i], acc[u]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < SA_DWAVE; ++u) {
        if (d0 + u < a.dx) {
            const float v = wave_sum(acc[u]);
            if (lane == 0) a.x[b * a.dx + d0 + u] = a.fcb ? v + a.fcb[d0 + u] : v;
        }
    }
}

struct MapsArgs {
    const float *rows;       // [B, hw, c]
    int64_t b, hw, c, dx;
    int h, w, H, W;
    const float *fcw;        // [dx, c] or null
    const float *x;          // [B, dx]       (k_simatt_embed)
    float *s;                // [maps, dx]    sign(x) * wt, with fc only
    float *g;                // [maps, c]
    int pairs, positive;
    float *out;              // [maps, H, W]
};

// max(|x|, eps) of one embedding, by one wave; a NaN norm stays NaN (clamp_min passes it)
__device__ inline float wave_denominator(const float *x, int64_t dx, int lane) {
    float sq = 0.f;
    for (int64_t d = lane; d < dx; d += 64) sq = fmaf(x[d], x[d], sq);
    const float nrm = sqrtf(wave_sum(sq));
    return (nrm > SA_NORM_EPS || nrm != nrm) ? nrm : SA_NORM_EPS;
}

__global__ __launch_bounds__(SA_MTHREADS) void k_simatt_maps(MapsArgs a) {
    __shared__ float den[1 + SA_MWAVES];       // the query's denominator, then one per image of the current tile of 16
    __shared__ float smap[MIRX_SIMATT_MAX_HW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = blockIdx.x;
    int64_t img, jlo, jhi;                     // this map's image; wt's factors are the images jlo .. jhi - 1
    if (a.pairs) {
        jlo = (m >> 1) + 1;
        jhi = jlo + 1;
        img = (m & 1) ? jlo : 0;
    } else {
        jlo = 1;
        jhi = a.b;
        img = m;
    }
    if (wave == 0) {
        const float dq = wave_denominator(a.x, a.dx, lane);
        if (lane == 0) den[0] = dq;
    }
    float wt[SA_WT];
#pragma unroll
    for (int u = 0; u < SA_WT; ++u) wt[u] = 1.f;
    for (int64_t j0 = jlo; j0 < jhi; j0 += SA_MWAVES) {
        if (j0 + wave < jhi) {                 // wave-uniform
            const float dj = wave_denominator(a.x + (j0 + wave) * a.dx, a.dx, lane);
            if (lane == 0) den[1 + wave] = dj;
        }
        __syncthreads();
        const int nt = jhi - j0 < SA_MWAVES ? (int)(jhi - j0) : SA_MWAVES;
#pragma unroll
        for (int u = 0; u < SA_WT; ++u) {
            const int64_t d = tid + (int64_t)u * SA_MTHREADS;
            if (d < a.dx) {
                const float xq = a.x[d] / den[0];
                for (int t = 0; t < nt; ++t) {
                    float v = fabsf(xq - a.x[(j0 + t) * a.dx + d] / den[1 + t]);
                    if (a.positive && j0 + t == jlo) v = 1.f - v;
                    wt[u] *= v;
                }
            }
        }
        __syncthreads();
    }
    const float n = (float)a.hw;
    const float *xb = a.x + img * a.dx;
    float *gm = a.g + m * a.c;
    if (!a.fcw) {
#pragma unroll
        for (int u = 0; u < SA_WT; ++u) {
            const int64_t d = tid + (int64_t)u * SA_MTHREADS;
            if (d < a.dx) gm[d] = sign0(xb[d]) * wt[u] / n;
        }
    } else {
        float *sm = a.s + m * a.dx;
#pragma unroll
        for (int u = 0; u < SA_WT; ++u) {
            const int64_t d = tid + (int64_t)u * SA_MTHREADS;
            if (d < a.dx) sm[d] = sign0(xb[d]) * wt[u];
        }
        __threadfence_block();
        __syncthreads();
        for (int64_t ch = tid; ch < a.c; ch += SA_MTHREADS) {
            float acc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] = 0.f;
            for (int64_t d = 0; d < a.dx; d += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (d + u < a.dx) acc[u] = fmaf(a.fcw[(d + u) * a.c + ch], sm[d + u], acc[u]);
            }
            gm[ch] = (((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))) / n;
        }
    }
    __threadfence_block();
    __syncthreads();
    const float *rb = a.rows + img * a.hw * a.c;
    for (int64_t pos = wave; pos < a.hw; pos += SA_MWAVES) {
        float acc = 0.f;
        for (int64_t ch = lane; ch < a.c; ch += 64) acc = fmaf(gm[ch], rb[pos * a.c + ch], acc);
        acc = wave_sum(acc);
        if (lane == 0) smap[pos] = relu_nan(acc);
    }
    __syncthreads();
    const float sh = (float)a.h / (float)a.H, sw = (float)a.w / (float)a.W;
    float *out = a.out + m * (int64_t)a.H * a.W;
    const unsigned npix = (unsigned)a.H * (unsigned)a.W, uw = (unsigned)a.W;      // H, W <= 8192: 32-bit index arithmetic
    for (unsigned e = tid; e < npix; e += SA_MTHREADS)
        out[e] = bilinear_half_pixel(smap, a.h, a.w, sh, sw, (int)(e / uw), (int)(e % uw));
}

}  // namespace

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

static const char *simatt_limits(int64_t b, int64_t c, int64_t d, int mode) {
    if (b < 2 || b > MIRX_SIMATT_MAX_B) return "simatt: b must be in [2, 65535]";
    if (c < 1 || c > MIRX_SIMATT_MAX_C) return "simatt: c must be in [1, 16384]";
    if (d < 0 || d > MIRX_SIMATT_MAX_D) return "simatt: d must be in [1, 16384], or 0 without fc";
    if (mode != MIRX_SIMATT_GROUP && mode != MIRX_SIMATT_PAIRS) return "simatt: mode must be 0 (group) or 1 (pairs)";
    return nullptr;
}

static int64_t simatt_maps_of(int64_t b, int mode) { return mode == MIRX_SIMATT_PAIRS ? 2 * (b - 1) : b; }

extern "C" int64_t mirx_simatt_workspace_floats(int64_t b, int64_t c, int64_t d, int mode) {
    if (const char *msg = simatt_limits(b, c, d, mode)) return fail(MIRX_EINVAL, msg);
    const int64_t dx = d ? d : c;
    return b * dx + simatt_maps_of(b, mode) * (c + (d ? d : 0));
}

extern "C" int mirx_simatt(const float *rows, int64_t b, int h, int w, int64_t c, const float *fc_weight, const float *fc_bias,
                           int64_t d, int mode, int positive, int H, int W, float *workspace, int64_t workspace_floats,
                           float *out, void *stream) {
    const int64_t hw = (int64_t)h * w;
    if (h < 1 || w < 1 || hw > MIRX_SIMATT_MAX_HW) return fail(MIRX_EINVAL, "simatt: h, w >= 1 and h * w <= 1024");
    if (const char *msg = simatt_limits(b, c, d, mode)) return fail(MIRX_EINVAL, msg);
    if (H < 1 || W < 1 || H > MIRX_SIMATT_MAX_SIZE || W > MIRX_SIMATT_MAX_SIZE) return fail(MIRX_EINVAL, "simatt: H, W must be in [1, 8192]");
    if (positive != 0 && positive != 1) return fail(MIRX_EINVAL, "simatt: positive must be 0 or 1");
    if ((fc_weight != nullptr) != (d != 0)) return fail(MIRX_EINVAL, "simatt: fc_weight and d > 0 go together (no fc: null and 0)");
    if (fc_bias && !fc_weight) return fail(MIRX_EINVAL, "simatt: fc_bias without fc_weight");
    if (!rows || !workspace || !out) return fail(MIRX_EINVAL, "simatt: null buffer");
    const int64_t dx = d ? d : c, maps = simatt_maps_of(b, mode);
    if (workspace_floats < b * dx + maps * (c + (d ? d : 0))) return fail(MIRX_EINVAL, "simatt: workspace smaller than mirx_simatt_workspace_floats()");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    EmbedArgs ea{rows, hw, c, dx, fc_weight, fc_bias, workspace};
    const unsigned gx = fc_weight ? (unsigned)((dx + SA_DSLICE - 1) / SA_DSLICE) : (unsigned)((c + SA_ETHREADS - 1) / SA_ETHREADS);
    hipLaunchKernelGGL(k_simatt_embed, dim3(gx, (unsigned)b), dim3(SA_ETHREADS), 0, st, ea);
    MIRX_HIP(hipGetLastError());
    MapsArgs ma{};
    ma.rows = rows;
    ma.b = b;
    ma.hw = hw;
    ma.c = c;
    ma.dx = dx;
    ma.h = h;
    ma.w = w;
    ma.H = H;
    ma.W = W;
    ma.fcw = fc_weight;
    ma.x = workspace;
    ma.g = workspace + b * dx;
    ma.s = ma.g + maps * c;
    ma.pairs = mode == MIRX_SIMATT_PAIRS;
    ma.positive = positive;
    ma.out = out;
    hipLaunchKernelGGL(k_simatt_maps, dim3((unsigned)maps), dim3(SA_MTHREADS), 0, st, ma);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}
