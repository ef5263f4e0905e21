// k_attnpool.hip -- the attention-pooling heads of the reference's ConvNeXtV2_SRA and ConvNeXtV2_PCAM (model.py:120-278 there) on
// the backbone's final channels-last residual stream x[n, hw, c] (fp32 rows), one workgroup of 4 waves per image:
//
//   pass A   a wave per pixel (p = wave, wave + 4, ...): the row in registers (lane owns float4 i = lane + 64 j), the K dot
//            products w[k] . row reduced across the wave -> d[k][p] in LDS.  PCAM first LayerNorms the row in place (two-pass
//            mean / variance, as k_layernorm_rows) and keeps the pixel's mean and 1 / std in LDS.
//   middle   a wave per head k: SRA = a softmax over the pixels (max-subtracted, expf); PCAM = sigmoid(d + b), the division by
//            (sum + 1e-8), and logit[k] = b[k] + sum_p q[k][p] d[k][p] (= P[k] . w[k] + b[k] by linearity, so the K x c class
//            pools are never formed); then PCAM's softmax over k in wave 0.  Both heads end in one weight per pixel:
//            SRA  om[p] = (1 / K) sum_k a[k][p];   PCAM  om[p] = sum_k softmax(logit)[k] q[k][p].
//   pass B   a thread per 4 channels: gap = sum_p x[p] and pool = sum_p om[p] x[p] (PCAM: om[p] LN(x[p])) in pixel order, then the
//            LayerNorms over c, y = LN(gap / hw) + lam * (SRA: LN(pool); PCAM: pool), and optionally y / max(||y||, 1e-12).
//
// Every sum has one fixed order per image (lane partials in index order, butterflies, the 4 wave partials as (0 + 1) + (2 + 3)), so
// an image's output bits depend on nothing but its own rows and the weights.  fp32 throughout: the head is ~2 K hw c FLOP per image.
#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int AP_THREADS = 256;

// sum over the workgroup; every thread gets the same value.  red = 4 floats of LDS, free on entry (guarded by the barriers)
__device__ inline float block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ inline float dot4(const f32x4 &a, const f32x4 &b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); }

// LDS (dynamic, floats): d[K * hw] | om[hw] | mu[hw] | rs[hw] | red[4] | kv[64]
// RV: c <= 256 RV (pass A: a wave holds a row as RV float4 per lane); RB = ceil(RV / 4) (pass B: c <= 1024 RB)
template <bool PCAM, int RV>
__global__ __launch_bounds__(AP_THREADS) void k_attnpool(const float *__restrict__ x, int hw, int c, const float *__restrict__ w,
                                                         const float *__restrict__ bias, int K, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, float eps, float lam, int normalize,
                                                         float *__restrict__ y, float *__restrict__ logits_out) {
    constexpr int RB = (RV + 3) / 4;
    extern __shared__ float lds[];
    float *s_d = lds;
    float *s_om = s_d + (size_t)K * hw;
    float *s_mu = s_om + hw;
    float *s_rs = s_mu + hw;
    float *s_red = s_rs + hw;
    float *s_kv = s_red + 4;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nv = c >> 2;
    const float *xb = x + (int64_t)blockIdx.x * hw * c;
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(gamma);
    const f32x4 *b4 = reinterpret_cast<const f32x4 *>(beta);
    const float rc = 1.f / (float)c;

    // ---- pass A: d[k][p] = w[k] . row(p), row(p) = x[p] (SRA) or LN(x[p]) (PCAM) ----
    for (int p = wv; p < hw; p += 4) {
        const f32x4 *xr = reinterpret_cast<const f32x4 *>(xb + (int64_t)p * c);
        f32x4 v[RV];
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            const int i = lane + 64 * j;
            v[j] = i < nv ? xr[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (PCAM) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < RV; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
            const float mean = wave_sum(s) * rc;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < RV; ++j) {
                if (lane + 64 * j < nv) {
                    const f32x4 dd = v[j] - mean;
                    q += dot4(dd, dd);
                }
            }
            const float rstd = 1.0f / sqrtf(wave_sum(q) * rc + eps);
#pragma unroll
            for (int j = 0; j < RV; ++j) {
                const int i = lane + 64 * j;
                if (i < nv) v[j] = (v[j] - mean) * rstd * g4[i] + b4[i];
            }
            if (lane == 0) {
                s_mu[p] = mean;
                s_rs[p] = rstd;
            }
        }
        for (int k = 0; k < K; ++k) {
            const f32x4 *wr = reinterpret_cast<const f32x4 *>(w + (int64_t)k * c);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < RV; ++j) {
                const int i = lane + 64 * j;
                if (i < nv) s += dot4(wr[i], v[j]);
            }
            s = wave_sum(s);
            if (lane == 0) s_d[k * hw + p] = s;
        }
    }
    __syncthreads();

    // ---- middle: per-head weights over the pixels ----
    for (int k = wv; k < K; k += 4) {
        float *dk = s_d + k * hw;
        if (!PCAM) {
            float m = -INFINITY;
            for (int p = lane; p < hw; p += 64) m = fmaxf(m, dk[p]);
            m = wave_fmax(m);
            float s = 0.f;
            for (int p = lane; p < hw; p += 64) {
                const float e = expf(dk[p] - m);
                dk[p] = e;
                s += e;
            }
            const float rs = 1.f / wave_sum(s);
            for (int p = lane; p < hw; p += 64) dk[p] = dk[p] * rs;
        } else {
            const float bk = bias[k];
            float s = 0.f;
            for (int p = lane; p < hw; p += 64) s += 1.f / (1.f + expf(-(dk[p] + bk)));
            const float den = wave_sum(s) + 1e-8f;
            float l = 0.f;
            for (int p = lane; p < hw; p += 64) {
                const float qn = (1.f / (1.f + expf(-(dk[p] + bk)))) / den;
                l += qn * dk[p];
                dk[p] = qn;
            }
            l = wave_sum(l);
            if (lane == 0) s_kv[k] = l + bk;
        }
    }
    __syncthreads();
    if (PCAM && wv == 0) {                        // softmax over the K <= 64 class logits, lane = class
        const float l = lane < K ? s_kv[lane] : -INFINITY;
        const float m = wave_fmax(l);
        const float e = lane < K ? expf(l - m) : 0.f;
        const float s = wave_sum(e);
        if (logits_out && lane < K) logits_out[(int64_t)blockIdx.x * K + lane] = l;
        if (lane < K) s_kv[lane] = e / s;         // (each lane overwrites only the slot it read)
    }
    __syncthreads();
    for (int p = tid; p < hw; p += AP_THREADS) {
        float s = 0.f;
        if (PCAM) {
            for (int k = 0; k < K; ++k) s += s_kv[k] * s_d[k * hw + p];
        } else {
            for (int k = 0; k < K; ++k) s += s_d[k * hw + p];
            s = s / (float)K;
        }
        s_om[p] = s;
    }
    __syncthreads();

    // ---- pass B: the pools over the pixels, a thread per float4 of channels ----
    f32x4 gp[RB], ap[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) gp[j] = ap[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < hw; ++p) {
        const f32x4 *xr = reinterpret_cast<const f32x4 *>(xb + (int64_t)p * c);
        const float om = s_om[p];
        float mu = 0.f, rs = 0.f;
        if (PCAM) {
            mu = s_mu[p];
            rs = s_rs[p];
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int i = tid + AP_THREADS * j;
            if (i < nv) {
                const f32x4 xv = xr[i];
                gp[j] += xv;
                if (PCAM)
                    ap[j] += om * ((xv - mu) * rs * g4[i] + b4[i]);
                else
                    ap[j] += om * xv;
            }
        }
    }
    // g = LN(gap / hw); SRA: s = LN(pool)
    const float rhw = 1.f / (float)hw;
    float sg = 0.f, sa = 0.f;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        if (tid + AP_THREADS * j < nv) {
            gp[j] = gp[j] * rhw;
            sg += (gp[j][0] + gp[j][1]) + (gp[j][2] + gp[j][3]);
            sa += (ap[j][0] + ap[j][1]) + (ap[j][2] + ap[j][3]);
        }
    }
    const float mg = block_sum(sg, s_red) * rc;
    const float ma = PCAM ? 0.f : block_sum(sa, s_red) * rc;
    float qg = 0.f, qa = 0.f;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        if (tid + AP_THREADS * j < nv) {
            const f32x4 dg = gp[j] - mg, da = ap[j] - ma;
            qg += dot4(dg, dg);
            qa += dot4(da, da);
        }
    }
    const float rg = 1.0f / sqrtf(block_sum(qg, s_red) * rc + eps);
    const float ra = PCAM ? 0.f : 1.0f / sqrtf(block_sum(qa, s_red) * rc + eps);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int i = tid + AP_THREADS * j;
        if (i < nv) {
            const f32x4 g = (gp[j] - mg) * rg * g4[i] + b4[i];
            const f32x4 a = PCAM ? ap[j] : (ap[j] - ma) * ra * g4[i] + b4[i];
            gp[j] = g + lam * a;
            ss += dot4(gp[j], gp[j]);
        }
    }
    float sc = 1.f;
    if (normalize) {
        const float nrm = sqrtf(block_sum(ss, s_red));
        sc = 1.f / (nrm > 1e-12f ? nrm : 1e-12f);
    }
    f32x4 *yr = reinterpret_cast<f32x4 *>(y + (int64_t)blockIdx.x * c);
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int i = tid + AP_THREADS * j;
        if (i < nv) yr[i] = normalize ? gp[j] * sc : gp[j];
    }
}

// the documented limits of include/mirx.h; the entry points check them before anything reaches the device
const char *attnpool_args_error(const float *x, int64_t n, int hw, int c, const float *w, int K, const float *gamma,
                                const float *beta, float eps, const float *y) {
    if (n < 0 || n > 0x7fffffff) return "batch must be in [0, 2^31 - 1]";
    if (c < 4 || c % 4 || c > MIRX_ATTNPOOL_MAX_C) return "c must be a multiple of 4 in [4, 8192]";
    if (K < 1 || K > MIRX_ATTNPOOL_MAX_K) return "K must be in [1, 64]";
    if (hw < 1 || (int64_t)(K + 3) * hw > MIRX_ATTNPOOL_LDS_FLOATS) return "(K + 3) * hw must be in [K + 3, 16384] (LDS budget)";
    if (!(eps >= 0.f)) return "eps must be >= 0";
    if (n > 0 && !(x && w && gamma && beta && y)) return "null buffer";
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) % 16)
        return "x, w, gamma, beta and y must be 16-byte aligned";
    return nullptr;
}

}  // namespace

template <bool PCAM>
static hipError_t launch_attnpool(const float *x, int64_t n, int hw, int c, const float *w, const float *b, int K,
                                  const float *gamma, const float *beta, float eps, float lam, int normalize, float *y, float *logits,
                                  hipStream_t st) {
    if (n == 0) return hipSuccess;
    const size_t lds = ((size_t)(K + 3) * hw + 4 + 64) * sizeof(float);
    const dim3 grid((unsigned)n), block(AP_THREADS);
#define MIRX_AP(RV)                                                                                                          \
    hipLaunchKernelGGL((k_attnpool<PCAM, RV>), grid, block, lds, st, x, hw, c, w, b, K, gamma, beta, eps, lam, normalize, y, \
                       logits)
    if (c <= 256) MIRX_AP(1);
    else if (c <= 512) MIRX_AP(2);
    else if (c <= 1024) MIRX_AP(4);
    else if (c <= 2048) MIRX_AP(8);
    else if (c <= 4096) MIRX_AP(16);
    else MIRX_AP(32);
#undef MIRX_AP
    return hipGetLastError();
}

hipError_t launch_sra_head(const float *x, int64_t n, int hw, int c, const float *w, int K, const float *gamma, const float *beta,
                           float eps, float lam, int normalize, float *y, hipStream_t st) {
    return launch_attnpool<false>(x, n, hw, c, w, nullptr, K, gamma, beta, eps, lam, normalize, y, nullptr, st);
}

hipError_t launch_pcam_head(const float *x, int64_t n, int hw, int c, const float *w, const float *b, int K, const float *gamma,
                            const float *beta, float eps, float lam, int normalize, float *feat, float *logits, hipStream_t st) {
    return launch_attnpool<true>(x, n, hw, c, w, b, K, gamma, beta, eps, lam, normalize, feat, logits, st);
}

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

extern "C" int mirx_sra_head_nhwc(const float *x, int64_t n, int hw, int c, const float *w_att, int K, const float *gamma,
                                  const float *beta, float eps, float lam, int normalize, float *y, void *stream) {
    const char *why = attnpool_args_error(x, n, hw, c, w_att, K, gamma, beta, eps, y);
    if (why) return fail(MIRX_EINVAL, std::string("sra_head: ") + why);
    MIRX_HIP(launch_sra_head(x, n, hw, c, w_att, K, gamma, beta, eps, lam, normalize, y, reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}

extern "C" int mirx_pcam_head_nhwc(const float *x, int64_t n, int hw, int c, const float *w_cls, const float *b_cls, int K,
                                   const float *gamma, const float *beta, float eps, float lam, int normalize, float *feat,
                                   float *class_logits_or_null, void *stream) {
    const char *why = attnpool_args_error(x, n, hw, c, w_cls, K, gamma, beta, eps, feat);
    if (why) return fail(MIRX_EINVAL, std::string("pcam_head: ") + why);
    if (n > 0 && !b_cls) return fail(MIRX_EINVAL, "pcam_head: null buffer (b_cls)");
    MIRX_HIP(launch_pcam_head(x, n, hw, c, w_cls, b_cls, K, gamma, beta, eps, lam, normalize, feat, class_logits_or_null,
                              reinterpret_cast<hipStream_t>(stream)));
    return MIRX_OK;
}
