// k_resample.hip -- batched Resize(shorter side) + CenterCrop, or Resize((S, S)), of 8-bit images, bit-equal to Pillow's BILINEAR
// and BICUBIC (gfx950, wave64; include/mirx.h).
//
// Pillow resizes an 8-bit image in two separable passes, horizontal first into an 8-bit intermediate, then vertical: per output
// index a run of source taps [first, first + count) with double-precision filter weights (triangle, or the a = -0.5 cubic, whose
// outer lobes are negative), normalised by their sum, quantised to 22 fractional bits, and out = clip((2^21 + sum pixel * coeff) >> 22, 0, 255) in 32-bit integers.  The weights depend on the
// sizes alone, so the HOST plans them (resample_plan, below: plain double arithmetic in Pillow's order, no device) and the kernel
// does integer multiply-adds only.  Only the S outputs inside the crop window are planned: the resized image outside the crop
// never exists.
//
// One launch resamples B images of different sizes.  Everything the kernel reads is one device byte buffer (the "blob", one
// host-to-device copy): B descriptors of 8 int64, the axis tables, the interleaved 8-bit sources.  A workgroup of 256 threads
// owns one image and one tile of 16 output rows x 32 output columns:
//   stage     the tile's x coefficients into LDS, transposed to [tap][column] (a wave then reads one tap of 32 columns from 32
//             consecutive banks; in global memory a column's taps are contiguous, so the stride sits on this one-off read)
//   pass 1    for the source rows [r0, r1) the tile's 16 output rows tap: lane = output column, 8 source rows in flight per
//             workgroup.  Neighbouring lanes read neighbouring source pixels (scale * channels bytes apart, the runs overlap), so a
//             wave's byte loads fall in a few consecutive cache lines.  8-bit results go to LDS as [row][channel][32 columns]
//   barrier
//   pass 2    a thread owns 4 adjacent columns of one output row and channel: one ds_read_b32 per tap (8 lanes cover a row-channel's
//             32 bytes, consecutive lanes consecutive banks), 4 multiply-adds, then one 4-byte (8-bit form) or 16-byte (fp32 form)
//             store when S % 4 == 0, single stores otherwise.  A one-channel source is resampled once and written to the three
//             planes (convert("RGB") of an "L" image replicates the channel).
// The fp32 form applies x = u / 255, (x - mean[c]) / std[c] in IEEE fp32 with correctly rounded division and no contraction: the
// operations of ToTensor + Normalize.  No atomic, no inline assembly, nothing data-dependent in any address: the tap ranges are
// checked on the host against the image before the launch (resample_check), so every load stays inside its image.
//
// Reference behaviour replaced: transforms.Resize + CenterCrop (+ ToTensor + Normalize) of milvus_retrieval.py:176-198,
// test.py:1286-1332, ingest_embeddings.py:112-122, nih_multilabel_retrieval.py:64-66.
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace mirx {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TW = MIRX_RESAMPLE_TILE_W;      // 32 output columns: a row-channel of the intermediate is 32 bytes
constexpr int RS_TH = MIRX_RESAMPLE_TILE_H;      // 16 output rows
constexpr int RS_BITS = 22;                      // fractional bits of a coefficient
constexpr int RS_HALF = 1 << (RS_BITS - 1);
constexpr int RS_DESC = MIRX_RESAMPLE_DESC_WORDS;
constexpr int RS_HDR = 4;                        // int32 words in front of a table's bounds
static_assert(RS_TW == 32 && RS_THREADS % RS_TW == 0, "pass 1 maps a lane to a column of a 32-column tile");

struct RsNorm {
    float mean[3], stdv[3];
};

// v is a signed sum (the cubic's outer coefficients are negative): an arithmetic shift, as in Pillow's clip8
__device__ inline int rs_clip8(int v) {
    v >>= RS_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <int CH>
__device__ inline void rs_rows(const unsigned char *__restrict__ src, int64_t pitch, int r0, int span, int xmin, int cnt,
                               const int32_t *lk, unsigned char *inter, int xx, int rsub) {
    for (int r = rsub; r < span; r += RS_THREADS / RS_TW) {
        const unsigned char *p = src + (int64_t)(r0 + r) * pitch + xmin * CH;
        int acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = RS_HALF;
        for (int t = 0; t < cnt; ++t) {
            const int k = lk[t * RS_TW + xx];
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] += (int)p[t * CH + c] * k;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) inter[(r * CH + c) * RS_TW + xx] = (unsigned char)rs_clip8(acc[c]);
    }
}

template <int OUT_F32>
__device__ inline void rs_store4(void *out, int64_t idx, const int (&v)[4], int nvalid, bool vec, float mean, float stdv) {
    if (OUT_F32) {
        float *o = reinterpret_cast<float *>(out) + idx;
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = ((float)v[e] / 255.0f - mean) / stdv;
        if (vec) {
            const f32x4 q = {f[0], f[1], f[2], f[3]};
            *reinterpret_cast<f32x4 *>(o) = q;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nvalid) o[e] = f[e];
        }
    } else {
        unsigned char *o = reinterpret_cast<unsigned char *>(out) + idx;
        if (vec) {
            *reinterpret_cast<unsigned *>(o) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nvalid) o[e] = (unsigned char)v[e];
        }
    }
}

template <int OUT_F32>
__global__ __launch_bounds__(RS_THREADS) void k_resample(const unsigned char *__restrict__ blob, int s, int tiles_x, int tiles_per_img,
                                                         RsNorm nm, void *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
    const int img = blockIdx.x / tiles_per_img, tile = blockIdx.x - img * tiles_per_img;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int64_t *d = reinterpret_cast<const int64_t *>(blob) + (int64_t)img * RS_DESC;
    const unsigned char *src = blob + d[0];
    const int64_t pitch = d[3];
    const int ch = (int)d[4];
    const int32_t *xt = reinterpret_cast<const int32_t *>(blob + d[5]), *yt = reinterpret_cast<const int32_t *>(blob + d[6]);
    const int kx = xt[0], ky = yt[0];
    const int32_t *xb = xt + RS_HDR, *xk = xb + 2 * s, *yb = yt + RS_HDR, *yk = yb + 2 * s;
    const int x0 = tx * RS_TW, y0 = ty * RS_TH;
    const int ncol = min(RS_TW, s - x0), nrow = min(RS_TH, s - y0);

    // the source rows this tile's output rows tap (the host sized the LDS with the same loop: resample_check)
    int r0 = INT32_MAX, r1 = 0;
    for (int j = 0; j < nrow; ++j) {
        const int f = yb[2 * (y0 + j)], c = yb[2 * (y0 + j) + 1];
        r0 = min(r0, f);
        r1 = max(r1, f + c);
    }
    const int span = r1 - r0;

    int32_t *lk = reinterpret_cast<int32_t *>(rs_smem);                  // [kx][32] x coefficients
    unsigned char *inter = rs_smem + (size_t)kx * RS_TW * 4;            // [span][ch][32] horizontal-pass results
    for (int i = threadIdx.x; i < kx * RS_TW; i += RS_THREADS) {
        const int t = i / RS_TW, xx = i - t * RS_TW;
        lk[i] = xx < ncol ? xk[(int64_t)(x0 + xx) * kx + t] : 0;
    }
    __syncthreads();

    {
        const int xx = threadIdx.x & (RS_TW - 1), rsub = threadIdx.x / RS_TW;
        if (xx < ncol) {
            const int xmin = xb[2 * (x0 + xx)], cnt = xb[2 * (x0 + xx) + 1];
            if (ch == 3)
                rs_rows<3>(src, pitch, r0, span, xmin, cnt, lk, inter, xx, rsub);
            else
                rs_rows<1>(src, pitch, r0, span, xmin, cnt, lk, inter, xx, rsub);
        }
    }
    __syncthreads();

    const bool vec = (s & 3) == 0;
    const int items = nrow * ch * (RS_TW / 4);
    for (int i = threadIdx.x; i < items; i += RS_THREADS) {
        const int col4 = i & (RS_TW / 4 - 1), jc = i / (RS_TW / 4);
        const int j = jc / ch, c = jc - j * ch;
        const int nvalid = ncol - col4 * 4;
        if (nvalid <= 0) continue;
        const int y = y0 + j;
        const int f = yb[2 * y] - r0, cnt = yb[2 * y + 1];
        const int32_t *k = yk + (int64_t)y * ky;
        int acc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF};
        for (int t = 0; t < cnt; ++t) {
            const unsigned v = *reinterpret_cast<const unsigned *>(inter + ((f + t) * ch + c) * RS_TW + col4 * 4);
            const int kk = k[t];
            acc[0] += (int)(v & 255u) * kk;
            acc[1] += (int)(v >> 8 & 255u) * kk;
            acc[2] += (int)(v >> 16 & 255u) * kk;
            acc[3] += (int)(v >> 24) * kk;
        }
        int res[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) res[e] = rs_clip8(acc[e]);
        const int64_t at = ((int64_t)img * 3 * s + y) * s + x0 + col4 * 4;          // plane 0
        const int64_t plane = (int64_t)s * s;
        if (ch == 3) {
            rs_store4<OUT_F32>(out, at + c * plane, res, nvalid, vec, nm.mean[c], nm.stdv[c]);
        } else {
#pragma unroll
            for (int p = 0; p < 3; ++p) rs_store4<OUT_F32>(out, at + p * plane, res, nvalid, vec, nm.mean[p], nm.stdv[p]);
        }
    }
}

}  // namespace

// ---- host: the plan -----------------------------------------------------------------------------------------------------------
namespace {

// Pillow's filters (Resample.c): the triangle of support 1 and the a = -0.5 cubic of support 2.  One operation per statement,
// in Pillow's association (this file is compiled with -ffp-contract=off).
inline double rs_triangle(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

inline double rs_bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) {
        double t = (a + 2.0) * x;
        t = t - (a + 3.0);
        t = t * x;
        t = t * x;
        return t + 1.0;
    }
    if (x < 2.0) {
        double t = x - 5.0;
        t = t * x;
        t = t + 8.0;
        t = t * x;
        t = t - 4.0;
        return t * a;
    }
    return 0.0;
}

inline double rs_support(int filter) { return filter == MIRX_RESAMPLE_BICUBIC ? 2.0 : 1.0; }

}  // namespace

// Pillow's coefficient count for an axis resized from in_size to out_size with a filter of support 1 (triangle) or 2 (cubic).
int resample_taps(int in_size, int out_size, int filter) {
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    const double support = rs_support(filter) * fs;
    return (int)ceil(support) * 2 + 1;
}

// table = int32 [4 + 2 n + n ksize]: {ksize, n, in_size, filter}, bounds [n][2] = (first tap, tap count), coefficients [n][ksize]
// (zero past the count), for the outputs [first, first + n) of the axis.  Double arithmetic in Pillow's order, one operation per
// statement (this file is compiled with -ffp-contract=off).
void resample_plan(int in_size, int out_size, int first, int n, int filter, int32_t *table) {
    const int ksize = resample_taps(in_size, out_size, filter);
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = rs_support(filter) * fs;
    const double ss = 1.0 / fs;
    table[0] = ksize, table[1] = n, table[2] = in_size, table[3] = filter;
    int32_t *bounds = table + RS_HDR, *coef = bounds + 2 * n;
    double w[MIRX_RESAMPLE_MAX_TAPS];
    for (int i = 0; i < n; ++i) {
        const double center = (first + i + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int cnt = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            const double a = (x + xmin - center + 0.5) * ss;
            w[x] = filter == MIRX_RESAMPLE_BICUBIC ? rs_bicubic(a) : rs_triangle(a);
            ww += w[x];
        }
        int32_t *k = coef + (int64_t)i * ksize;
        for (int x = 0; x < ksize; ++x) {
            if (x >= cnt) {
                k[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            // a triangle weight is never negative; the cubic is negative for 1 < |x| < 2, and Pillow rounds away from zero
            k[x] = v < 0.0 ? (int32_t)(-0.5 + v * (double)(1 << RS_BITS)) : (int32_t)(0.5 + v * (double)(1 << RS_BITS));
        }
        bounds[2 * i] = xmin, bounds[2 * i + 1] = cnt;
    }
}

// ---- host: what a launch may touch --------------------------------------------------------------------------------------------
namespace {

struct RsTable {
    int64_t off;
    int in_size, ksize, filter;
    int64_t max_span;      // y use only: the largest source-row span of a tile row
};

// One axis table at blob + off, for an axis of in_size source pixels and s outputs: inside the blob, every tap run inside
// [0, in_size), and by the filter in header word 3: triangle, every coefficient >= 0 and every run's sum <= 2^23; cubic, signed
// coefficients and every run's sum of magnitudes <= 2^23 (255 * 2^23 + 2^21 < 2^31: the 32-bit sums cannot overflow, in
// either direction and at any prefix of a run).
const char *rs_check_table(const unsigned char *blob, int64_t blob_bytes, int64_t head_bytes, int64_t off, int in_size, int s,
                           RsTable &tb) {
    if (off < head_bytes || (off & 15) || off > blob_bytes - RS_HDR * 4) return "resample: a table offset is misaligned or outside the buffer";
    const int32_t *t = reinterpret_cast<const int32_t *>(blob + off);
    const int ksize = t[0];
    if (ksize < 1 || ksize > MIRX_RESAMPLE_MAX_TAPS) return "resample: tap count over the cap (MIRX_RESAMPLE_MAX_TAPS = 65: scale > 32)";
    if (t[1] != s || t[2] != in_size) return "resample: a table was planned for another output or source size";
    const int filter = t[3];
    if (filter != MIRX_RESAMPLE_BILINEAR && filter != MIRX_RESAMPLE_BICUBIC)
        return "resample: unknown filter in a table's header (word 3: 0 = bilinear, 1 = bicubic)";
    const int64_t words = RS_HDR + 2 * (int64_t)s + (int64_t)s * ksize;
    if (off + words * 4 > blob_bytes) return "resample: a table runs past the buffer";
    const int32_t *bounds = t + RS_HDR, *coef = bounds + 2 * s;
    for (int i = 0; i < s; ++i) {
        const int f = bounds[2 * i], c = bounds[2 * i + 1];
        if (f < 0 || c < 1 || c > ksize || f > in_size - c) return "resample: a tap range lies outside the image";
        int64_t sum = 0;
        for (int x = 0; x < c; ++x) {
            const int32_t k = coef[(int64_t)i * ksize + x];
            if (k < 0 && filter == MIRX_RESAMPLE_BILINEAR) return "resample: negative coefficient";
            sum += k < 0 ? -(int64_t)k : k;
        }
        if (sum > (1 << (RS_BITS + 1)))
            return filter == MIRX_RESAMPLE_BILINEAR ? "resample: a coefficient run sums to more than 2^23"
                                                    : "resample: a bicubic coefficient run's magnitudes sum to more than 2^23";
    }
    tb.off = off, tb.in_size = in_size, tb.ksize = ksize, tb.filter = filter, tb.max_span = 0;
    for (int y0 = 0; y0 < s; y0 += RS_TH) {
        int r0 = INT32_MAX, r1 = 0;
        for (int j = y0; j < std::min(s, y0 + RS_TH); ++j) {
            r0 = std::min(r0, bounds[2 * j]);
            r1 = std::max(r1, bounds[2 * j] + bounds[2 * j + 1]);
        }
        tb.max_span = std::max<int64_t>(tb.max_span, r1 - r0);
    }
    return nullptr;
}

const RsTable *rs_find(const std::vector<RsTable> &seen, int64_t off, int in_size) {
    for (const RsTable &t : seen)
        if (t.off == off && t.in_size == in_size) return &t;
    return nullptr;
}

}  // namespace

// Checks the descriptors and tables of a blob (HOST memory) and returns the dynamic LDS bytes the launch needs through *lds.
// nullptr = everything a launch on a device copy of this blob reads lies inside it.  Images that share a table (same offset)
// have it checked once.
const char *resample_check(const void *blob_host, int64_t blob_bytes, int64_t b, int s, int64_t *lds) {
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(blob_host);
    const int64_t head = b * RS_DESC * 8;
    if (blob_bytes < head) return "resample: the buffer is smaller than its descriptors";
    const int64_t *d = reinterpret_cast<const int64_t *>(blob);
    std::vector<RsTable> xs, ys;
    int64_t need = 0;
    for (int64_t i = 0; i < b; ++i, d += RS_DESC) {
        const int64_t off = d[0], w = d[1], h = d[2], pitch = d[3], ch = d[4];
        if (w < 1 || h < 1 || w > MIRX_RESAMPLE_MAX_SIDE || h > MIRX_RESAMPLE_MAX_SIDE)
            return "resample: source side outside [1, MIRX_RESAMPLE_MAX_SIDE = 8192]";
        if (ch != 1 && ch != 3) return "resample: channels must be 1 or 3";
        if (pitch < w * ch || pitch > (int64_t)MIRX_RESAMPLE_MAX_SIDE * 4) return "resample: row pitch smaller than a row (or over 32768)";
        if (off < head || (off & 15)) return "resample: an image offset is misaligned or inside the descriptors";
        if (off > blob_bytes || (h - 1) * pitch + w * ch > blob_bytes - off) return "resample: an image runs past the buffer";
        const RsTable *tx = rs_find(xs, d[5], (int)w), *ty = rs_find(ys, d[6], (int)h);
        RsTable t;
        if (!tx) {
            if (const char *msg = rs_check_table(blob, blob_bytes, head, d[5], (int)w, s, t)) return msg;
            xs.push_back(t);
            tx = &xs.back();
        }
        if (!ty) {
            if (const char *msg = rs_check_table(blob, blob_bytes, head, d[6], (int)h, s, t)) return msg;
            ys.push_back(t);
            ty = &ys.back();
        }
        if (tx->filter != ty->filter) return "resample: the x and y tables of an image name different filters";
        need = std::max<int64_t>(need, (int64_t)tx->ksize * RS_TW * 4 + ty->max_span * ch * RS_TW);
    }
    if (need > MIRX_RESAMPLE_MAX_LDS) return "resample: a tile's source rows need more LDS than the cap (MIRX_RESAMPLE_MAX_LDS = 65536)";
    *lds = (need + 15) / 16 * 16;
    return nullptr;
}

hipError_t launch_resample(const void *blob_dev, int64_t b, int s, int out_f32, const float *mean3, const float *std3, void *out,
                           int64_t lds, hipStream_t st) {
    const int tiles_x = (s + RS_TW - 1) / RS_TW, tiles = tiles_x * ((s + RS_TH - 1) / RS_TH);
    RsNorm nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    if (out_f32)
        for (int c = 0; c < 3; ++c) nm.mean[c] = mean3[c], nm.stdv[c] = std3[c];
    const dim3 grid((unsigned)(b * tiles));
    const unsigned char *blob = reinterpret_cast<const unsigned char *>(blob_dev);
    // the attribute is raised once per device to the cap; a launch then asks for what its batch needs
    if (out_f32) {
        static std::atomic<unsigned long long> attr_devs{0};
        const hipError_t e = set_dynamic_lds(k_resample<1>, MIRX_RESAMPLE_MAX_LDS, &attr_devs);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_resample<1>, grid, dim3(RS_THREADS), (size_t)lds, st, blob, s, tiles_x, tiles, nm, out);
    } else {
        static std::atomic<unsigned long long> attr_devs{0};
        const hipError_t e = set_dynamic_lds(k_resample<0>, MIRX_RESAMPLE_MAX_LDS, &attr_devs);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_resample<0>, grid, dim3(RS_THREADS), (size_t)lds, st, blob, s, tiles_x, tiles, nm, out);
    }
    return hipGetLastError();
}

}  // namespace mirx
