// k_simcam.hip -- SimCAM similarity saliency (the reference's explanations.py SimCAM / SimCAM_MedSigLIP / SimCAM_Densenet121)
// on channels-last fp32 token rows.  One query row block Q [hw, C] against P retrieved row blocks R [P, hw, C]; per pair p
// D_p = Q R_p^T [hw, hw], s_p = max(D_p) + eps and the two maps
//     decom_1[i] = sum_j relu(D_p[i, j] / s_p)   (query map)      decom_2[j] = sum_i relu(D_p[i, j] / s_p)   (retrieved map)
// or, with a point, the retrieved map as the bilinear blend of up to four rows relu(D_p[i*, :] / s_p), clamped at 0; every
// map upsampled to H x W with F.interpolate(mode="bilinear", align_corners=False)'s source-index rule.
//
//   k_simcam_pairs   a 64 x 64 tile of D_p per workgroup on v_mfma_f32_16x16x4_f32 (f32 operands and accumulator: every D
//                    element is a fixed-order MFMA reduction over its two rows, whatever the tile or P).  Epilogue through LDS: the tile's max (NaN
//                    kept), per row and per column of the tile the sums of max(D, 0) and of min(D, 0) in column / row order,
//                    and the tile's part of the point rows, each to its own workspace slot (no atomics).
//   k_simcam_maps    per (pair, map, band of output rows): the pair's tile maxima in tile order -> s; partial sums in tile order
//                    -> relu(D) / s when s > 0 (sum max(D, 0) / s), min(D, 0) / s when s < 0, NaN when s is 0 or NaN (the
//                    reference's 0 / 0 and NaN propagation); the h x w map in LDS; the bilinear upsample; the stores.
//   k_bn_relu_rows   relu(x * scale + shift) of an NCHW map written as channels-last rows [B, hw, C] (DenseNet's norm5 + ReLU).
//
// Every output of pair p is a fixed-order function of Q and R_p alone: bit-identical whatever P is and wherever p sits.
#include <algorithm>
#include <cmath>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int SC_TILE = 64;              // D tile edge
constexpr int SC_KT = 16;                // K chunk staged through LDS
constexpr int SC_THREADS = 256;          // 4 waves, a 32 x 32 quarter of the tile each
constexpr int SC_LDS_STRIDE = SC_KT + 1; // operand rows in LDS, padded
constexpr int SC_D_STRIDE = SC_TILE + 1; // the D tile in LDS, padded
constexpr int SC_MAP_ROWS = 16;          // output rows per maps workgroup

struct PairsArgs {
    const float *q;          // [hw, c]
    const float *r;          // [P, hw, c]
    int64_t hw, c, pair_stride;
    int nt;                  // tiles per edge
    int sel[4];              // query positions whose D rows are kept (point mode), -1 = none
    float *ws;               // workspace, simcam_ws_pair_floats(hw) per pair
};

// per-pair workspace layout (floats); hp = nt * 64
__host__ __device__ inline int64_t ws_pair_floats(int nt) { return (int64_t)nt * nt + 4LL * nt * nt * SC_TILE + 4LL * nt * SC_TILE; }
__host__ __device__ inline int64_t ws_rowpos(int nt) { return (int64_t)nt * nt; }                          // [nt (tj)][hp]
__host__ __device__ inline int64_t ws_rowneg(int nt) { return ws_rowpos(nt) + (int64_t)nt * nt * SC_TILE; }
__host__ __device__ inline int64_t ws_colpos(int nt) { return ws_rowneg(nt) + (int64_t)nt * nt * SC_TILE; } // [nt (ti)][hp]
__host__ __device__ inline int64_t ws_colneg(int nt) { return ws_colpos(nt) + (int64_t)nt * nt * SC_TILE; }
__host__ __device__ inline int64_t ws_sel(int nt) { return ws_colneg(nt) + (int64_t)nt * nt * SC_TILE; }    // [4][hp]

__global__ __launch_bounds__(SC_THREADS) void k_simcam_pairs(PairsArgs a) {
    __shared__ float As[SC_TILE * SC_LDS_STRIDE];
    __shared__ float Bs[SC_TILE * SC_LDS_STRIDE];
    __shared__ float Dt[SC_TILE * SC_D_STRIDE];
    __shared__ float rmax[SC_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = blockIdx.x / a.nt, tj = blockIdx.x % a.nt;
    const int64_t p = blockIdx.y;
    const int64_t i0 = (int64_t)ti * SC_TILE, j0 = (int64_t)tj * SC_TILE;
    const float *qb = a.q, *rb = a.r + p * a.pair_stride;
    f32x4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lr = tid >> 4, lk = tid & 15;          // staging: 16 rows x 16 k per pass, 4 passes
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    for (int64_t k0 = 0; k0 < a.c; k0 += SC_KT) {
        const int64_t k = k0 + lk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = lr + 16 * u;
            const int64_t gi = i0 + row, gj = j0 + row;
            As[row * SC_LDS_STRIDE + lk] = (gi < a.hw && k < a.c) ? qb[gi * a.c + k] : 0.f;
            Bs[row * SC_LDS_STRIDE + lk] = (gj < a.hw && k < a.c) ? rb[gj * a.c + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < SC_KT / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            float af[2], bf[2];
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                af[b2] = As[(wr + b2 * 16 + (lane & 15)) * SC_LDS_STRIDE + kk];
                bf[b2] = Bs[(wc + b2 * 16 + (lane & 15)) * SC_LDS_STRIDE + kk];
            }
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[bi], bf[bj], acc[bi][bj], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the 16x16 block: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                Dt[(wr + bi * 16 + (lane >> 4) * 4 + e) * SC_D_STRIDE + wc + bj * 16 + (lane & 15)] = acc[bi][bj][e];
    __syncthreads();
    const int vi = a.hw - i0 < SC_TILE ? (int)(a.hw - i0) : SC_TILE;   // valid rows / cols of the tile
    const int vj = a.hw - j0 < SC_TILE ? (int)(a.hw - j0) : SC_TILE;
    float *ws = a.ws + p * ws_pair_floats(a.nt);
    const int64_t hp = (int64_t)a.nt * SC_TILE;
    if (tid < SC_TILE) {                                        // row sums (column order) and row maxima
        const int i = tid;
        float sp = 0.f, sn = 0.f, m = -INFINITY;
        if (i < vi) {
            for (int j = 0; j < vj; ++j) {
                const float d = Dt[i * SC_D_STRIDE + j];
                sp += fmaxf(d, 0.f);
                sn += fminf(d, 0.f);
                m = nanmax(m, d);
                if (d != d) { sp = d; sn = d; }                 // fmaxf / fminf drop NaN: carry it into both sums
            }
            ws[ws_rowpos(a.nt) + tj * hp + i0 + i] = sp;
            ws[ws_rowneg(a.nt) + tj * hp + i0 + i] = sn;
        }
        rmax[i] = m;
    } else if (tid < 2 * SC_TILE) {                            // column sums (row order)
        const int j = tid - SC_TILE;
        if (j < vj) {
            float sp = 0.f, sn = 0.f;
            for (int i = 0; i < vi; ++i) {
                const float d = Dt[i * SC_D_STRIDE + j];
                sp += fmaxf(d, 0.f);
                sn += fminf(d, 0.f);
                if (d != d) { sp = d; sn = d; }
            }
            ws[ws_colpos(a.nt) + ti * hp + j0 + j] = sp;
            ws[ws_colneg(a.nt) + ti * hp + j0 + j] = sn;
        }
    } else if (tid < 3 * SC_TILE) {                            // the point rows that fall in this tile
        const int j = tid - 2 * SC_TILE;
        if (j < vj) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int64_t li = (int64_t)a.sel[s] - i0;
                if (a.sel[s] >= 0 && li >= 0 && li < vi) ws[ws_sel(a.nt) + s * hp + j0 + j] = Dt[li * SC_D_STRIDE + j];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float m = -INFINITY;
        for (int i = 0; i < vi; ++i) m = nanmax(m, rmax[i]);
        ws[ti * a.nt + tj] = m;
    }
}

struct MapsArgs {
    const float *ws;
    int64_t hw;
    int h, w, nt, H, W;
    float eps;
    int first_map, nmaps;    // maps first_map .. first_map + nmaps - 1 of {0: query, 1: retrieved}
    int point;               // 1: map 1 is the point blend of the sel rows
    float wt[4][2];          // point weights per corner: the reference multiplies by (1 - dx) or dx, then (1 - dy) or dy
    float *out;              // [P, nmaps, H, W]
};

__global__ __launch_bounds__(SC_THREADS) void k_simcam_maps(MapsArgs a) {
    extern __shared__ float smap[];                           // [hw]
    __shared__ float s_sh;
    const int tid = threadIdx.x;
    const int mi = blockIdx.y, map = a.first_map + mi;
    const int64_t p = blockIdx.z;
    const int nt = a.nt;
    const float *ws = a.ws + p * ws_pair_floats(nt);
    const int64_t hp = (int64_t)nt * SC_TILE;
    if (tid == 0) {
        float m = -INFINITY;
        for (int t = 0; t < nt * nt; ++t) m = nanmax(m, ws[t]);
        s_sh = m + a.eps;
    }
    __syncthreads();
    const float s = s_sh;
    for (int64_t i = tid; i < a.hw; i += SC_THREADS) {
        float v;
        if (map == 1 && a.point) {
            v = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = relu_nan(ws[ws_sel(nt) + c * hp + i] / s);
                v = v + (d * a.wt[c][0]) * a.wt[c][1];
            }
            v = relu_nan(v);
        } else {
            const float *pos = ws + (map == 0 ? ws_rowpos(nt) : ws_colpos(nt));
            const float *neg = ws + (map == 0 ? ws_rowneg(nt) : ws_colneg(nt));
            float sp = 0.f, sn = 0.f;
            for (int t = 0; t < nt; ++t) {
                sp += pos[t * hp + i];
                sn += neg[t * hp + i];
            }
            v = (s < 0.f) ? sn / s : sp / s;                  // s == 0 or NaN: NaN (0 / 0, x / NaN), as the reference
        }
        smap[i] = v;
    }
    __syncthreads();
    // bilinear, align_corners=False (ATen's upsample_bilinear2d source index: max(scale * (dst + 0.5) - 0.5, 0))
    const float sh = (float)a.h / (float)a.H, sw = (float)a.w / (float)a.W;
    const int y_lo = blockIdx.x * SC_MAP_ROWS, y_hi = min(a.H, y_lo + SC_MAP_ROWS);
    float *out = a.out + (p * a.nmaps + mi) * (int64_t)a.H * a.W;
    const int64_t n = (int64_t)(y_hi - y_lo) * a.W;
    for (int64_t e = tid; e < n; e += SC_THREADS) {
        const int y = y_lo + (int)(e / a.W), x = (int)(e % a.W);
        out[(int64_t)y * a.W + x] = bilinear_half_pixel(smap, a.h, a.w, sh, sw, y, x);
    }
}

// relu(x * scale + shift), NCHW [b, c, hw] -> rows [b, hw, c]; a 32 x 32 (channel, position) tile through LDS
__global__ __launch_bounds__(256) void k_bn_relu_rows(const float *__restrict__ x, int64_t c, int64_t hw, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, float *__restrict__ out) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t b = blockIdx.z, c0 = (int64_t)blockIdx.y * 32, p0 = (int64_t)blockIdx.x * 32;
    const float *xb = x + b * c * hw;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t ch = c0 + ty + 8 * u, pos = p0 + tx;
        float v = 0.f;
        if (ch < c && pos < hw) v = relu_nan(fmaf(xb[ch * hw + pos], scale[ch], shift[ch]));
        t[ty + 8 * u][tx] = v;
    }
    __syncthreads();
    float *ob = out + b * hw * c;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t pos = p0 + ty + 8 * u, ch = c0 + tx;
        if (ch < c && pos < hw) ob[pos * c + ch] = t[tx][ty + 8 * u];
    }
}

}  // namespace

}  // namespace mirx

// ---- C ABI (include/mirx.h) -------------------------------------------------------------------------------------------
using namespace mirx;

static int simcam_tiles(int64_t hw) { return (int)((hw + SC_TILE - 1) / SC_TILE); }

extern "C" int64_t mirx_simcam_workspace_floats(int64_t pairs, int64_t hw) {
    if (pairs < 0 || pairs > MIRX_SIMCAM_MAX_PAIRS || hw < 1 || hw > MIRX_SIMCAM_MAX_HW)
        return fail(MIRX_EINVAL, "simcam_workspace_floats: pairs must be in [0, 65535] and hw in [1, 1024]");
    return pairs * ws_pair_floats(simcam_tiles(hw));
}

extern "C" int mirx_simcam(const float *q, const float *r, int64_t pairs, int64_t pair_stride, int h, int w, int64_t c, float eps,
                           int maps, const double *point, int H, int W, float *workspace, int64_t workspace_floats, float *out,
                           void *stream) {
    const int64_t hw = (int64_t)h * w;
    if (h < 1 || w < 1 || hw > MIRX_SIMCAM_MAX_HW) return fail(MIRX_EINVAL, "simcam: h, w >= 1 and h * w <= 1024");
    if (c < 1 || c > MIRX_SIMCAM_MAX_C) return fail(MIRX_EINVAL, "simcam: c must be in [1, 16384]");
    if (pairs < 0 || pairs > MIRX_SIMCAM_MAX_PAIRS) return fail(MIRX_EINVAL, "simcam: pairs must be in [0, 65535]");
    if (pair_stride < hw * c) return fail(MIRX_EINVAL, "simcam: pair_stride < hw * c");
    if (H < 1 || W < 1 || H > MIRX_SIMCAM_MAX_SIZE || W > MIRX_SIMCAM_MAX_SIZE) return fail(MIRX_EINVAL, "simcam: H, W must be in [1, 8192]");
    if (maps != MIRX_SIMCAM_MAPS_BOTH && maps != MIRX_SIMCAM_MAPS_RETRIEVED) return fail(MIRX_EINVAL, "simcam: maps must be 0 (both) or 1 (retrieved)");
    if (!(eps >= 0.f) || !(eps < INFINITY)) return fail(MIRX_EINVAL, "simcam: eps must be finite and >= 0");
    MapsArgs ma{};
    PairsArgs pa{};
    pa.sel[0] = pa.sel[1] = pa.sel[2] = pa.sel[3] = -1;
    if (point) {
        // the reference's Point_Specific: x = (point[0] + 0.5) / H * h + 0.5 on the replicate-padded grid [h + 2, w + 2], corners
        // at floor / floor + 1; a padded index k is the query row clamp(k - 1, 0, h - 1)
        const double p0 = point[0], p1 = point[1];
        if (!(p0 >= 0.0 && p0 < H && p1 >= 0.0 && p1 < W)) return fail(MIRX_EINVAL, "simcam: point outside [0, H) x [0, W)");
        const double xf = (p0 + 0.5) / H * h + 0.5, yf = (p1 + 0.5) / W * w + 0.5;
        const int xm = (int)floor(xf), ym = (int)floor(yf);
        if (xm < 0 || ym < 0 || xm + 1 > h + 1 || ym + 1 > w + 1) return fail(MIRX_EINVAL, "simcam: point maps outside the padded grid");
        const double dx = xf - xm, dy = yf - ym;
        const int xs[4] = {xm, xm + 1, xm, xm + 1}, ys[4] = {ym, ym, ym + 1, ym + 1};
        const double wx[4] = {1.0 - dx, dx, 1.0 - dx, dx}, wy[4] = {1.0 - dy, 1.0 - dy, dy, dy};
        for (int k = 0; k < 4; ++k) {
            const int rr = std::min(std::max(xs[k] - 1, 0), h - 1), cc = std::min(std::max(ys[k] - 1, 0), w - 1);
            pa.sel[k] = rr * w + cc;
            ma.wt[k][0] = (float)wx[k];
            ma.wt[k][1] = (float)wy[k];
        }
        ma.point = 1;
    }
    if (pairs == 0) return MIRX_OK;
    if (!q || !r || !workspace || !out) return fail(MIRX_EINVAL, "simcam: null buffer");
    const int nt = simcam_tiles(hw);
    if (workspace_floats < pairs * ws_pair_floats(nt)) return fail(MIRX_EINVAL, "simcam: workspace smaller than mirx_simcam_workspace_floats()");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    pa.q = q;
    pa.r = r;
    pa.hw = hw;
    pa.c = c;
    pa.pair_stride = pair_stride;
    pa.nt = nt;
    pa.ws = workspace;
    hipLaunchKernelGGL(k_simcam_pairs, dim3(nt * nt, (unsigned)pairs), dim3(SC_THREADS), 0, st, pa);
    MIRX_HIP(hipGetLastError());
    ma.ws = workspace;
    ma.hw = hw;
    ma.h = h;
    ma.w = w;
    ma.nt = nt;
    ma.H = H;
    ma.W = W;
    ma.eps = eps;
    ma.first_map = maps == MIRX_SIMCAM_MAPS_BOTH ? 0 : 1;
    ma.nmaps = maps == MIRX_SIMCAM_MAPS_BOTH ? 2 : 1;
    ma.out = out;
    const dim3 grid((H + SC_MAP_ROWS - 1) / SC_MAP_ROWS, ma.nmaps, (unsigned)pairs);
    hipLaunchKernelGGL(k_simcam_maps, grid, dim3(SC_THREADS), hw * sizeof(float), st, ma);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}

extern "C" int mirx_bn_relu_rows(const float *x, int64_t b, int64_t c, int64_t hw, const float *scale, const float *shift, float *out,
                                 void *stream) {
    if (b < 0 || b > 65535 || c < 1 || c > (1 << 20) || hw < 1 || hw > (1 << 24)) return fail(MIRX_EINVAL, "bn_relu_rows: bad b / c / hw");
    if (b == 0) return MIRX_OK;
    if (!x || !scale || !shift || !out) return fail(MIRX_EINVAL, "bn_relu_rows: null buffer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_bn_relu_rows, dim3((unsigned)((hw + 31) / 32), (unsigned)((c + 31) / 32), (unsigned)b), dim3(256), 0, st, x, c, hw,
                       scale, shift, out);
    MIRX_HIP(hipGetLastError());
    return MIRX_OK;
}
