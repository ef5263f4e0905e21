// k_ivf.hip -- the kernels of the IVF indexes (mirx_ivf.hip, include/mirx.h): the probe table inverted into list order, one
// launch that scores every (query, probed list) pair in fp64, the top-k of a query's compact score row, the k-means update, and
// IVF_SQ8's quantiser (per-column range, encode, decode); the list scan reads fp32 rows or 8-bit code rows from one source.
// Every score comes from the transposed lane tree of k_scores_f64_lds (k_exact.hip), so it has the bits of oracle/search_ref.c;
// the integer atomics below only hand out slots that their owners alone write, so no result depends on their order.
//
// Reference behaviour replaced (paths into /root/reference):
//   index_params = {"index_type": "IVF_FLAT", "params": {"nlist": 1024}}        milvus/milvus_setup.py:191-213
//   collection.search(..., param={"params": {"nprobe": 10}})                    milvus/milvus_retrieval.py:69-86
//   index_type: 'IVF_FLAT', 'IVF_SQ8', 'IVF_PQ', 'HNSW', 'FLAT'                  milvus/milvus_setup.py:191-213
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

namespace mirx {

namespace {

// ---- row moves ------------------------------------------------------------------------------------------------------------------
// dst row (dst_pos ? dst_pos[i] : i) = src row (src_pos ? src_pos[i] : i), `cols` elements, the rest of the dst row zeroed; a
// negative dst_pos drops the row.  One workgroup walks rows, a thread a column: the layout changes of add / remove / re-assign.
// T = float for fp32 rows, uint32_t for code rows (four codes a word).
template <typename T>
__global__ __launch_bounds__(256) void k_ivf_place(const T *__restrict__ src, int64_t n, int src_ld, int cols,
                                                   const int64_t *__restrict__ src_pos, const int64_t *__restrict__ dst_pos,
                                                   T *__restrict__ dst, int dst_ld) {
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t d = dst_pos ? dst_pos[i] : i;
        if (d < 0) continue;
        const T *s = src + (src_pos ? src_pos[i] : i) * src_ld;
        T *o = dst + d * dst_ld;
        for (int c = threadIdx.x; c < dst_ld; c += 256) o[c] = c < cols ? s[c] : T(0);
    }
}

__global__ __launch_bounds__(256) void k_ivf_place_ids(const int64_t *__restrict__ src, int64_t n,
                                                       const int64_t *__restrict__ dst_pos, int64_t *__restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t d = dst_pos[i];
        if (d >= 0) dst[d] = src[i];
    }
}

// ---- the SQ8 quantiser ------------------------------------------------------------------------------------------------------------
// code = min(255, max(0, floor(((double)x - vmin) / scale + 0.5))), NaN and a zero scale -> 0; xhat = (float)(vmin + code * scale)
// with the product exact in double (8 x 24 bits), so the fma below rounds once to double as the sum does, then once to float.
__device__ __forceinline__ uint32_t sq8_encode(float x, float vmin, float scale) {
    if (scale == 0.f) return 0u;
    const double t = ((double)x - (double)vmin) / (double)scale;
    const double r = floor(t + 0.5);
    if (!(r >= 0.0)) return 0u;                                                    // NaN too
    return r > 255.0 ? 255u : (uint32_t)r;
}
__device__ __forceinline__ float sq8_decode(uint32_t code, double vmin, double scale) {
    return (float)fma((double)code, scale, vmin);
}

// Per-column min / max over rows [n, dim], NaN ignored (every comparison with it is false).  Workgroup b folds rows b, b + grid,
// ... into part[b] = [2][dim]; k_sq8_range folds the partials in workgroup order: no atomics, every call the same bits.
__global__ __launch_bounds__(256) void k_sq8_minmax(const float *__restrict__ rows, int64_t n, int dim, float *__restrict__ part) {
    for (int c = threadIdx.x; c < dim; c += 256) {
        float mn = INFINITY, mx = -INFINITY;
        for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
            const float v = rows[i * dim + c];
            if (v < mn) mn = v;
            if (v > mx) mx = v;
        }
        part[((int64_t)blockIdx.x * 2 + 0) * dim + c] = mn;
        part[((int64_t)blockIdx.x * 2 + 1) * dim + c] = mx;
    }
}

// vmin[c], scale[c] = (float)(((double)vmax - (double)vmin) / 255) from nparts partials; columns dim .. dimp-1 and a column
// without a number get vmin = scale = 0; a zero minimum is stored as +0 (min does not order the two zeros).
__global__ __launch_bounds__(256) void k_sq8_range(const float *__restrict__ part, int nparts, int dim, int dimp,
                                                   float *__restrict__ vmin, float *__restrict__ scale) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= dimp) return;
    float mn = INFINITY, mx = -INFINITY;
    if (c < dim)
        for (int b = 0; b < nparts; ++b) {
            const float a = part[((int64_t)b * 2 + 0) * dim + c], z = part[((int64_t)b * 2 + 1) * dim + c];
            if (a < mn) mn = a;
            if (z > mx) mx = z;
        }
    const bool any = mn <= mx;
    vmin[c] = any ? mn + 0.f : 0.f;
    scale[c] = any ? (float)(((double)mx - (double)mn) / 255.0) : 0.f;
}

// rows [n, cols] fp32 -> code rows of dst_ld bytes (a multiple of 4) at dst row (dst_pos ? dst_pos[i] : i), a thread four columns
// and one 4-byte store; columns cols .. dst_ld-1 hold code 0.  k_ivf_place of the code master.
__global__ __launch_bounds__(256) void k_sq8_encode_place(const float *__restrict__ src, int64_t n, int cols,
                                                          const float *__restrict__ vmin, const float *__restrict__ scale,
                                                          const int64_t *__restrict__ dst_pos, uint8_t *__restrict__ dst,
                                                          int dst_ld) {
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t d = dst_pos ? dst_pos[i] : i;
        if (d < 0) continue;
        const float *s = src + i * cols;
        uint32_t *o = reinterpret_cast<uint32_t *>(dst + d * dst_ld);
        for (int w = threadIdx.x; w < (dst_ld >> 2); w += 256) {
            uint32_t word = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * w + e;
                if (c < cols) word |= sq8_encode(s[c], vmin[c], scale[c]) << (8 * e);
            }
            o[w] = word;
        }
    }
}

// code rows of src_ld bytes -> fp32 rows [n, cols]
__global__ __launch_bounds__(256) void k_sq8_decode(const uint8_t *__restrict__ src, int64_t n, int src_ld, int cols,
                                                    const float *__restrict__ vmin, const float *__restrict__ scale,
                                                    float *__restrict__ dst) {
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
        for (int c = threadIdx.x; c < cols; c += 256)
            dst[i * cols + c] = sq8_decode(src[i * src_ld + c], (double)vmin[c], (double)scale[c]);
}

// ---- k-means update -------------------------------------------------------------------------------------------------------------
// One workgroup per list, one thread per column: ONE fp64 accumulator over the list's rows in ascending row order (order[] holds
// the rows sorted by list, stable), divided by the count and rounded once to fp32.  An empty list copies its centroid.
__global__ __launch_bounds__(256) void k_ivf_update(const float *__restrict__ rows, int dim, const int32_t *__restrict__ order,
                                                    const int64_t *__restrict__ loff, const float *__restrict__ cent,
                                                    float *__restrict__ out) {
    const int l = blockIdx.x;
    const int64_t b = loff[l], e = loff[l + 1];
    for (int c = threadIdx.x; c < dim; c += 256) {
        if (e == b) {
            out[(int64_t)l * dim + c] = cent[(int64_t)l * dim + c];
            continue;
        }
        double acc = 0.0;
        for (int64_t i = b; i < e; ++i) acc += (double)rows[(int64_t)order[i] * dim + c];
        out[(int64_t)l * dim + c] = (float)(acc / (double)(e - b));
    }
}

// cent[l] = upd[l] for the lists that hold rows (an empty list keeps its centroid's bits, whatever the normalisation did to upd)
__global__ __launch_bounds__(256) void k_ivf_keep(const float *__restrict__ upd, const int64_t *__restrict__ loff, int dim,
                                                  float *__restrict__ cent) {
    const int l = blockIdx.x;
    if (loff[l + 1] == loff[l]) return;
    for (int c = threadIdx.x; c < dim; c += 256) cent[(int64_t)l * dim + c] = upd[(int64_t)l * dim + c];
}

// ---- the probe table, inverted ---------------------------------------------------------------------------------------------------
// One wave per query: its probes as int32, the offset of every probed list inside the query's compact score row (the lists
// concatenated in probe order: an exclusive scan of their sizes, qoff[nprobe] = the row's length) and the histogram of the lists.
__global__ __launch_bounds__(64) void k_ivf_probes(const int64_t *__restrict__ pids, int nq, int nprobe,
                                                   const int64_t *__restrict__ offsets, int nlist, int32_t *__restrict__ probes,
                                                   int32_t *__restrict__ out_probes, int32_t *__restrict__ qoff,
                                                   int *__restrict__ cnt) {
    const int q = blockIdx.x, lane = lane_id();
    int carry = 0;
    for (int base = 0; base < nprobe; base += WAVE) {
        const int p = base + lane;
        int l = -1, sz = 0;
        if (p < nprobe) {
            const int64_t v = pids[(int64_t)q * nprobe + p];
            l = (v >= 0 && v < nlist) ? (int)v : -1;
            if (l >= 0) {
                sz = (int)(offsets[l + 1] - offsets[l]);
                atomicAdd(&cnt[l], 1);
            }
            probes[(int64_t)q * nprobe + p] = l;
            if (out_probes) out_probes[(int64_t)q * nprobe + p] = l;
        }
        int incl = sz;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int o = __shfl_up(incl, off, WAVE);
            if (lane >= off) incl += o;
        }
        if (p < nprobe) qoff[(int64_t)q * (nprobe + 1) + p] = carry + incl - sz;
        carry += __shfl(incl, WAVE - 1, WAVE);
    }
    if (lane == 0) qoff[(int64_t)q * (nprobe + 1) + nprobe] = carry;
}

// One wave: exclusive scans over the lists of the pair counts (pairoff) and of the work items (itemoff), a list of `size` rows
// that cnt queries probe giving ceil(size / IVF_ROWS) * ceil(cnt / qt) items; the search's counters go up by the batch's.
__global__ __launch_bounds__(64) void k_ivf_scan(const int *__restrict__ cnt, const int64_t *__restrict__ offsets, int nlist, int qt,
                                                 int32_t *__restrict__ pairoff, int32_t *__restrict__ itemoff,
                                                 unsigned long long *__restrict__ stats) {
    const int lane = lane_id();
    const int per = (nlist + WAVE - 1) / WAVE;
    const int l0 = lane * per < nlist ? lane * per : nlist, l1 = l0 + per < nlist ? l0 + per : nlist;
    int pairs = 0, items = 0;
    unsigned long long scored = 0;
    for (int l = l0; l < l1; ++l) {
        const int c = cnt[l];
        const int64_t sz = offsets[l + 1] - offsets[l];
        pairs += c;
        items += (int)((sz + IVF_ROWS - 1) / IVF_ROWS) * ((c + qt - 1) / qt);
        scored += (unsigned long long)c * (unsigned long long)sz;
    }
    int ip = pairs, ii = items;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int a = __shfl_up(ip, off, WAVE), b = __shfl_up(ii, off, WAVE);
        if (lane >= off) { ip += a; ii += b; }
    }
    int pbase = ip - pairs, ibase = ii - items;
    for (int l = l0; l < l1; ++l) {
        const int c = cnt[l];
        const int64_t sz = offsets[l + 1] - offsets[l];
        pairoff[l] = pbase;
        itemoff[l] = ibase;
        pbase += c;
        ibase += (int)((sz + IVF_ROWS - 1) / IVF_ROWS) * ((c + qt - 1) / qt);
    }
    if (lane == WAVE - 1) {
        pairoff[nlist] = ip;
        itemoff[nlist] = ii;
        atomicAdd(&stats[1], (unsigned long long)ip);
        atomicAdd(&stats[2], (unsigned long long)ii);
    }
    if (scored) atomicAdd(&stats[0], scored);
}

// Every (query, probe) pair takes the next slot of its list: the slot's query and the pair's offset in that query's compact row.
__global__ __launch_bounds__(256) void k_ivf_scatter(const int32_t *__restrict__ probes, const int32_t *__restrict__ qoff, int nq,
                                                     int nprobe, const int32_t *__restrict__ pairoff, int *__restrict__ cursor,
                                                     int32_t *__restrict__ pair_q, int32_t *__restrict__ pair_off) {
    const int64_t total = (int64_t)nq * nprobe;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int l = probes[i];
        if (l < 0) continue;
        const int q = (int)(i / nprobe), p = (int)(i - (int64_t)q * nprobe);
        const int slot = pairoff[l] + atomicAdd(&cursor[l], 1);
        pair_q[slot] = q;
        pair_off[slot] = qoff[(int64_t)q * (nprobe + 1) + p];
    }
}

// ---- the list scan ----------------------------------------------------------------------------------------------------------------
// A work item = (a list, IVF_ROWS of its rows, up to qt of the queries that probe it).  The item's queries sit in LDS as doubles,
// each of the four waves walks 64 rows, four at a time, and reduces them transposed exactly as k_scores_f64_lds does (the same
// association of every sum), so the rows stream once per query group and not once per query.  The grid is persistent: workgroup b
// takes items b, b + gridDim.x, ...; consecutive items of a list share its rows (the query group is the fast index), so
// workgroups that run side by side read the same lines.  The score of (query, row) goes to the query's compact row at the pair's
// offset + the row's position in its list: every entry has one writer.
// SQ8: `rows` are code rows of dimp bytes.  A lane's chunk is one 4-byte load of four codes (the fp32 rows' lane-to-column map),
// decoded once per row group to the fp32 values k_sq8_decode gives, with the lane's (double) vmin and scale held in registers for
// the whole launch; from there on the two forms are the same instructions, so a score has the bits of the decoded row's.
template <int METRIC, int CPL, bool SQ8>
__global__ __launch_bounds__(256, 2) void k_ivf_scores(const float *__restrict__ q32p, const void *__restrict__ rows,
                                                       const float *__restrict__ vmin, const float *__restrict__ scale, int dimp,
                                                       const int64_t *__restrict__ offsets, int nlist, int qt,
                                                       const int32_t *__restrict__ pairoff, const int32_t *__restrict__ itemoff,
                                                       const int32_t *__restrict__ pair_q, const int32_t *__restrict__ pair_off,
                                                       double *__restrict__ out, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *qs = reinterpret_cast<double *>(smem);                                 // [qt][dimp]
    int32_t *sq = reinterpret_cast<int32_t *>(smem + (size_t)qt * dimp * 8);       // [16] the item's queries
    int32_t *so = sq + 16;                                                         // [16] and their pair offsets
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int nchunk = dimp >> 2;
    const int sel_hi = lane >> 5, sel_16 = (lane >> 4) & 1;
    const int my_row_in4 = sel_hi + 2 * sel_16;
    const int total = itemoff[nlist];
    double dmin[SQ8 ? 4 * CPL : 1], dscale[SQ8 ? 4 * CPL : 1];
    if (SQ8) {
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int chunk = lane + WAVE * c;
            const bool in = chunk < nchunk;
            const float4 a = in ? *reinterpret_cast<const float4 *>(vmin + 4 * chunk) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 b = in ? *reinterpret_cast<const float4 *>(scale + 4 * chunk) : make_float4(0.f, 0.f, 0.f, 0.f);
            dmin[4 * c] = (double)a.x; dmin[4 * c + 1] = (double)a.y; dmin[4 * c + 2] = (double)a.z; dmin[4 * c + 3] = (double)a.w;
            dscale[4 * c] = (double)b.x; dscale[4 * c + 1] = (double)b.y; dscale[4 * c + 2] = (double)b.z; dscale[4 * c + 3] = (double)b.w;
        }
    }
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        int lo = 0, hi = nlist;                                                    // itemoff[lo] <= item < itemoff[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (itemoff[mid] <= item) lo = mid; else hi = mid;
        }
        const int l = lo, local = item - itemoff[l];
        const int64_t first = offsets[l];
        const int n = (int)(offsets[l + 1] - first);
        const int p0 = pairoff[l], cnt = pairoff[l + 1] - p0;
        const int nqg = (cnt + qt - 1) / qt;
        const int rb = local / nqg, qg = local - rb * nqg;
        const int nloc = (cnt - qg * qt) < qt ? (cnt - qg * qt) : qt;
        __syncthreads();                                                           // the previous item's reads of qs / sq / so
        if (threadIdx.x < 16) {
            const bool live = (int)threadIdx.x < nloc;
            sq[threadIdx.x] = live ? pair_q[p0 + qg * qt + threadIdx.x] : 0;
            so[threadIdx.x] = live ? pair_off[p0 + qg * qt + threadIdx.x] : 0;
        }
        for (int i = threadIdx.x; i < qt * dimp; i += 256) {
            const int t = i / dimp, e = i - t * dimp;
            qs[i] = t < nloc ? (double)q32p[(int64_t)pair_q[p0 + qg * qt + t] * dimp + e] : 0.0;
        }
        __syncthreads();
        const int r0 = rb * IVF_ROWS + wave * 64;                                  // this wave's 64 rows, counted inside the list
        if (r0 >= n) continue;                                                     // (no barrier is skipped: both are behind us)
        const float *g32 = static_cast<const float *>(rows) + (SQ8 ? 0 : first * dimp);
        const uint8_t *g8 = static_cast<const uint8_t *>(rows) + (SQ8 ? first * dimp : 0);
        double keep[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) keep[t] = 0.0;
        for (int grp = 0; grp < 16; ++grp) {                                       // 4 rows per group
            const int rg = r0 + grp * 4;
            if (rg >= n) break;
            float4 gv[4][CPL];
            uint32_t gw[SQ8 ? 4 : 1][CPL];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = rg + r < n ? rg + r : n - 1;                   // clamp: results of rows >= n are not stored
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const int chunk = lane + WAVE * c;
                    if (SQ8)
                        gw[r][c] = chunk < nchunk ? *reinterpret_cast<const uint32_t *>(g8 + row * dimp + 4 * chunk) : 0u;
                    else
                        gv[r][c] = chunk < nchunk ? *reinterpret_cast<const float4 *>(g32 + row * dimp + 4 * chunk)
                                                  : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            if (SQ8) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < CPL; ++c) {
                        const uint32_t w = gw[r][c];
                        gv[r][c] = make_float4(sq8_decode(w & 255u, dmin[4 * c], dscale[4 * c]),
                                               sq8_decode((w >> 8) & 255u, dmin[4 * c + 1], dscale[4 * c + 1]),
                                               sq8_decode((w >> 16) & 255u, dmin[4 * c + 2], dscale[4 * c + 2]),
                                               sq8_decode(w >> 24, dmin[4 * c + 3], dscale[4 * c + 3]));
                    }
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                if (t >= nloc) continue;
                double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const int chunk = lane + WAVE * c;
                    double qv[4] = {0.0, 0.0, 0.0, 0.0};
                    if (chunk < nchunk) {
                        const double2 a = *reinterpret_cast<const double2 *>(qs + (int64_t)t * dimp + 4 * chunk);
                        const double2 b = *reinterpret_cast<const double2 *>(qs + (int64_t)t * dimp + 4 * chunk + 2);
                        qv[0] = a.x; qv[1] = a.y; qv[2] = b.x; qv[3] = b.y;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double gd[4] = {(double)gv[r][c].x, (double)gv[r][c].y, (double)gv[r][c].z, (double)gv[r][c].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (METRIC == 0) {
                                p[r] = fma(qv[e], gd[e], p[r]);
                            } else {
                                const double d = qv[e] - gd[e];
                                p[r] = fma(d, d, p[r]);
                            }
                        }
                    }
                }
                // the lane tree's levels off = 32 and off = 16, transposed: afterwards each quarter of the wave carries one row
                const double k01 = sel_hi ? p[1] : p[0], s01 = sel_hi ? p[0] : p[1];
                const double k23 = sel_hi ? p[3] : p[2], s23 = sel_hi ? p[2] : p[3];
                const double a01 = k01 + __shfl_xor(s01, 32, 64);
                const double a23 = k23 + __shfl_xor(s23, 32, 64);
                const double kk = sel_16 ? a23 : a01, ss = sel_16 ? a01 : a23;
                double v = kk + __shfl_xor(ss, 16, 64);
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
                if (METRIC == 1) v = -v;
                if ((lane & 15) == grp) keep[t] = v;
            }
        }
        const int orow = r0 + 4 * (lane & 15) + my_row_in4;                        // the row this lane holds for every query
        if (orow < n) {
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (t < nloc) out[(int64_t)sq[t] * ld + so[t] + orow] = keep[t];
        }
    }
}

// ---- top-k of a compact score row -------------------------------------------------------------------------------------------------
// k_row_topk (k_exact.hip) on a row whose entry j belongs to row (j - qoff[p]) of probed list p: the id comes from the list, so
// the tie rule sees ids, never positions.
constexpr int IVF_TK_TOTAL = 2048;   // LDS records: kp sorted + (IVF_TK_TOTAL - kp) pending, kp <= 1024

__global__ __launch_bounds__(256) void k_ivf_topk(const double *__restrict__ scores, int64_t ld, const int32_t *__restrict__ probes,
                                                  const int32_t *__restrict__ qoff, int nprobe, const int64_t *__restrict__ offsets,
                                                  const int64_t *__restrict__ ids, const int64_t *__restrict__ exclude, int k, int kp,
                                                  int metric, double *__restrict__ out_f64, int64_t *__restrict__ out_ids,
                                                  float *__restrict__ out_val) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Hit *best = reinterpret_cast<Hit *>(smem);
    int *pend_cnt = reinterpret_cast<int *>(smem + (size_t)IVF_TK_TOTAL * sizeof(Hit));
    const int round = IVF_TK_TOTAL - kp;
    const int64_t qi = blockIdx.x;
    const int64_t ex = exclude ? exclude[qi] : -1;
    const double *row = scores + qi * ld;
    const int32_t *qo = qoff + qi * (nprobe + 1);
    const int32_t *pr = probes + qi * nprobe;
    const int n = qo[nprobe];
    for (int i = threadIdx.x; i < kp; i += 256) { best[i].s = -INFINITY; best[i].id = ID_LAST; }
    for (int base = 0; base < n; base += round) {
        if (threadIdx.x == 0) *pend_cnt = 0;
        __syncthreads();
        const Hit kth = best[k - 1];
        for (int e = threadIdx.x; e < round; e += 256) {
            const int j = base + e;
            if (j < n) {
                int lo = 0, hi = nprobe;                                           // qo[lo] <= j < qo[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (qo[mid] <= j) lo = mid; else hi = mid;
                }
                const double s = row[j];
                const int64_t id = ids[offsets[pr[lo]] + (j - qo[lo])];
                if (id != ex && hit_before(s, id, kth.s, kth.id)) {
                    const int p = atomicAdd(pend_cnt, 1);
                    best[kp + p].s = s;
                    best[kp + p].id = id;
                }
            }
        }
        __syncthreads();
        const int c = *pend_cnt;
        if (c > 0) {
            const int m = pow2_ceil(kp + c);
            for (int i = kp + c + threadIdx.x; i < m; i += 256) { best[i].s = -INFINITY; best[i].id = ID_LAST; }
            bitonic_lds(best, m, [](const Hit &x, const Hit &y) { return hit_before(x.s, x.id, y.s, y.id); });
        }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < k; r += 256) {
        const Hit h = best[r];
        const bool empty = h.id == ID_LAST;
        if (out_f64) out_f64[qi * k + r] = empty ? -INFINITY : h.s;
        out_ids[qi * k + r] = empty ? -1 : h.id;
        if (out_val) out_val[qi * k + r] = empty ? -INFINITY : reported_value(h.s, metric);
    }
}

template <int METRIC, bool SQ8>
hipError_t launch_ivf_scores_t(const IvfScoreArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.qt * a.dimp * sizeof(double) + 32 * sizeof(int32_t);
    const unsigned grid = (unsigned)current_device_cus() * 4;
#define MIRX_IVF_LAUNCH(CPL)                                                                                                   \
    {                                                                                                                          \
        hipError_t e = set_dynamic_lds(k_ivf_scores<METRIC, CPL, SQ8>, lds);                                                   \
        if (e != hipSuccess) return e;                                                                                         \
        hipLaunchKernelGGL((k_ivf_scores<METRIC, CPL, SQ8>), dim3(grid), dim3(256), lds, st, a.q32p, a.rows, a.vmin, a.scale,  \
                           a.dimp, a.offsets, a.nlist, a.qt, a.pairoff, a.itemoff, a.pair_q, a.pair_off, a.out, a.ld);         \
    }
    if (a.dimp <= 256) MIRX_IVF_LAUNCH(1)
    else if (a.dimp <= 512) MIRX_IVF_LAUNCH(2)
    else if (a.dimp <= 1024) MIRX_IVF_LAUNCH(4)
    else MIRX_IVF_LAUNCH(8)
#undef MIRX_IVF_LAUNCH
    return hipGetLastError();
}

}  // namespace

int ivf_query_tile(int dimp) {
    const int qt = IVF_LDS_BYTES / (dimp * 8);
    return qt > 16 ? 16 : qt;
}

hipError_t launch_ivf_place(const float *src, int64_t n, int src_ld, int cols, const int64_t *src_pos, const int64_t *dst_pos,
                            float *dst, int dst_ld, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(k_ivf_place<float>, dim3(grid), dim3(256), 0, st, src, n, src_ld, cols, src_pos, dst_pos, dst, dst_ld);
    return hipGetLastError();
}

hipError_t launch_ivf_place_codes(const uint8_t *src, int64_t n, int ld, const int64_t *dst_pos, uint8_t *dst, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(k_ivf_place<uint32_t>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(src), n, ld >> 2,
                       ld >> 2, nullptr, dst_pos, reinterpret_cast<uint32_t *>(dst), ld >> 2);
    return hipGetLastError();
}

int sq8_minmax_parts(int64_t n) { return (int)(n < 1024 ? n : 1024); }

hipError_t launch_sq8_range(const float *rows, int64_t n, int dim, int dimp, float *part, float *vmin, float *scale,
                            hipStream_t st) {
    const int parts = sq8_minmax_parts(n);
    hipLaunchKernelGGL(k_sq8_minmax, dim3(parts), dim3(256), 0, st, rows, n, dim, part);
    hipLaunchKernelGGL(k_sq8_range, dim3((dimp + 255) / 256), dim3(256), 0, st, part, parts, dim, dimp, vmin, scale);
    return hipGetLastError();
}

hipError_t launch_sq8_encode_place(const float *src, int64_t n, int cols, const float *vmin, const float *scale,
                                   const int64_t *dst_pos, uint8_t *dst, int dst_ld, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(k_sq8_encode_place, dim3(grid), dim3(256), 0, st, src, n, cols, vmin, scale, dst_pos, dst, dst_ld);
    return hipGetLastError();
}

hipError_t launch_sq8_decode(const uint8_t *src, int64_t n, int src_ld, int cols, const float *vmin, const float *scale,
                             float *dst, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(k_sq8_decode, dim3(grid), dim3(256), 0, st, src, n, src_ld, cols, vmin, scale, dst);
    return hipGetLastError();
}

hipError_t launch_ivf_place_ids(const int64_t *src, int64_t n, const int64_t *dst_pos, int64_t *dst, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_ivf_place_ids, dim3(grid), dim3(256), 0, st, src, n, dst_pos, dst);
    return hipGetLastError();
}

hipError_t launch_ivf_update(const float *rows, int dim, const int32_t *order, const int64_t *loff, int nlist, float *cent,
                             float *upd, bool normalize, hipStream_t st) {
    hipLaunchKernelGGL(k_ivf_update, dim3(nlist), dim3(256), 0, st, rows, dim, order, loff, cent, upd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (normalize && (e = launch_l2_normalize(upd, nlist, dim, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ivf_keep, dim3(nlist), dim3(256), 0, st, upd, loff, dim, cent);
    return hipGetLastError();
}

hipError_t launch_ivf_probes(const int64_t *pids, int nq, int nprobe, const int64_t *offsets, int nlist, int32_t *probes,
                             int32_t *out_probes, int32_t *qoff, int *cnt, hipStream_t st) {
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)nlist * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ivf_probes, dim3(nq), dim3(64), 0, st, pids, nq, nprobe, offsets, nlist, probes, out_probes, qoff, cnt);
    return hipGetLastError();
}

hipError_t launch_ivf_invert(const int64_t *pids, int nq, int nprobe, const int64_t *offsets, int nlist, int qt, int32_t *probes,
                             int32_t *out_probes, int32_t *qoff, int *cnt_cursor, int32_t *pairoff, int32_t *itemoff,
                             int32_t *pair_q, int32_t *pair_off, unsigned long long *stats, hipStream_t st) {
    hipError_t e = hipMemsetAsync(cnt_cursor, 0, (size_t)2 * nlist * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ivf_probes, dim3(nq), dim3(64), 0, st, pids, nq, nprobe, offsets, nlist, probes, out_probes, qoff,
                       cnt_cursor);
    hipLaunchKernelGGL(k_ivf_scan, dim3(1), dim3(64), 0, st, cnt_cursor, offsets, nlist, qt, pairoff, itemoff, stats);
    const int64_t total = (int64_t)nq * nprobe;
    const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_ivf_scatter, dim3(grid), dim3(256), 0, st, probes, qoff, nq, nprobe, pairoff, cnt_cursor + nlist, pair_q,
                       pair_off);
    return hipGetLastError();
}

hipError_t launch_ivf_scores(const IvfScoreArgs &a, int metric, hipStream_t st) {
    if (a.vmin) return metric == MIRX_METRIC_IP ? launch_ivf_scores_t<0, true>(a, st) : launch_ivf_scores_t<1, true>(a, st);
    return metric == MIRX_METRIC_IP ? launch_ivf_scores_t<0, false>(a, st) : launch_ivf_scores_t<1, false>(a, st);
}

hipError_t launch_ivf_topk(const double *scores, int64_t ld, const int32_t *probes, const int32_t *qoff, int nq, int nprobe,
                           const int64_t *offsets, const int64_t *ids, const int64_t *exclude, int k, int metric, double *out_f64,
                           int64_t *out_ids, float *out_val, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    int kp = 1;
    while (kp < k) kp <<= 1;
    if (kp > IVF_TK_TOTAL / 2) return hipErrorInvalidValue;
    const size_t lds = (size_t)IVF_TK_TOTAL * sizeof(Hit) + 16;
    hipLaunchKernelGGL(k_ivf_topk, dim3(nq), dim3(256), lds, st, scores, ld, probes, qoff, nprobe, offsets, ids, exclude, k, kp,
                       metric, out_f64, out_ids, out_val);
    return hipGetLastError();
}

}  // namespace mirx
