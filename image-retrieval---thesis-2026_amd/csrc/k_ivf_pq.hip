// k_ivf_pq.hip -- the kernels of IVF_PQ (mirx_ivf.hip, include/mirx.h): a query's asymmetric-distance tables, the scan of the
// probed lists' code rows against them, and the small moves around the code master (codes packed from the codeword search,
// codes decoded to their codewords), and the kernels of residual coding (mirx_ivf_create_pq_ex): residuals, the per-(query, list)
// bases, the row norms of L2 and the residual instantiations of the scan.  The lists, probes, compact score rows and their top-k are
// k_ivf.hip's, unchanged.
//
// A score is defined by its order of additions (include/mirx.h): a table entry is ONE sequential fp64 accumulator over the
// sub-space's columns, a row's score ONE sequential accumulator over the sub-quantisers, so the numpy restatement
// (tests/_pq_ref.py) has the same bits.  Nothing here is fused: L2's d * d is rounded before it is added.
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

namespace mirx {

namespace {

// ---- tables -----------------------------------------------------------------------------------------------------------------------
// One workgroup per (query, sub-quantiser), one thread per codeword: T[q][j][c] over the dsub columns of sub-space j, ascending.
// The query's sub-vector sits in LDS (dsub <= 512 floats); a thread streams its codeword as float4s.
template <int METRIC>
__global__ __launch_bounds__(256) void k_pq_tables(const float *__restrict__ q, int64_t nq, int dim, int m,
                                                   const float *__restrict__ cb, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float qs[PQ_MAX_DSUB];
    const int dsub = dim / m;
    const int64_t total = nq * m;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t qi = w / m;
        const int j = (int)(w - qi * m);
        __syncthreads();                                                           // the previous pair's reads of qs
        for (int e = threadIdx.x; e < dsub; e += 256) qs[e] = q[qi * dim + (int64_t)j * dsub + e];
        __syncthreads();
        const float4 *row = reinterpret_cast<const float4 *>(cb + ((int64_t)j * 256 + threadIdx.x) * dsub);
        double acc = 0.0;
        for (int e4 = 0; e4 < (dsub >> 2); ++e4) {
            const float4 v = row[e4];
            const float cv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (METRIC == 0) {
                    acc = __dadd_rn(acc, __dmul_rn((double)qs[4 * e4 + e], (double)cv[e]));   // the product is exact
                } else {
                    const double d = __dsub_rn((double)qs[4 * e4 + e], (double)cv[e]);
                    acc = __dadd_rn(acc, __dmul_rn(d, d));                                    // rounded, then added
                }
            }
        }
        out[w * 256 + threadIdx.x] = acc;
    }
}

// ---- the work items of the scan ---------------------------------------------------------------------------------------------------
// One workgroup: itemoff[q] = the items before query q, a query of n entries giving ceil(n / PQ_ITEM_ROWS); the search's counters
// go up by the batch's rows scored (the entries), pairs (the histogram of k_ivf_probes) and items.
__global__ __launch_bounds__(256) void k_pq_items(const int32_t *__restrict__ qoff, int nq, int nprobe, const int *__restrict__ cnt,
                                                  int nlist, int32_t *__restrict__ itemoff, unsigned long long *__restrict__ stats) {
    __shared__ int part[256];
    __shared__ unsigned long long rows_s[256], pairs_s[256];
    const int t = threadIdx.x;
    const int per = (nq + 255) / 256;
    const int q0 = t * per < nq ? t * per : nq, q1 = q0 + per < nq ? q0 + per : nq;
    int items = 0;
    unsigned long long rows = 0, pairs = 0;
    for (int qi = q0; qi < q1; ++qi) {
        const int n = qoff[(int64_t)qi * (nprobe + 1) + nprobe];
        items += (n + PQ_ITEM_ROWS - 1) / PQ_ITEM_ROWS;
        rows += (unsigned long long)n;
    }
    for (int l = t; l < nlist; l += 256) pairs += (unsigned long long)cnt[l];
    part[t] = items;
    rows_s[t] = rows;
    pairs_s[t] = pairs;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        unsigned long long r = 0, p = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
            r += rows_s[i];
            p += pairs_s[i];
        }
        itemoff[nq] = run;
        atomicAdd(&stats[0], r);
        atomicAdd(&stats[1], p);
        atomicAdd(&stats[2], (unsigned long long)run);
    }
    __syncthreads();
    int base = part[t];
    for (int qi = q0; qi < q1; ++qi) {
        itemoff[qi] = base;
        base += (qoff[(int64_t)qi * (nprobe + 1) + nprobe] + PQ_ITEM_ROWS - 1) / PQ_ITEM_ROWS;
    }
}

// ---- the scan ---------------------------------------------------------------------------------------------------------------------
// A work item = (a query, PQ_ITEM_ROWS consecutive entries of its compact score row).  The shape is the opposite of k_ivf_scores':
// a query's table is m x 2 KiB and a row m bytes, so the TABLE is what a workgroup must amortise and the code rows are cheap to
// read again for every query.  The grid is persistent and every workgroup takes a CONTIGUOUS run of items -- items are numbered
// query by query, so a run stays on one query for as long as it can and T[q] is copied into LDS once per (workgroup, query).
// Each of the 1024 threads owns one entry of the item: it finds the entry's probed list in the query's nprobe + 1 offsets (as
// k_ivf_topk does), loads the row's m code bytes as words -- all of them before the first look-up -- and adds T[j][code[j]], j
// ascending, into one accumulator.  The entry has one writer.
// LDS layout: T[j][c] as the tables kernel left it, no padding and no stagger.  Every lane of a wave is at the same j at the same
// time, so lanes with EQUAL codes read one address (a broadcast) and lanes with different codes of one j spread over that j's 256
// entries = 32 bank pairs of a ds_read_b64 half-wave; staggering T[j] by j would move all lanes alike and change nothing.
// RES (residual coding, include/mirx.h): T is the IP table of the residual codebooks whatever the metric, and an entry's sum starts
// from the base of ITS OWN (query, probed list) -- base[qi * nprobe + lo], lo the slot the entry bisected -- so lanes of one wave
// start from different bases wherever a list boundary falls inside the wave.  L2 then reads the row's N2 beside its code row and
// ranks by -((QQ + N2) - 2 ip).  Without RES the three pointers are never read and the code is the raw form's.
template <int METRIC, bool V16, bool RES>
__global__ __launch_bounds__(PQ_ITEM_ROWS) void k_pq_scan(const double *__restrict__ tables, const uint8_t *__restrict__ codes, int m,
                                                           const int32_t *__restrict__ probes, const int32_t *__restrict__ qoff,
                                                           int nq, int nprobe, const int64_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ itemoff, double *__restrict__ out,
                                                           int64_t ld, const double *__restrict__ base,
                                                           const double *__restrict__ qq, const double *__restrict__ n2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *T = reinterpret_cast<double *>(smem);                                  // [m][256]
    const int total = itemoff[nq];
    const int chunk = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int i0 = (int)blockIdx.x * chunk;
    const int i1 = i0 + chunk < total ? i0 + chunk : total;
    if (i0 >= i1) return;
    int qi = 0;
    {
        int lo = 0, hi = nq;                                                       // itemoff[lo] <= i0 < itemoff[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (itemoff[mid] <= i0) lo = mid; else hi = mid;
        }
        qi = lo;
    }
    const int nw = m >> 2;                                                         // 4-code words of a row, <= 16
    int loaded = -1;
    for (int item = i0; item < i1; ++item) {
        while (itemoff[qi + 1] <= item) ++qi;                                      // queries without entries have no items
        if (qi != loaded) {
            __syncthreads();                                                       // the previous query's look-ups
            const double2 *src = reinterpret_cast<const double2 *>(tables + (int64_t)qi * m * 256);
            double2 *dst = reinterpret_cast<double2 *>(T);
            for (int i = threadIdx.x; i < m * 128; i += PQ_ITEM_ROWS) dst[i] = src[i];
            __syncthreads();
            loaded = qi;
        }
        const int32_t *qo = qoff + (int64_t)qi * (nprobe + 1);
        const int n = qo[nprobe];
        const int e = (item - itemoff[qi]) * PQ_ITEM_ROWS + (int)threadIdx.x;
        if (e >= n) continue;                                                      // (no barrier is skipped: they are behind us)
        int lo = 0, hi = nprobe;                                                   // qo[lo] <= e < qo[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (qo[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t pos = offsets[probes[(int64_t)qi * nprobe + lo]] + (e - qo[lo]);
        const uint8_t *row = codes + pos * m;
        uint32_t w[16];
        if (V16) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 v = 4 * i < nw ? reinterpret_cast<const uint4 *>(row)[i] : make_uint4(0u, 0u, 0u, 0u);
                w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] = i < nw ? reinterpret_cast<const uint32_t *>(row)[i] : 0u;
        }
        double s = RES ? base[(int64_t)qi * nprobe + lo] : 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < nw) {
                const double *Tj = T + (4 * i) * 256;
                s = s + Tj[w[i] & 255u];
                s = s + Tj[256 + ((w[i] >> 8) & 255u)];
                s = s + Tj[512 + ((w[i] >> 16) & 255u)];
                s = s + Tj[768 + (w[i] >> 24)];
            }
        }
        if (RES && METRIC != 0)                                                    // 2.0 * ip is exact; every step rounds once
            out[(int64_t)qi * ld + e] = -__dsub_rn(__dadd_rn(qq[qi], n2[pos]), __dmul_rn(2.0, s));
        else
            out[(int64_t)qi * ld + e] = METRIC == 0 ? s : -s;
    }
}

// ---- the code master's small moves ------------------------------------------------------------------------------------------------
// codes[i][j] = the codeword the search of sub-space j returned for row i (ids 0 .. 255)
__global__ __launch_bounds__(256) void k_pq_pack(const int64_t *__restrict__ found, int64_t n, int m, int j,
                                                 uint8_t *__restrict__ codes) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        codes[i * m + j] = (uint8_t)found[i];
}

// rows[i] = the row's m codewords, concatenated: exact fp32 copies
__global__ __launch_bounds__(256) void k_pq_decode(const uint8_t *__restrict__ codes, int64_t n, int dim, int m,
                                                   const float *__restrict__ cb, float *__restrict__ dst) {
    const int dsub = dim / m;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x)
        for (int c = threadIdx.x; c < dim; c += 256) {
            const int j = c / dsub, e = c - j * dsub;
            dst[i * dim + c] = cb[((int64_t)j * 256 + codes[i * m + j]) * dsub + e];
        }
}

// ---- residual coding (include/mirx.h, mirx_ivf_create_pq_ex) ----------------------------------------------------------------------
// dst[i][e] = rows[i][col0 + e] - cent[lists[i]][col0 + e], e < cols: one fp32 subtraction.  The column window lets the trainer
// write sub-space j's residuals straight into its [n, dsub] buffer and the encoder a chunk of whole rows.
__global__ __launch_bounds__(256) void k_pq_residual(const float *__restrict__ rows, int64_t n, int dim, int col0, int cols,
                                                     const int64_t *__restrict__ lists, const float *__restrict__ cent, int nlist,
                                                     float *__restrict__ dst, int dst_ld) {
    const int64_t total = n * cols;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / cols;
        const int e = (int)(idx - i * cols);
        const int64_t l = lists[i];
        float r = NAN;                                                             // no such list: nothing is read
        if (l >= 0 && l < nlist) r = __fsub_rn(rows[i * dim + col0 + e], cent[l * dim + col0 + e]);
        dst[i * dst_ld + e] = r;
    }
}

// One workgroup per query, the query in LDS.  A round takes 256 / m probe slots: thread (slot, j) streams sub-space j of the
// slot's centroid as float4s into P_j, ONE sequential accumulator; behind a barrier thread `slot` adds the m P_j, j ascending.
// The order of additions is the definition's; only who computes which P_j is free.  METRIC 1 adds QQ[q], the same sum of q * q.
template <int METRIC>
__global__ __launch_bounds__(256) void k_pq_base(const float *__restrict__ q, int64_t nq, int dim, int m,
                                                 const int32_t *__restrict__ lists, int nprobe, const float *__restrict__ cent,
                                                 int nlist, double *__restrict__ base, double *__restrict__ qq) {
    __shared__ float qs[MIRX_IVF_MAX_DIM];
    __shared__ double part[256];
    const int dsub = dim / m, t = threadIdx.x;
    const int per = 256 / m;                                                       // slots of a round, >= 4
    const int sl = t / m, j = t - sl * m;
    for (int64_t qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        __syncthreads();                                                           // the previous query's reads of qs
        for (int e = t; e < dim; e += 256) qs[e] = q[qi * dim + e];
        __syncthreads();
        for (int s0 = 0; s0 < nprobe; s0 += per) {
            const int s = s0 + sl;
            double acc = 0.0;
            if (sl < per && s < nprobe) {
                const int l = lists[qi * nprobe + s];
                if (l >= 0 && l < nlist) {
                    const float4 *row = reinterpret_cast<const float4 *>(cent + (int64_t)l * dim + (int64_t)j * dsub);
                    const float *qj = qs + j * dsub;
                    for (int e4 = 0; e4 < (dsub >> 2); ++e4) {
                        const float4 v = row[e4];
                        const float cv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc = __dadd_rn(acc, __dmul_rn((double)qj[4 * e4 + e], (double)cv[e]));   // the product is exact
                    }
                }
            }
            part[t] = acc;
            __syncthreads();
            if (t < per && s0 + t < nprobe) {
                double b = 0.0;
                for (int jj = 0; jj < m; ++jj) b = __dadd_rn(b, part[t * m + jj]);
                base[qi * nprobe + s0 + t] = b;
            }
            __syncthreads();                                                       // part is rewritten by the next round
        }
        if (METRIC != 0) {
            double acc = 0.0;
            if (t < m)
                for (int e = 0; e < dsub; ++e) acc = __dadd_rn(acc, __dmul_rn((double)qs[t * dsub + e], (double)qs[t * dsub + e]));
            part[t] = acc;
            __syncthreads();
            if (t == 0) {
                double b = 0.0;
                for (int jj = 0; jj < m; ++jj) b = __dadd_rn(b, part[jj]);
                qq[qi] = b;
            }
        }
    }
}

// N2 of coded rows: thread (row, j) of a round of 256 / m rows walks sub-space j of xh = centroid + codeword, the square rounded
// before it is added; thread `row` then adds the m partial sums, j ascending.
__global__ __launch_bounds__(256) void k_pq_norms(const uint8_t *__restrict__ codes, int64_t n, int dim, int m,
                                                  const int64_t *__restrict__ lists, const float *__restrict__ cent, int nlist,
                                                  const float *__restrict__ cb, double *__restrict__ n2) {
    __shared__ double part[256];
    const int dsub = dim / m, t = threadIdx.x;
    const int per = 256 / m;
    const int rl = t / m, j = t - rl * m;
    const int64_t rounds = (n + per - 1) / per;
    for (int64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const int64_t i = r * per + rl;
        double acc = 0.0;
        if (rl < per && i < n) {
            const int64_t l = lists[i];
            if (l >= 0 && l < nlist) {
                const float4 *c4 = reinterpret_cast<const float4 *>(cent + l * dim + (int64_t)j * dsub);
                const float4 *w4 = reinterpret_cast<const float4 *>(cb + ((int64_t)j * 256 + codes[i * m + j]) * dsub);
                for (int e4 = 0; e4 < (dsub >> 2); ++e4) {
                    const float4 c = c4[e4], w = w4[e4];
                    const float cv[4] = {c.x, c.y, c.z, c.w}, wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double xh = __dadd_rn((double)cv[e], (double)wv[e]);
                        acc = __dadd_rn(acc, __dmul_rn(xh, xh));                   // rounded, then added
                    }
                }
            } else {
                acc = NAN;
            }
        }
        part[t] = acc;
        __syncthreads();
        if (t < per && r * per + t < n) {
            double b = 0.0;
            for (int jj = 0; jj < m; ++jj) b = __dadd_rn(b, part[t * m + jj]);
            n2[r * per + t] = b;
        }
        __syncthreads();
    }
}

// rows[i] = (float)(centroid of the row's list + its codewords): one fp32 addition per column
__global__ __launch_bounds__(256) void k_pq_decode_residual(const uint8_t *__restrict__ codes, int64_t n, int dim, int m,
                                                            const float *__restrict__ cb, const int64_t *__restrict__ lists,
                                                            const float *__restrict__ cent, int nlist, float *__restrict__ dst) {
    const int dsub = dim / m;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t l = lists[i];
        for (int c = threadIdx.x; c < dim; c += 256) {
            const int j = c / dsub, e = c - j * dsub;
            float v = NAN;
            if (l >= 0 && l < nlist) v = __fadd_rn(cent[l * dim + c], cb[((int64_t)j * 256 + codes[i * m + j]) * dsub + e]);
            dst[i * dim + c] = v;
        }
    }
}

template <int METRIC, bool V16, bool RES>
hipError_t launch_pq_scan_t(const PqScanArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.m * 256 * sizeof(double);
    static std::atomic<unsigned long long> once{0};
    hipError_t e = set_dynamic_lds(k_pq_scan<METRIC, V16, RES>, (size_t)PQ_MAX_M * 256 * sizeof(double), &once);
    if (e != hipSuccess) return e;
    const int per_cu = lds * 2 <= PQ_CU_LDS_BYTES ? 2 : 1;                         // 1024 threads each: two workgroups fill a CU
    const unsigned grid = (unsigned)(current_device_cus() * per_cu);
    hipLaunchKernelGGL((k_pq_scan<METRIC, V16, RES>), dim3(grid), dim3(PQ_ITEM_ROWS), lds, st, a.tables, a.codes, a.m, a.probes,
                       a.qoff, a.nq, a.nprobe, a.offsets, a.itemoff, a.out, a.ld, a.base, a.qq, a.n2);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pq_tables(const float *q, int64_t nq, int dim, int m, int metric, const float *cb, double *out, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    const int64_t total = nq * m;
    const unsigned grid = (unsigned)(total < (1 << 20) ? total : (1 << 20));
    if (metric == MIRX_METRIC_IP)
        hipLaunchKernelGGL(k_pq_tables<0>, dim3(grid), dim3(256), 0, st, q, nq, dim, m, cb, out);
    else
        hipLaunchKernelGGL(k_pq_tables<1>, dim3(grid), dim3(256), 0, st, q, nq, dim, m, cb, out);
    return hipGetLastError();
}

hipError_t launch_pq_items(const int32_t *qoff, int nq, int nprobe, const int *cnt, int nlist, int32_t *itemoff,
                           unsigned long long *stats, hipStream_t st) {
    hipLaunchKernelGGL(k_pq_items, dim3(1), dim3(256), 0, st, qoff, nq, nprobe, cnt, nlist, itemoff, stats);
    return hipGetLastError();
}

hipError_t launch_pq_scan(const PqScanArgs &a, int metric, hipStream_t st) {
    if (a.base) {                                                                  // residual coding
        if (metric != MIRX_METRIC_IP && (!a.qq || !a.n2)) return hipErrorInvalidValue;
        if (a.m % 16 == 0)
            return metric == MIRX_METRIC_IP ? launch_pq_scan_t<0, true, true>(a, st) : launch_pq_scan_t<1, true, true>(a, st);
        return metric == MIRX_METRIC_IP ? launch_pq_scan_t<0, false, true>(a, st) : launch_pq_scan_t<1, false, true>(a, st);
    }
    if (a.m % 16 == 0)
        return metric == MIRX_METRIC_IP ? launch_pq_scan_t<0, true, false>(a, st) : launch_pq_scan_t<1, true, false>(a, st);
    return metric == MIRX_METRIC_IP ? launch_pq_scan_t<0, false, false>(a, st) : launch_pq_scan_t<1, false, false>(a, st);
}

hipError_t launch_pq_pack(const int64_t *found, int64_t n, int m, int j, uint8_t *codes, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_pq_pack, dim3(grid), dim3(256), 0, st, found, n, m, j, codes);
    return hipGetLastError();
}

hipError_t launch_pq_decode(const uint8_t *codes, int64_t n, int dim, int m, const float *cb, float *dst, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(k_pq_decode, dim3(grid), dim3(256), 0, st, codes, n, dim, m, cb, dst);
    return hipGetLastError();
}

hipError_t launch_pq_residual(const float *rows, int64_t n, int dim, int col0, int cols, const int64_t *lists, const float *cent,
                              int nlist, float *dst, int dst_ld, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n * cols + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
    hipLaunchKernelGGL(k_pq_residual, dim3(grid), dim3(256), 0, st, rows, n, dim, col0, cols, lists, cent, nlist, dst, dst_ld);
    return hipGetLastError();
}

hipError_t launch_pq_base(const float *q, int64_t nq, int dim, int m, const int32_t *lists, int nprobe, const float *cent, int nlist,
                          double *base, double *qq_or_null, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(nq < (1 << 20) ? nq : (1 << 20));
    if (qq_or_null)
        hipLaunchKernelGGL(k_pq_base<1>, dim3(grid), dim3(256), 0, st, q, nq, dim, m, lists, nprobe, cent, nlist, base, qq_or_null);
    else
        hipLaunchKernelGGL(k_pq_base<0>, dim3(grid), dim3(256), 0, st, q, nq, dim, m, lists, nprobe, cent, nlist, base, qq_or_null);
    return hipGetLastError();
}

hipError_t launch_pq_norms(const uint8_t *codes, int64_t n, int dim, int m, const int64_t *lists, const float *cent, int nlist,
                           const float *cb, double *n2, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t rounds = (n + 256 / m - 1) / (256 / m);
    const unsigned grid = (unsigned)(rounds < 65536 ? rounds : 65536);
    hipLaunchKernelGGL(k_pq_norms, dim3(grid), dim3(256), 0, st, codes, n, dim, m, lists, cent, nlist, cb, n2);
    return hipGetLastError();
}

hipError_t launch_pq_decode_residual(const uint8_t *codes, int64_t n, int dim, int m, const float *cb, const int64_t *lists,
                                     const float *cent, int nlist, float *dst, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
    hipLaunchKernelGGL(k_pq_decode_residual, dim3(grid), dim3(256), 0, st, codes, n, dim, m, cb, lists, cent, nlist, dst);
    return hipGetLastError();
}

}  // namespace mirx
