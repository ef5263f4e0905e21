// k_ivf_pq.hip -- the kernels of IVF_PQ (mirx_ivf.hip, include/mirx.h): a query's asymmetric-distance tables, the scan of the
// probed lists' code rows against them, and the small moves around the code master (codes packed from the codeword search,
// codes decoded to their codewords).  The lists, probes, compact score rows and their top-k are k_ivf.hip's, unchanged.
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
template <int METRIC, bool V16>
__global__ __launch_bounds__(PQ_ITEM_ROWS) void k_pq_scan(const double *__restrict__ tables, const uint8_t *__restrict__ codes, int m,
                                                           const int32_t *__restrict__ probes, const int32_t *__restrict__ qoff,
                                                           int nq, int nprobe, const int64_t *__restrict__ offsets,
                                                           const int32_t *__restrict__ itemoff, double *__restrict__ out,
                                                           int64_t ld) {
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
        double s = 0.0;
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

template <int METRIC, bool V16>
hipError_t launch_pq_scan_t(const PqScanArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.m * 256 * sizeof(double);
    static std::atomic<unsigned long long> once{0};
    hipError_t e = set_dynamic_lds(k_pq_scan<METRIC, V16>, (size_t)PQ_MAX_M * 256 * sizeof(double), &once);
    if (e != hipSuccess) return e;
    const int per_cu = lds * 2 <= PQ_CU_LDS_BYTES ? 2 : 1;                         // 1024 threads each: two workgroups fill a CU
    const unsigned grid = (unsigned)(current_device_cus() * per_cu);
    hipLaunchKernelGGL((k_pq_scan<METRIC, V16>), dim3(grid), dim3(PQ_ITEM_ROWS), lds, st, a.tables, a.codes, a.m, a.probes, a.qoff,
                       a.nq, a.nprobe, a.offsets, a.itemoff, a.out, a.ld);
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
    if (a.m % 16 == 0) return metric == MIRX_METRIC_IP ? launch_pq_scan_t<0, true>(a, st) : launch_pq_scan_t<1, true>(a, st);
    return metric == MIRX_METRIC_IP ? launch_pq_scan_t<0, false>(a, st) : launch_pq_scan_t<1, false>(a, st);
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

}  // namespace mirx
