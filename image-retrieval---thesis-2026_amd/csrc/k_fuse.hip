// k_fuse.hip -- hybrid search: fuses the ranked lists of up to 8 search requests into one ranking per query.
//
//   k_fuse_ranked  one workgroup per query over the concatenated lists [m = sum limit_r] of document codes (-1 = empty slot) and
//                  fp32 distances.  (1) a bitonic sort of the keys (code, position) in LDS brings the entries of one document
//                  together, in ascending request order since the lists are concatenated in that order; (2) the first entry of
//                  each run adds the run's contributions front to back -- one thread, one fixed order, separate multiply and add
//                  (the library is built with -ffp-contract=off), so the fp64 score has the bits of the host restatement; (3) a
//                  second bitonic sort orders the documents by (score descending, code ascending); (4) the first `limit` go out.
//                  No atomics, and no index is ever derived from a code: positions come from the thread index alone.
// LDS: 16 bytes per slot of the sort width (8-byte keys first, then the 16-byte records in the same memory): 64 KiB at m = 4096.
#include <climits>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int FUSE_ITEMS = 4;                    // slots of the sort width per thread (the launcher sizes the workgroup for it)
constexpr unsigned long long FUSE_PAD = ~0ull;   // key of a slot without an entry: behind every entry
constexpr int FUSE_NO_CODE = INT_MAX;            // code of a record without a document: behind every document

struct FuseRec {
    double s;        // fused score
    int code;        // document code, FUSE_NO_CODE = none
    int first;       // position in the concatenated lists of the document's first entry
};

__device__ inline bool fuse_before(const FuseRec &x, const FuseRec &y) {
    const bool xn = x.code == FUSE_NO_CODE, yn = y.code == FUSE_NO_CODE;
    if (xn != yn) return yn;
    if (x.s != y.s) return x.s > y.s;
    return x.code < y.code;
}

// request of position j of the concatenated lists
__device__ inline int fuse_request(const FuseArgs &a, int j) {
    int r = 0;
    while (r + 1 < a.n_requests && j >= a.offsets[r + 1]) ++r;
    return r;
}

// contribution of the entry at position j of query row `dist`
__device__ inline double fuse_term(const FuseArgs &a, const float *dist, int j) {
#pragma clang fp contract(off)
    const int r = fuse_request(a, j);
    if (a.ranker == MIRX_FUSE_RRF) {
        const double rank = (double)(j - a.offsets[r] + 1);
        return 1.0 / (a.rrf_k + rank);
    }
    const double d = (double)dist[j];
    double n = d;
    switch (a.norms[r]) {
        case MIRX_FUSE_NORM_COSINE: n = (1.0 + d) * 0.5; break;
        case MIRX_FUSE_NORM_IP: n = 0.5 + atan(d) / M_PI; break;
        case MIRX_FUSE_NORM_L2: n = 1.0 - 2.0 * atan(d) / M_PI; break;
        default: break;
    }
    return a.weights[r] * n;
}

__global__ __launch_bounds__(1024) void k_fuse_ranked(FuseArgs a, int mp) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned long long fuse_lds[];
    unsigned long long *keys = fuse_lds;                     // [mp], phases 1 and 2
    FuseRec *rec = reinterpret_cast<FuseRec *>(fuse_lds);    // [mp], phases 3 and 4, over the keys
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t *codes = a.codes + q * a.row_stride;
    const float *dist = a.distances + q * a.row_stride;

    for (int i = tid; i < mp; i += nt) {
        unsigned long long key = FUSE_PAD;
        if (i < a.m) {
            const int64_t c = codes[i];
            if (c >= 0 && c < a.n_codes) key = ((unsigned long long)c << 32) | (unsigned)i;
        }
        keys[i] = key;
    }
    bitonic_lds(keys, mp, [](unsigned long long x, unsigned long long y) { return x < y; });

    // the first entry of each run of one code adds the run, front to back: ascending position = ascending request
    FuseRec mine[FUSE_ITEMS];
#pragma unroll
    for (int t = 0; t < FUSE_ITEMS; ++t) {
        const int i = tid + t * nt;
        mine[t] = FuseRec{-INFINITY, FUSE_NO_CODE, -1};
        if (i >= mp) continue;
        const unsigned long long k = keys[i];
        if (k == FUSE_PAD) continue;
        const unsigned code = (unsigned)(k >> 32);
        if (i > 0 && (unsigned)(keys[i - 1] >> 32) == code) continue;
        double s = 0.0;
        for (int e = i; e < mp; ++e) {
            const unsigned long long ke = keys[e];
            if ((unsigned)(ke >> 32) != code) break;         // (a slot without an entry carries no code)
            s = s + fuse_term(a, dist, (int)(unsigned)ke);    // the low word is a position < m by construction
        }
        mine[t] = FuseRec{s, (int)code, (int)(unsigned)k};
    }
    __syncthreads();                                         // every key is read before the records take their place
#pragma unroll
    for (int t = 0; t < FUSE_ITEMS; ++t) {
        const int i = tid + t * nt;
        if (i < mp) rec[i] = mine[t];
    }
    bitonic_lds(rec, mp, [](const FuseRec &x, const FuseRec &y) { return fuse_before(x, y); });

    const int64_t ob = q * a.limit;
    for (int p = tid; p < a.limit; p += nt) {
        const bool have = p < mp && rec[p].code != FUSE_NO_CODE;
        int r = -1, slot = -1;
        if (have) {
            r = fuse_request(a, rec[p].first);
            slot = rec[p].first - a.offsets[r];
        }
        a.out_codes[ob + p] = have ? (int64_t)rec[p].code : -1;
        a.out_scores[ob + p] = have ? rec[p].s : -INFINITY;
        a.out_request[ob + p] = r;
        a.out_slot[ob + p] = slot;
    }
    // the documents stand in front of the empty records: the last of them knows the count
    for (int p = tid; p < mp; p += nt) {
        const bool have = rec[p].code != FUSE_NO_CODE;
        if (p == 0 && !have) a.out_count[q] = 0;
        if (have && (p + 1 == mp || rec[p + 1].code == FUSE_NO_CODE)) a.out_count[q] = p + 1 < a.limit ? p + 1 : a.limit;
    }
}

}  // namespace

int fuse_sort_width(int m) {
    int p = 1;
    while (p < m) p <<= 1;
    return p;
}

hipError_t launch_fuse_ranked(const FuseArgs &a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const int mp = fuse_sort_width(a.m);
    // FUSE_ITEMS slots per thread, whole wavefronts, at most 1024 threads (m <= 4096)
    int threads = (mp + FUSE_ITEMS - 1) / FUSE_ITEMS;
    threads = threads < 64 ? 64 : (threads + 63) / 64 * 64;
    if (threads > 1024 || mp > threads * FUSE_ITEMS) return hipErrorInvalidValue;
    const size_t lds = (size_t)mp * sizeof(FuseRec);
    hipLaunchKernelGGL(k_fuse_ranked, dim3((unsigned)a.nq), dim3(threads), lds, st, a, mp);
    return hipGetLastError();
}

}  // namespace mirx
