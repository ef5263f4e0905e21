// k_mask.hip -- searching under a row mask (mirx_index_search_masked / mirx_index_rank_top_masked): the one pass over the
// caller's allow bytes, and the small passes that keep masked rows out of the exact scan and of the radix ranking.
//
//   pass     per row r < cap: the search's bias vector (what the unmasked filter GEMM would add -- gbias[r], or 0 without one --
//            for an allowed row and for the zero rows past `size`; -inf for a masked row), and per row r < size the keep flag
//            pos[r] = 0 / 1, the masked id (the row's id, or INT64_MAX = "no row") and one sum per COMPACT_TILE rows in
//            part[tile].  k_compact.hip's scan turns the flags into positions and the total (launch_compact_scan_flags).
//   scores   fp64 score tile [cnt, ld]: the entries of masked rows become -inf.  Together with the masked ids such an entry is
//            (-inf, INT64_MAX), which k_row_topk never takes: it is not before the empty slot it would replace.
//   keys     radix ranking: the key of a masked row becomes RANK_KEY_LAST, behind every score's (as the dropped excluded id)
//   tail     radix ranking: an output slot whose row is masked reads (-1, -inf)
// scores reads the scanned positions, which its caller needs anyway for the gather; keys and tail, shared by rank_top under a
// mask and the range search's exact route, read the allow bytes themselves: a row is masked iff its byte is zero.
//
// Why -inf and not a large negative number: the filter tests `score + bias > tau` with a strict >, so -inf passes no threshold,
// not even tau = -inf.  A sum can only be NaN where the bf16 dot product itself is +inf or NaN, and NaN > tau is false as well;
// fmaxf drops a NaN operand, so a group maximum never is one.
//
// Every kernel writes each word from exactly one thread, there is no atomic and no workgroup reads another's output of the
// same launch: the result does not depend on scheduling.
#include <algorithm>

#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

namespace mirx {

namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_PER_THREAD = COMPACT_TILE / MK_THREADS;
static_assert(COMPACT_TILE % MK_THREADS == 0, "a tile is a whole number of rows per thread");

// a masked row in the scanned positions: nothing is kept between pos[r] and pos[r + 1]
__device__ inline bool row_masked(const int32_t *__restrict__ pos, int64_t r) { return pos[r + 1] == pos[r]; }

__global__ __launch_bounds__(MK_THREADS) void mask_pass(const uint8_t *__restrict__ allow, int64_t n, int64_t cap,
                                                         const float *__restrict__ gbias, const int64_t *__restrict__ ids,
                                                         float *__restrict__ bias, int64_t *__restrict__ mids,
                                                         int32_t *__restrict__ pos, int32_t *__restrict__ part, int64_t ntiles) {
    __shared__ int lds_wave[MK_THREADS / WAVE];
    const int64_t base = (int64_t)blockIdx.x * COMPACT_TILE;
    int kept = 0;
#pragma unroll
    for (int i = 0; i < MK_PER_THREAD; ++i) {
        const int64_t r = base + i * MK_THREADS + threadIdx.x;             // coalesced over the tile
        if (r < cap) {
            const bool live = r < n;
            const bool ok = live && allow[r] != 0;
            const float b = gbias ? gbias[r] : 0.0f;
            bias[r] = (live && !ok) ? -INFINITY : b;
            if (live) {
                pos[r] = ok ? 1 : 0;
                mids[r] = ok ? ids[r] : INT64_MAX;
                kept += ok ? 1 : 0;
            }
        }
    }
    kept = wave_isum(kept);
    if (lane_id() == 0) lds_wave[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < ntiles) {                         // tiles wholly past `size` have no part[] entry
        int s = 0;
        for (int w = 0; w < MK_THREADS / WAVE; ++w) s += lds_wave[w];
        part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void mask_scores(double *__restrict__ scores, int64_t ld, int64_t n,
                                                   const int32_t *__restrict__ pos) {
    const int64_t qi = blockIdx.y;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        if (row_masked(pos, r)) scores[qi * ld + r] = -INFINITY;
}

// leave-group-out: the entries of the rows that carry the query's code become NaN (see launch_leave_out_scores)
__global__ __launch_bounds__(256) void leave_out_scores(double *__restrict__ scores, int64_t ld, int64_t n,
                                                        const int32_t *__restrict__ row_codes,
                                                        const int32_t *__restrict__ query_codes,
                                                        const int32_t *__restrict__ qlist) {
    const int64_t pos = blockIdx.y;
    const int32_t qc = query_codes[qlist ? (int64_t)qlist[pos] : pos];
    if (qc < 0) return;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        if (row_codes[r] == qc) scores[pos * ld + r] = __longlong_as_double(0x7FF8000000000000ll);
}

__global__ __launch_bounds__(256) void mask_gather_codes(const int32_t *__restrict__ row_codes, const int32_t *__restrict__ pos,
                                                         int64_t n, int32_t *__restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        if (!row_masked(pos, r)) out[pos[r]] = row_codes[r];
}

__global__ __launch_bounds__(256) void mask_rank_keys(uint64_t *__restrict__ keys, const int32_t *__restrict__ pay, int64_t n,
                                                      const uint8_t *__restrict__ allow) {
    const int64_t qi = blockIdx.y;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int32_t r = pay[qi * n + j];
        if ((uint32_t)r < (uint64_t)n && allow[r] == 0) keys[qi * n + j] = RANK_KEY_LAST;
    }
}

__global__ __launch_bounds__(256) void mask_rank_tail(const int32_t *__restrict__ pay, int64_t n, int64_t kout,
                                                      const uint8_t *__restrict__ allow, int64_t *__restrict__ out_ids,
                                                      float *__restrict__ out_val, double *__restrict__ out_f64) {
    const int64_t qi = blockIdx.y;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < kout; j += (int64_t)gridDim.x * 256) {
        const int32_t r = pay[qi * n + j];
        if ((uint32_t)r < (uint64_t)n && allow[r] == 0) {
            out_ids[qi * kout + j] = -1;
            if (out_val) out_val[qi * kout + j] = -INFINITY;
            if (out_f64) out_f64[qi * kout + j] = -INFINITY;
        }
    }
}

unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 4096); }

}  // namespace

hipError_t launch_mask_pass(const uint8_t *allow, int64_t n, int64_t cap, const float *gbias, const int64_t *ids, float *bias,
                            int64_t *mids, int32_t *pos, int32_t *part, hipStream_t st) {
    if (n <= 0 || cap < n) return hipErrorInvalidValue;
    const int64_t tiles = (cap + COMPACT_TILE - 1) / COMPACT_TILE;
    if (tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_pass, dim3((unsigned)tiles), dim3(MK_THREADS), 0, st, allow, n, cap, gbias, ids, bias, mids, pos, part,
                       compact_tiles(n));
    return hipGetLastError();
}

hipError_t launch_mask_scores(double *scores, int64_t ld, int64_t n, const int32_t *pos, int nq, hipStream_t st) {
    if (nq <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_scores, dim3(grid_for(n), (unsigned)nq), dim3(256), 0, st, scores, ld, n, pos);
    return hipGetLastError();
}

hipError_t launch_leave_out_scores(double *scores, int64_t ld, int64_t n, const int32_t *row_codes, const int32_t *query_codes,
                                   const int32_t *qlist, int nq, hipStream_t st) {
    if (nq <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(leave_out_scores, dim3(grid_for(n), (unsigned)nq), dim3(256), 0, st, scores, ld, n, row_codes, query_codes,
                       qlist);
    return hipGetLastError();
}

hipError_t launch_mask_gather_codes(const int32_t *row_codes, const int32_t *pos, int64_t n, int32_t *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_gather_codes, dim3(grid_for(n)), dim3(256), 0, st, row_codes, pos, n, out);
    return hipGetLastError();
}

hipError_t launch_mask_rank_keys(uint64_t *keys, const int32_t *pay, int64_t n, const uint8_t *allow, int nq, hipStream_t st) {
    if (nq <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_rank_keys, dim3(grid_for(n), (unsigned)nq), dim3(256), 0, st, keys, pay, n, allow);
    return hipGetLastError();
}

hipError_t launch_mask_rank_tail(const int32_t *pay, int64_t n, int64_t kout, const uint8_t *allow, int nq, int64_t *out_ids,
                                 float *out_val, double *out_f64, hipStream_t st) {
    if (nq <= 0 || kout <= 0) return hipSuccess;
    hipLaunchKernelGGL(mask_rank_tail, dim3(grid_for(kout), (unsigned)nq), dim3(256), 0, st, pay, n, kout, allow, out_ids, out_val,
                       out_f64);
    return hipGetLastError();
}

}  // namespace mirx
