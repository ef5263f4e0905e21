// k_ranksort.hip -- the full ranking past the bitonic network's reach: a segmented, stable, least-significant-digit radix sort
// of 64-bit keys with an int32 row payload (gfx950, wave64).  One segment = one query's n gallery rows, n < 2^31.
//
// Order.  The key is rank_key(fp64 score) (mirx_common.h): ascending key = score descending.  The id half of hit_before comes
// from stability: the payload starts as the gallery rows in (id, row) order -- the identity when ids ascend with the row, else
// a permutation the index caches, made by this same sort with key = id ^ sign bit -- and eight stable passes keep that order
// among equal keys.  Rows with equal ids keep row order.  A NaN score sorts outside the numbers (before +inf or after -inf).
//
// One digit pass = three launches; launch boundaries are the only synchronisation between workgroups:
//   k_rs_hist     grid (tiles, segments): digit counts of one RANK_TILE-element tile -> hist[segment][digit][tile]
//   k_rs_scan     grid (segments): exclusive scan of a segment's hist in that (digit-major) order = where in the segment the
//                 elements of (digit, tile) go
//   k_rs_scatter  grid (tiles, segments): ranks the tile's elements within their digit (__ballot multi-split per 64-element
//                 row, per-wave counters in LDS), orders the tile by digit in LDS, writes runs of equal digits
// Eight 8-bit passes over two key and two payload buffers end in the buffers they started from.
//
// Reference behaviour replaced: torch.argsort(dists, dim=0, descending=True) (test.py:1090,179) and the top_k = num_entities
// search of query_nih_zilliz.py:53-63, for galleries of more than 65536 rows (below that: k_exact.hip's bitonic network).
#include "mirx_device.h"
#include "mirx_kernels.h"

#include <math.h>

#include <algorithm>
#include <utility>

namespace mirx {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / WAVE;
constexpr int RS_ROWS = RANK_TILE / RS_THREADS;          // 64-element rows per wave, = elements per thread
constexpr int RS_BITS = 8;
constexpr int RS_BINS = 1 << RS_BITS;
static_assert(RS_BINS == RS_THREADS, "one thread per digit in the tile's digit scan");
static_assert(RANK_TILE == RS_WAVES * RS_ROWS * WAVE, "a tile is RS_WAVES chunks of RS_ROWS rows of 64 elements");

__device__ inline unsigned digit_of(uint64_t key, int shift) { return (unsigned)(key >> shift) & (RS_BINS - 1); }

// inclusive sum over the lanes at or below this one
__device__ inline unsigned wave_inclusive_sum(unsigned v, int lane) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)v, off, WAVE);
        if (lane >= off) v += o;
    }
    return v;
}

// exclusive sum of `v` over the workgroup's 256 threads in thread order (wsum: RS_WAVES LDS words); ends with a barrier, so
// wsum may be used again at once.  *total = the sum over all threads.
__device__ inline unsigned block_exclusive_sum(unsigned v, unsigned *wsum, unsigned *total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const unsigned inc = wave_inclusive_sum(v, lane);
    if (lane == WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) {
        const unsigned s = wsum[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// ---- keys and payload of a batch of queries ---------------------------------------------------------------------------------
// Position j of segment qi holds gallery row r = perm ? perm[j] : j with the key of its score.  The excluded id gets the key of
// -inf (rank_all: it ties with genuine -inf rows by id, as in the bitonic path) or, with drop_excluded, the key after every
// score's (rank_top leaves it out: it must end behind every eligible row).
__global__ __launch_bounds__(256) void k_rs_build(const double *__restrict__ scores, int64_t ld, int64_t n,
                                                  const int64_t *__restrict__ ids, const int32_t *__restrict__ perm,
                                                  const int64_t *__restrict__ exclude, int drop_excluded,
                                                  uint64_t *__restrict__ keys, int32_t *__restrict__ pay) {
    const int64_t qi = blockIdx.y;
    const bool has_ex = exclude != nullptr;
    const int64_t ex = has_ex ? exclude[qi] : 0;
    const uint64_t ex_key = drop_excluded ? RANK_KEY_LAST : rank_key(-INFINITY);
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        int32_t r = perm ? perm[j] : (int32_t)j;
        if ((uint32_t)r >= (uint64_t)n) r = (int32_t)j;            // never for a permutation: keeps a bug in bounds
        keys[qi * n + j] = (has_ex && ids[r] == ex) ? ex_key : rank_key(scores[qi * ld + r]);
        pay[qi * n + j] = r;
    }
}

// One segment whose ascending order is (id, row): key = id with the sign bit flipped, payload = row.
__global__ __launch_bounds__(256) void k_rs_build_ids(const int64_t *__restrict__ ids, int64_t n, uint64_t *__restrict__ keys,
                                                      int32_t *__restrict__ pay) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        keys[j] = (uint64_t)ids[j] ^ 0x8000000000000000ull;
        pay[j] = (int32_t)j;
    }
}

// ---- pass, launch 1: the tile's digit counts --------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void k_rs_hist(const uint64_t *__restrict__ keys, int64_t n, int shift,
                                                        unsigned *__restrict__ hist, int ntiles) {
    __shared__ unsigned h[RS_BINS];
    const int64_t seg = blockIdx.y;
    const int tile = blockIdx.x;
    const int64_t t0 = (int64_t)tile * RANK_TILE;
    const int tile_n = (int)((n - t0) < RANK_TILE ? (n - t0) : RANK_TILE);
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t *src = keys + seg * n + t0;
    for (int i = threadIdx.x; i < tile_n; i += RS_THREADS) {
        const unsigned d = digit_of(src[i], shift);
        // a wave whose 64 elements share the digit (the leading digits of scores mostly do) adds once, not 64 times to one word
        const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
        const unsigned long long active = __ballot(1);
        if (__ballot(d == d0) == active) {
            if (lane_id() == __ffsll((long long)active) - 1) atomicAdd(&h[d0], (unsigned)__popcll(active));
        } else {
            atomicAdd(&h[d], 1u);
        }
    }
    __syncthreads();
    hist[(seg * RS_BINS + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// ---- pass, launch 2: exclusive scan of one segment's len = RS_BINS * ntiles counts, in place --------------------------------
__global__ __launch_bounds__(RS_THREADS) void k_rs_scan(unsigned *__restrict__ hist, int64_t len) {
    __shared__ unsigned wsum[RS_WAVES];
    u32x4 *seg = reinterpret_cast<u32x4 *>(hist + (int64_t)blockIdx.x * len);       // len % 4 == 0, 16-byte aligned
    const int64_t nvec = len >> 2;
    unsigned running = 0;
    for (int64_t base = 0; base < nvec; base += RS_THREADS) {
        const int64_t i = base + threadIdx.x;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (i < nvec) v = seg[i];
        unsigned total;
        const unsigned ex = running + block_exclusive_sum(v[0] + v[1] + v[2] + v[3], wsum, &total);
        if (i < nvec) {
            const u32x4 o = {ex, ex + v[0], ex + v[0] + v[1], ex + v[0] + v[1] + v[2]};
            seg[i] = o;
        }
        running += total;
    }
}

// ---- pass, launch 3: the stable scatter of one tile -------------------------------------------------------------------------
// Element e of the tile belongs to wave e / (RS_ROWS * 64), row (e / 64) % RS_ROWS, lane e % 64: tile order = wave, row, lane.
// Its place among the tile's elements of the same digit d is
//     (elements of d in earlier waves) + (elements of d in this wave's earlier rows) + (lanes below it with d in its row),
// the last from eight ballots, the middle from a per-wave counter row in LDS that the group's lowest lane advances after every
// lane has read it (a wave's LDS accesses execute in program order; the counters are volatile so the compiler keeps that order).
// The tile is then laid out by digit in LDS and leaves as runs of equal digits: element i of that layout, digit d, goes to
// scanned hist[d][tile] + (i - first element of d in the layout).
__global__ __launch_bounds__(RS_THREADS) void k_rs_scatter(const uint64_t *__restrict__ keys_in, const int32_t *__restrict__ pay_in,
                                                           uint64_t *__restrict__ keys_out, int32_t *__restrict__ pay_out,
                                                           int64_t n, int shift, const unsigned *__restrict__ hist, int ntiles) {
    __shared__ uint64_t skey[RANK_TILE];
    __shared__ int32_t spay[RANK_TILE];
    __shared__ unsigned wcnt[RS_WAVES][RS_BINS];
    __shared__ unsigned gofs[RS_BINS];          // segment position of element i of digit d = gofs[d] + i  (mod 2^32)
    __shared__ unsigned wsum[RS_WAVES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t seg = blockIdx.y;
    const int tile = blockIdx.x;
    const int64_t t0 = (int64_t)tile * RANK_TILE;
    const int tile_n = (int)((n - t0) < RANK_TILE ? (n - t0) : RANK_TILE);
    const uint64_t *kin = keys_in + seg * n + t0;
    const int32_t *pin = pay_in + seg * n + t0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();

    uint64_t key[RS_ROWS];
    int32_t pay[RS_ROWS];
    unsigned off[RS_ROWS];
    volatile unsigned *mycnt = wcnt[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
        const int e = (wave * RS_ROWS + r) * WAVE + lane;
        const bool valid = e < tile_n;
        key[r] = valid ? kin[e] : 0ull;
        pay[r] = valid ? pin[e] : 0;
        const unsigned d = digit_of(key[r], shift);
        unsigned long long same = __ballot(valid);                  // lanes of this row with my digit
#pragma unroll
        for (int b = 0; b < RS_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const unsigned lower = (unsigned)__popcll(same & below);
        const unsigned prior = mycnt[d];
        off[r] = prior + lower;
        if (valid && lower == 0) mycnt[d] = prior + (unsigned)__popcll(same);
    }
    __syncthreads();

    {   // thread t = digit t: the tile's counts are scanned over the digits (first = where digit t starts in the tile's layout),
        // and wave w's count becomes where ITS elements of digit t start: first + the counts of the waves before it
        const int t = threadIdx.x;
        unsigned c[RS_WAVES], sum = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) {
            c[w] = wcnt[w][t];
            sum += c[w];
        }
        unsigned total;
        const unsigned first = block_exclusive_sum(sum, wsum, &total);
        unsigned at = first;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) {
            wcnt[w][t] = at;
            at += c[w];
        }
        gofs[t] = hist[(seg * RS_BINS + t) * ntiles + tile] - first;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
        const int e = (wave * RS_ROWS + r) * WAVE + lane;
        if (e < tile_n) {
            const unsigned d = digit_of(key[r], shift);
            const unsigned pos = wcnt[wave][d] + off[r];
            if (pos < (unsigned)RANK_TILE) { skey[pos] = key[r]; spay[pos] = pay[r]; }
        }
    }
    __syncthreads();

    uint64_t *kout = keys_out + seg * n;
    int32_t *pout = pay_out + seg * n;
    for (int i = threadIdx.x; i < tile_n; i += RS_THREADS) {
        const uint64_t k = skey[i];
        const unsigned dst = gofs[digit_of(k, shift)] + (unsigned)i;
        if ((int64_t)dst < n) { kout[dst] = k; pout[dst] = spay[i]; }   // always true for a consistent hist: keeps a bug in bounds
    }
}

// ---- the first kout ranks of every segment -> ids / reported values / fp64 scores ----------------------------------------
// drop_excluded (rank_top): a slot that holds the excluded id reads (-1, -inf) -- those rows carry RANK_KEY_LAST, so they are the
// segment's last and every eligible row has moved up past them.
__global__ __launch_bounds__(256) void k_rs_write(const int32_t *__restrict__ pay, int64_t n, int64_t kout,
                                                  const double *__restrict__ scores, int64_t ld, const int64_t *__restrict__ ids,
                                                  const int64_t *__restrict__ exclude, int drop_excluded, int metric,
                                                  int64_t *__restrict__ out_ids, float *__restrict__ out_val,
                                                  double *__restrict__ out_f64) {
    const int64_t qi = blockIdx.y;
    const bool has_ex = exclude != nullptr;
    const int64_t ex = has_ex ? exclude[qi] : 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < kout; j += (int64_t)gridDim.x * 256) {
        const int32_t r = pay[qi * n + j];
        const bool in_range = (uint32_t)r < (uint64_t)n;            // always, for a sorted payload: keeps a bug in bounds
        int64_t id = in_range ? ids[r] : -1;
        const bool excluded = !in_range || (has_ex && id == ex);
        const double s = excluded ? -INFINITY : scores[qi * ld + r];
        if (!in_range || (excluded && drop_excluded)) id = -1;
        out_ids[qi * kout + j] = id;
        if (out_val) out_val[qi * kout + j] = reported_value(s, metric);
        if (out_f64) out_f64[qi * kout + j] = s;
    }
}

unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 4096); }

}  // namespace

int64_t rank_sort_tiles(int64_t n) { return (n + RANK_TILE - 1) / RANK_TILE; }

// Sorts nseg segments of n (key, payload) pairs ascending by key, stably: in and out in keys_a / pay_a, keys_b / pay_b of the
// same size are scratch, hist = nseg * 256 * rank_sort_tiles(n) words.  key_bits (a multiple of 16): the low bits that can differ
// between keys -- the digits above them are not sorted on.
hipError_t launch_rank_sort(uint64_t *keys_a, int32_t *pay_a, uint64_t *keys_b, int32_t *pay_b, unsigned *hist, int64_t n,
                            int nseg, hipStream_t st, int key_bits) {
    if (nseg <= 0 || n <= 0) return hipSuccess;
    if (key_bits < 2 * RS_BITS || key_bits > 64 || key_bits % (2 * RS_BITS)) return hipErrorInvalidValue;
    const int ntiles = (int)rank_sort_tiles(n);
    const dim3 grid((unsigned)ntiles, (unsigned)nseg);
    for (int pass = 0; pass < key_bits / RS_BITS; ++pass) {
        const int shift = pass * RS_BITS;
        hipLaunchKernelGGL(k_rs_hist, grid, dim3(RS_THREADS), 0, st, keys_a, n, shift, hist, ntiles);
        hipLaunchKernelGGL(k_rs_scan, dim3((unsigned)nseg), dim3(RS_THREADS), 0, st, hist, (int64_t)RS_BINS * ntiles);
        hipLaunchKernelGGL(k_rs_scatter, grid, dim3(RS_THREADS), 0, st, keys_a, pay_a, keys_b, pay_b, n, shift, hist, ntiles);
        std::swap(keys_a, keys_b);
        std::swap(pay_a, pay_b);
    }
    // key_bits % (2 * RS_BITS) == 0: an even number of passes ends in the buffers it started from
    return hipGetLastError();
}

hipError_t launch_rank_sort_build(const double *scores, int64_t ld, int64_t n, const int64_t *ids, const int32_t *perm,
                                  const int64_t *exclude, int drop_excluded, int nq, uint64_t *keys, int32_t *pay, hipStream_t st) {
    if (nq <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rs_build, dim3(grid_for(n), (unsigned)nq), dim3(256), 0, st, scores, ld, n, ids, perm, exclude,
                       drop_excluded, keys, pay);
    return hipGetLastError();
}

hipError_t launch_rank_sort_build_ids(const int64_t *ids, int64_t n, uint64_t *keys, int32_t *pay, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rs_build_ids, dim3(grid_for(n)), dim3(256), 0, st, ids, n, keys, pay);
    return hipGetLastError();
}

hipError_t launch_rank_sort_write(const int32_t *pay, int64_t n, int64_t kout, const double *scores, int64_t ld,
                                  const int64_t *ids, const int64_t *exclude, int drop_excluded, int metric, int nq,
                                  int64_t *out_ids, float *out_val, double *out_f64, hipStream_t st) {
    if (nq <= 0 || kout <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rs_write, dim3(grid_for(kout), (unsigned)nq), dim3(256), 0, st, pay, n, kout, scores, ld, ids, exclude,
                       drop_excluded, metric, out_ids, out_val, out_f64);
    return hipGetLastError();
}

}  // namespace mirx
