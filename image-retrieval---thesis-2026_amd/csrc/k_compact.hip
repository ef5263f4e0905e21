// k_compact.hip -- removing rows from a resident index (mirx_index_remove_ids): membership, an exclusive scan of the keep
// flags, and the order-preserving row moves.
//
//   mark     pos[r] = 1 when row r's id is absent from the sorted request (a binary search over its keys, id ^ sign bit in
//            ascending unsigned order, as the ranking's radix sort leaves them), else 0; one sum per tile of COMPACT_TILE
//            rows goes to part[tile]
//   partials one workgroup turns part[] into its exclusive scan and writes the total to pos[n]
//   apply    every tile scans its own flags again and adds part[tile]: pos[r] = survivors before row r, so row r survives iff
//            pos[r + 1] != pos[r] and then lands on row pos[r]
//   gather   the survivors of one source chunk [c0, c1) -> scratch row pos[r] - pos[c0]
//   place    scratch row j -> gallery row pos[c0] + j, for j < pos[c1] - pos[c0]
//
// The launch boundary is the only synchronisation between workgroups: no workgroup reads what another one of the same launch
// writes, nothing polls memory, and there is no atomic, so the result does not depend on scheduling.  gather and place are
// two launches per chunk because a chunk's destination [pos[c0], pos[c0] + count) may overlap its own source rows; it never
// reaches past c1 (pos[c0] <= c0 and count <= c1 - c0), so no later chunk's source is overwritten before it is read.
#include <algorithm>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_PER_THREAD = COMPACT_TILE / CP_THREADS;
static_assert(COMPACT_TILE % CP_THREADS == 0, "a tile is a whole number of rows per thread");

// exclusive scan of one value per thread over the workgroup (CP_THREADS threads = 4 waves); *total = the sum, in every thread
__device__ inline int block_exclusive_scan(int v, int *lds_wave, int *total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int o = __shfl_up(inc, off, WAVE);
        if (lane >= off) inc += o;
    }
    if (lane == WAVE - 1) lds_wave[wave] = inc;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < CP_THREADS / WAVE; ++w) {
        const int s = lds_wave[w];
        if (w < wave) before += s;
        sum += s;
    }
    __syncthreads();                                       // lds_wave is reused by the caller's next scan
    *total = sum;
    return before + inc - v;
}

__global__ __launch_bounds__(CP_THREADS) void compact_mark(const int64_t *__restrict__ ids, int64_t n,
                                                            const uint64_t *__restrict__ req, int64_t nreq,
                                                            int32_t *__restrict__ pos, int32_t *__restrict__ part) {
    __shared__ int lds_wave[CP_THREADS / WAVE];
    const int64_t base = (int64_t)blockIdx.x * COMPACT_TILE;
    int kept = 0;
#pragma unroll
    for (int i = 0; i < CP_PER_THREAD; ++i) {
        const int64_t r = base + i * CP_THREADS + threadIdx.x;         // coalesced over the tile
        if (r < n) {
            const uint64_t id = (uint64_t)ids[r] ^ 0x8000000000000000ull;
            int64_t lo = 0, hi = nreq;                                  // first request key >= the row's
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (req[mid] < id) lo = mid + 1; else hi = mid;
            }
            const int keep = !(lo < nreq && req[lo] == id);
            pos[r] = keep;
            kept += keep;
        }
    }
    kept = wave_isum(kept);
    if (lane_id() == 0) lds_wave[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < CP_THREADS / WAVE; ++w) s += lds_wave[w];
        part[blockIdx.x] = s;
    }
}

// one workgroup: part[0 .. ntiles) -> its exclusive scan, the total -> *total_out
__global__ __launch_bounds__(CP_THREADS) void compact_partials(int32_t *__restrict__ part, int64_t ntiles,
                                                                int32_t *__restrict__ total_out) {
    __shared__ int lds_wave[CP_THREADS / WAVE];
    int carry = 0;
    for (int64_t b = 0; b < ntiles; b += CP_THREADS) {
        const int64_t i = b + threadIdx.x;
        const int v = i < ntiles ? part[i] : 0;
        int sum;
        const int ex = block_exclusive_scan(v, lds_wave, &sum);
        if (i < ntiles) part[i] = carry + ex;
        carry += sum;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(CP_THREADS) void compact_apply(int32_t *__restrict__ pos, int64_t n,
                                                             const int32_t *__restrict__ part) {
    __shared__ int lds_wave[CP_THREADS / WAVE];
    // each thread owns CP_PER_THREAD consecutive rows, so the scan runs in row order
    const int64_t first = (int64_t)blockIdx.x * COMPACT_TILE + (int64_t)threadIdx.x * CP_PER_THREAD;
    int f[CP_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < CP_PER_THREAD; ++i) {
        f[i] = first + i < n ? pos[first + i] : 0;
        mine += f[i];
    }
    int sum;
    int at = part[blockIdx.x] + block_exclusive_scan(mine, lds_wave, &sum);
#pragma unroll
    for (int i = 0; i < CP_PER_THREAD; ++i) {
        if (first + i < n) pos[first + i] = at;
        at += f[i];
    }
}

// One source chunk [c0, c1), one wave per row: a row is dimp / 4 16-byte pieces of the fp32 master and dimp / 8 of the bf16
// copy, plus its id and bias.  MODE 0 (gather): surviving row r -> scratch row pos[r] - pos[c0].  MODE 1 (place): scratch row
// j < pos[c1] - pos[c0] -> gallery row pos[c0] + j.  A chunk in front of the first removed row (pos[c1] == c1) has nothing to
// move and both modes return.  s16 / sbias may be null (launch_compact_gather: a gather of the fp32 rows and ids alone).
template <int MODE>
__global__ __launch_bounds__(CP_THREADS) void compact_move(float *g32, uint16_t *g16, int64_t *ids, float *gbias, float *s32,
                                                            uint16_t *s16, int64_t *sid, float *sbias,
                                                            const int32_t *__restrict__ pos, int64_t c0, int64_t c1, int dimp) {
    const int64_t d0 = pos[c0], d1 = pos[c1];
    if (d1 == c1) return;
    const int lane = lane_id(), u32 = dimp >> 2, u16 = dimp >> 3;
    const int64_t rows = MODE == 0 ? c1 - c0 : d1 - d0;
    const int64_t nwaves = (int64_t)gridDim.x * (CP_THREADS / WAVE);
    for (int64_t j = (int64_t)blockIdx.x * (CP_THREADS / WAVE) + (threadIdx.x >> 6); j < rows; j += nwaves) {
        int64_t grow, srow;                                             // gallery row, scratch row (wave-uniform)
        if (MODE == 0) {
            grow = c0 + j;
            const int64_t p = pos[grow];
            if (pos[grow + 1] == p) continue;                           // removed
            srow = p - d0;
        } else {
            grow = d0 + j;
            srow = j;
        }
        uint4 *ga = reinterpret_cast<uint4 *>(g32 + grow * dimp), *sa = reinterpret_cast<uint4 *>(s32 + srow * dimp);
        if (MODE == 0) {
            for (int u = lane; u < u32; u += WAVE) sa[u] = ga[u];
            if (s16) {
                const uint4 *gb = reinterpret_cast<const uint4 *>(g16 + grow * dimp);
                uint4 *sb = reinterpret_cast<uint4 *>(s16 + srow * dimp);
                for (int u = lane; u < u16; u += WAVE) sb[u] = gb[u];
            }
            if (lane == 0) {
                sid[srow] = ids[grow];
                if (sbias) sbias[srow] = gbias[grow];
            }
        } else {
            uint4 *gb = reinterpret_cast<uint4 *>(g16 + grow * dimp);
            const uint4 *sb = reinterpret_cast<const uint4 *>(s16 + srow * dimp);
            for (int u = lane; u < u32; u += WAVE) ga[u] = sa[u];
            for (int u = lane; u < u16; u += WAVE) gb[u] = sb[u];
            if (lane == 0) {
                ids[grow] = sid[srow];
                gbias[grow] = sbias[srow];
            }
        }
    }
}

}  // namespace

int64_t compact_tiles(int64_t n) { return (n + COMPACT_TILE - 1) / COMPACT_TILE; }

size_t compact_scratch_bytes(int64_t chunk_rows, int dimp) {
    return (size_t)chunk_rows * ((size_t)dimp * (sizeof(float) + sizeof(uint16_t)) + sizeof(int64_t) + sizeof(float));
}

hipError_t launch_compact_scan(const int64_t *ids, int64_t n, const uint64_t *req, int64_t nreq, int32_t *pos, int32_t *part,
                               hipStream_t st) {
    const int64_t ntiles = compact_tiles(n);
    if (ntiles <= 0 || ntiles > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_mark, dim3((unsigned)ntiles), dim3(CP_THREADS), 0, st, ids, n, req, nreq, pos, part);
    return launch_compact_scan_flags(pos, n, part, st);
}

hipError_t launch_compact_scan_flags(int32_t *pos, int64_t n, int32_t *part, hipStream_t st) {
    const int64_t ntiles = compact_tiles(n);
    if (ntiles <= 0 || ntiles > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_partials, dim3(1), dim3(CP_THREADS), 0, st, part, ntiles, pos + n);
    hipLaunchKernelGGL(compact_apply, dim3((unsigned)ntiles), dim3(CP_THREADS), 0, st, pos, n, part);
    return hipGetLastError();
}

hipError_t launch_compact_gather(const float *g32, const int64_t *ids, const int32_t *pos, int64_t n, int dimp, float *s32,
                                 int64_t *sid, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    constexpr int WAVES = CP_THREADS / WAVE;
    const unsigned grid = (unsigned)std::min<int64_t>((n + WAVES - 1) / WAVES, 8 * (int64_t)current_device_cus());
    // the gather mode only reads the gallery
    hipLaunchKernelGGL(compact_move<0>, dim3(grid), dim3(CP_THREADS), 0, st, const_cast<float *>(g32), (uint16_t *)nullptr,
                       const_cast<int64_t *>(ids), (float *)nullptr, s32, (uint16_t *)nullptr, sid, (float *)nullptr, pos,
                       (int64_t)0, n, dimp);
    return hipGetLastError();
}

hipError_t launch_compact_chunk(float *g32, uint16_t *g16, int64_t *ids, float *gbias, void *scratch, int64_t chunk_rows,
                                const int32_t *pos, int64_t c0, int64_t c1, int dimp, hipStream_t st) {
    if (c1 <= c0 || c1 - c0 > chunk_rows) return hipErrorInvalidValue;
    float *s32 = reinterpret_cast<float *>(scratch);
    uint16_t *s16 = reinterpret_cast<uint16_t *>(s32 + chunk_rows * dimp);
    int64_t *sid = reinterpret_cast<int64_t *>(s16 + chunk_rows * dimp);
    float *sbias = reinterpret_cast<float *>(sid + chunk_rows);
    constexpr int WAVES = CP_THREADS / WAVE;                            // one row per wave and trip
    const unsigned grid = (unsigned)std::min<int64_t>((c1 - c0 + WAVES - 1) / WAVES, 8 * (int64_t)current_device_cus());
    hipLaunchKernelGGL(compact_move<0>, dim3(grid), dim3(CP_THREADS), 0, st, g32, g16, ids, gbias, s32, s16, sid, sbias, pos,
                       c0, c1, dimp);
    hipLaunchKernelGGL(compact_move<1>, dim3(grid), dim3(CP_THREADS), 0, st, g32, g16, ids, gbias, s32, s16, sid, sbias, pos,
                       c0, c1, dimp);
    return hipGetLastError();
}

}  // namespace mirx
