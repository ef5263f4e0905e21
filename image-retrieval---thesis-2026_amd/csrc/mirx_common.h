// mirx_common.h -- shared host helpers for libmirx (gfx950 only); the device helpers live in mirx_device.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>

#include "../../include/mirx.h"

// ---- diagnostic builds ----------------------------------------------------------------------------------------------
// A few kernels carry arms that give WRONG RESULTS on purpose (a phase skipped, raw bits stored instead of values, operands
// never refreshed) or add cycle stamps / printf, to attribute a kernel's time.  The macros below select them, and they are
// honoured only together with -DMIRX_DIAG: the shipped library never defines it (csrc/Makefile refuses a CXXFLAGS that
// carries any -DMIRX_ switch; the diag-* targets build such objects into exp/ under other names).
#if !defined(MIRX_DIAG) &&                                                                                             \
    (defined(MIRX_EXP_NODMA) || defined(MIRX_EXP_NOBAR) || defined(MIRX_EXP_NOEPI) || defined(MIRX_EXP_NOLDS) ||         \
     defined(MIRX_EXP_SLOTS) || defined(MIRX_EXP_SAMEA) || defined(MIRX_EXP_NOA) || defined(MIRX_EXP_NOB) ||             \
     defined(MIRX_EXP_CYCLES) || defined(MIRX_C1H2_EXP_SKIP) || defined(MIRX_C1H2_EXP_SPLIT) ||                          \
     defined(MIRX_C1H2_EXP_ONE_MFMA) || defined(MIRX_C1H2_STAMPS) || defined(MIRX_LT2_EXP) || defined(MIRX_LH2_EXP) ||   \
     defined(MIRX_DF_EXP) || defined(MIRX_DF_STAMPS) || defined(MIRX_DW_STAMPS) || defined(MIRX_STEM_EXP) ||             \
     defined(MIRX_W3_CYCLES) || defined(MIRX_D2P_WAVES) || defined(MIRX_STEM_PLAIN_ORDER) || defined(MIRX_ATT_EXP))
#error "a MIRX diagnostic switch without -DMIRX_DIAG: these arms give wrong results or alter timing and must never reach libmirx.so"
#endif

namespace mirx {

// ---- error plumbing -------------------------------------------------------------------
void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

#define MIRX_HIP(expr)                                                                     \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess)                                                             \
            return ::mirx::fail(MIRX_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

#define MIRX_CHECK(cond, msg)                                   \
    do {                                                        \
        if (!(cond)) return ::mirx::fail(MIRX_EINVAL, (msg));   \
    } while (0)

// ---- what the stateful objects (mirx_index.hip, mirx_ivf.hip) share on the host --------
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }                          // on the device that is current: the owner's destroy call selects its device
    hipError_t ensure(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            bytes = 0;
            if (e != hipSuccess) return e;
        }
        size_t want = need + need / 4;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            e = hipMalloc(&p, need);
            want = need;
        }
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline bool is_device_pointer(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();   // unregistered host memory reports an error: treat as host
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// ---- sizes ----------------------------------------------------------------------------
constexpr int WAVE = 64;
constexpr int DIM_ALIGN = 128;       // rows are stored padded to a multiple of 128 elements (2 GEMM K-steps)
constexpr int ROW_ALIGN = 256;       // gallery capacity is a multiple of the GEMM M tile
constexpr int CAND_CAP = 1024;       // per-query candidate capacity of the threshold filter
constexpr int CAND_OVF = 256;        // per-query shared overflow list (global atomics, rare)
constexpr int MAX_K = 1024;
// The deep route (mirx_index_search_deep): the filter sequence for k_eff past TIER1_MAX_K, with its own capacities.
constexpr int DEEP_CAP = 4096;          // per-query candidate capacity of k_finalize on the deep route (regions and overflow list together)
constexpr int DEEP_MIN_SLOTS = 32;      // fewest slots of a deep candidate region: a wave row's rows of one gallery tile at the 64-query tile
constexpr int DEEP_MAX_REGIONS = 2048;  // most producer regions per query gather_cands scans, on every route (256 phases x 8 wave rows)
constexpr int DEEP_TARGET_MUL = 2;      // the sampled threshold aims at DEEP_TARGET_MUL * k_eff + DEEP_TARGET_ADD candidates per query,
constexpr int DEEP_TARGET_ADD = 512;    //   and the sample resolves that many only from
constexpr int DEEP_GROUP_ROWS = 512;    //   deep_min_rows = target * DEEP_GROUP_ROWS / (groups per 256-row tile) gallery rows on
constexpr int MAX_DIMP = 4096;

struct Cand {          // one row that passed the bf16 threshold filter
    float s;           // approximate score (bf16 MFMA, fp32 accumulate [+ bias])
    int32_t row;       // gallery row
};

struct Hit {           // one exactly scored row
    double s;          // fp64 ranking score (lane-tree order)
    int64_t id;
};

// `a` ranks before `b`: higher score first, then lower id.
__host__ __device__ inline bool hit_before(double sa, int64_t ia, double sb, int64_t ib) {
    return sa > sb || (sa == sb && ia < ib);
}

// The radix ranking's sort key (k_ranksort.hip): an unsigned 64-bit image of an fp64 ranking score that ASCENDS as the score
// descends, so an ascending sort ranks best first: rank_key(a) < rank_key(b) iff a > b for every pair that is not NaN.  The
// usual bit trick (flip all bits of a negative value, the sign bit of the others) gives an ascending image; its complement is
// the key.  hit_before compares with ==, for which -0.0 and +0.0 tie, so -0.0 takes +0.0's key.  -inf has the largest key of
// any number (0xFFF0000000000000); a NaN lands outside the numbers (before +inf or after -inf, by its sign bit).
__host__ __device__ inline uint64_t rank_key(double s) {
    uint64_t u;
    __builtin_memcpy(&u, &s, 8);
    if ((u << 1) == 0) u = 0;                              // -0.0 -> +0.0
    return (u >> 63) ? u : ~u ^ 0x8000000000000000ull;     // = ~(u ^ (negative ? all ones : the sign bit))
}
// The key that sorts after every score's: rows that a top-k ranking leaves out (k_ranksort.hip).
constexpr uint64_t RANK_KEY_LAST = ~0ull;
// Elements one workgroup of the radix ranking's scatter orders at a time (mirx_rank_sort_tile, tests reach its boundaries).
constexpr int RANK_TILE = 4096;
// Rows one workgroup of the compaction's scan covers (mirx_compact_tile, tests reach its boundaries).
constexpr int COMPACT_TILE = 2048;

// CUs of the CURRENT device, cached per device (a process that drives several GPUs sizes every persistent grid for the one it
// launches on).  Host threads launch concurrently: the cache is atomic, and two threads that both miss store the same value.
inline int current_device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    int v = cache[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        v = 256;
        (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev);
        if (v <= 0) v = 256;
        cache[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

// Raise `kernel`'s dynamic-LDS limit to `bytes` on the current device -- every launcher that needs more than the default goes
// through here.  `once` = the call site's `static std::atomic<unsigned long long>` (one bit per device), for a byte count that
// is fixed for that call site (per instantiation): the attribute is set on the site's first launch on each device and the
// call costs nothing afterwards.  The bit goes in only after hipFuncSetAttribute has succeeded, so a failure is reported and
// the next launch tries again; threads that race on a first use each set the same value.  No `once` = a byte count that
// depends on runtime arguments: set on every launch.
template <typename Kernel>
inline hipError_t set_dynamic_lds(Kernel *kernel, size_t bytes, std::atomic<unsigned long long> *once = nullptr) {
    int dev = -1;
    if (once && (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)) dev = -1;      // unknown device: set it again
    if (dev >= 0 && (once->load(std::memory_order_acquire) >> dev & 1ull)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)bytes);
    if (e == hipSuccess && dev >= 0) once->fetch_or(1ull << dev, std::memory_order_release);
    return e;
}

}  // namespace mirx
