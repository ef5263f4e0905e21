// mirx_device.h -- the device helpers every kernel file of libmirx shares (gfx950 only): vector types, wave reductions, the
// NaN-keeping scalar ops, the term splits and a few macros.  Each exists ONCE, here; a k_*.hip keeps only what it alone uses.
// Device code only: every k_*.hip includes this header, host-only translation units include mirx_common.h.
#pragma once
#include "mirx_common.h"
#include "mirx_kernels.h"      // CandLists, which gather_cands reads

namespace mirx {

// ---- vector types ---------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// a generic pointer into LDS as the address-space-3 pointer the LDS-DMA builtins take
#define LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))

// ---- the term order of a product block: defined HERE and nowhere else -----------------------------------------------
// The bit-identity tests pin the summation order, so every kernel of a scheme issues the same (A term, B term) sequence,
// smallest products first.  SWAP (compile-time) exchanges the MFMA's operand SLOTS -- the result comes out transposed, rows
// <-> lanes -- and leaves the SEQUENCE alone: calling a block with A and B exchanged instead would issue l*h and h*l in the
// opposite order and round differently.
#define MIRX_MFMA_TERM(OP, C, A, B, SWAP) C = (SWAP) ? OP(B, A, C, 0, 0, 0) : OP(A, B, C, 0, 0, 0);
// two fp16 terms per operand: the three cross terms that matter (l*h, h*l, h*h)
#define MIRX_MFMA3_SLOTS(C, AH, AL, BH, BL, SWAP)                                   \
    {                                                                               \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_f16, C, AL, BH, SWAP)     \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_f16, C, AH, BL, SWAP)     \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_f16, C, AH, BH, SWAP)     \
    }
#define MIRX_MFMA3(C, AH, AL, BH, BL) MIRX_MFMA3_SLOTS(C, AH, AL, BH, BL, false)
// three bf16 terms per operand: the six that matter (m*m, l*h, h*l, m*h, h*m, h*h)
#define MIRX_MFMA6_SLOTS(C, AH, AM, AL, BH, BM, BL, SWAP)                           \
    {                                                                               \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_bf16, C, AM, BM, SWAP)    \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_bf16, C, AL, BH, SWAP)    \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_bf16, C, AH, BL, SWAP)    \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_bf16, C, AM, BH, SWAP)    \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_bf16, C, AH, BM, SWAP)    \
        MIRX_MFMA_TERM(__builtin_amdgcn_mfma_f32_32x32x16_bf16, C, AH, BH, SWAP)    \
    }
#define MIRX_MFMA6(C, AH, AM, AL, BH, BM, BL) MIRX_MFMA6_SLOTS(C, AH, AM, AL, BH, BM, BL, false)

__device__ inline int lane_id() { return threadIdx.x & 63; }

// ---- wave reductions ------------------------------------------------------------------------------------------------
// All are the butterfly s[l] = s[l] (op) s[l ^ off], off = 32 .. 1 -- the order search_ref.c and the saliency kernels' float64
// restatements pin.  The ops commute bit for bit, so every lane ends with the same value.
__device__ inline double wave_butterfly_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ inline int wave_isum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- NaN-keeping scalar ops -----------------------------------------------------------------------------------------
// torch's relu / clamp(min=0), amax / max and amin / min PROPAGATE a NaN (fmaxf, fminf and v_max_f32 drop it): a comparison
// with a NaN is false, so `a != a` lets it through.  The saliency kernels are specified bit for bit against torch, NaN included.
__device__ inline float relu_nan(float v) { return (v > 0.f || v != v) ? v : 0.f; }
__device__ inline float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ inline float nanmin(float a, float b) { return (a < b || a != a) ? a : b; }

// wave maximum that DROPS a NaN (fmaxf) ...
__device__ inline float wave_fmax(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// ... and the one that keeps it (nanmax)
__device__ inline float wave_nanmax(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = nanmax(v, __shfl_xor(v, off, 64));
    return v;
}

// max of a value over the two 32-lane halves of the wave, in every lane: v_permlane32_swap (gfx950) hands each half the other's
// value inside the vector unit -- the ds_bpermute of __shfl_xor(.., 32) was an LDS round trip on the critical path of every tile
__device__ inline float max_over_halves(float v) {
    const unsigned b = __float_as_uint(v);
    const u32x2 r = __builtin_amdgcn_permlane32_swap(b, b, false, false);    // r[0] = the low half's value, r[1] = the high half's
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// 2^x as the bare v_exp_f32.  exp2f() wraps the instruction in a compare, two selects, an add and a multiply so that results below
// 2^-126 come out as denormals; a softmax weight that small changes neither the running sum (>= 1) nor its bf16 terms, and the
// wrapper was 4 of every 6 VALU instructions of the softmax.
__device__ inline float exp2_raw(float x) { return __builtin_amdgcn_exp2f(x); }

// smallest power of two >= v (v >= 1)
__device__ inline int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Bitonic network over a[0 .. m) in LDS (m a power of two), every thread of the workgroup taking part: before(x, y) = x ranks
// in front of y.  Ends behind a barrier.
template <typename T, typename Before>
__device__ inline void bitonic_lds(T *a, int m, Before before) {
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (m >> 1); t += blockDim.x) {
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                const bool best_first = (i & size) == 0;
                const T x = a[i], y = a[j];
                if (before(y, x) == best_first) { a[i] = y; a[j] = x; }
            }
        }
    }
    __syncthreads();
}

// An unsigned image of an fp32 value that ascends with the value (the candidate sort of k_finalize.hip).
__device__ inline uint32_t f32_orderable(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float f32_from_orderable(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

// ---- the filter GEMM's candidate lists (CandLists, mirx_kernels.h) as their readers see them ---------------------------
constexpr int64_t ID_LAST = INT64_MAX;   // sentinel id of an empty Hit: sorts after every real id

// A candidate as one sortable word: the orderable s~ above the complemented row, so that descending keys rank the higher s~
// first and, among equal s~, the lower row.  One key per row: the keys of a query are distinct.
__device__ inline unsigned long long cand_key(const Cand cd) {
    return ((unsigned long long)f32_orderable(cd.s) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)cd.row);
}
__device__ inline float cand_key_score(unsigned long long key) { return f32_from_orderable((uint32_t)(key >> 32)); }
__device__ inline uint32_t cand_key_row(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull); }

struct Gathered {
    int raw;      // rows that passed the filter, counted by the regions (what the stats call candidates)
    int taken;    // entries the lists hold for the query: every region's min(count, slots), then the overflow list's
    bool lost;    // the overflow list overflowed, or `taken` exceeds the caller's capacity: nothing was put
};

// The candidates of query slot `slot_q`, by a workgroup of THREADS threads: put(p, cand) for every p in [0, taken), the regions'
// entries in region order, then the overflow list's.  Deterministic: the regions' takes are scanned (thread t owns the regions
// [t * per, (t + 1) * per)), then every thread copies flattened positions, finding a position's region by a binary search of
// the offsets.  roff = LDS scratch of L.regions + 1 <= DEEP_MAX_REGIONS + 1 ints, free again on return.  Ends behind a barrier.
template <int THREADS, typename Put>
__device__ inline Gathered gather_cands(const CandLists &L, int slot_q, int cap, int *roff, Put put) {
    constexpr int WAVES = THREADS / WAVE;
    __shared__ int sh_wsum[WAVES], sh_wraw[WAVES];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int per = (L.regions + THREADS - 1) / THREADS;
    const int *rcnt = L.region_cnt + (int64_t)slot_q * L.regions;
    const int oc = L.ovf_cnt[slot_q];                               // read beside the region counts, not behind a barrier
    int mine = 0, raw = 0;
    for (int j = 0; j < per; ++j) {
        const int rg = threadIdx.x * per + j;
        if (rg < L.regions) {
            const int cr = rcnt[rg];
            raw += cr;
            mine += cr < L.slots ? cr : L.slots;
        }
    }
    int incl = mine;                                                // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int v = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += v;
    }
    raw = wave_isum(raw);
    if (lane == WAVE - 1) sh_wsum[wave] = incl;
    if (lane == 0) sh_wraw[wave] = raw;
    __syncthreads();
    int base = 0, c_reg = 0;
    Gathered g;
    g.raw = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        if (w < wave) base += sh_wsum[w];
        c_reg += sh_wsum[w];
        g.raw += sh_wraw[w];
    }
    int at = base + incl - mine;                                    // exclusive offset of this thread's first region
    for (int j = 0; j < per; ++j) {
        const int rg = threadIdx.x * per + j;
        if (rg < L.regions) {
            roff[rg] = at;
            const int cr = rcnt[rg];
            at += cr < L.slots ? cr : L.slots;
        }
    }
    if (threadIdx.x == 0) roff[L.regions] = c_reg;
    const int otake = oc < CAND_OVF ? oc : CAND_OVF;
    // (a full overflow list has lost rows; the candidates of the regions and of the list share the one capacity)
    g.taken = c_reg + otake;
    g.lost = oc > CAND_OVF || g.taken > cap;
    __syncthreads();
    if (!g.lost) {
        const Cand *qcand = L.cand + (int64_t)slot_q * L.regions * L.slots;
        for (int i = threadIdx.x; i < c_reg; i += THREADS) {
            int lo_r = 0, hi_r = L.regions;                         // the last region with roff[rg] <= i (empty regions share offsets)
            while (hi_r - lo_r > 1) {
                const int mid = (lo_r + hi_r) >> 1;
                if (roff[mid] <= i) lo_r = mid; else hi_r = mid;
            }
            put(i, qcand[(int64_t)lo_r * L.slots + (i - roff[lo_r])]);
        }
        for (int i = threadIdx.x; i < otake; i += THREADS) put(c_reg + i, L.ovf[(int64_t)slot_q * CAND_OVF + i]);
    }
    __syncthreads();
    return g;
}

// fp32 -> bf16, round to nearest even (finite inputs).
__device__ inline uint16_t f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// Lane-tree fp64 score of two fp32 rows of `dimp` (multiple of 64) elements.
// METRIC 0: sum q*g ; METRIC 1: -(sum (q-g)^2).  All lanes return the same value.
template <int METRIC>
__device__ inline double lane_tree_score(const float *__restrict__ q, const float *__restrict__ g,
                                         int dimp) {
    const int lane = lane_id();
    const int nchunk = dimp >> 2;
    double acc = 0.0;
    for (int c = lane; c < nchunk; c += WAVE) {
        const float4 a = *reinterpret_cast<const float4 *>(q + 4 * c);
        const float4 b = *reinterpret_cast<const float4 *>(g + 4 * c);
        if (METRIC == 0) {
            acc = fma((double)a.x, (double)b.x, acc);
            acc = fma((double)a.y, (double)b.y, acc);
            acc = fma((double)a.z, (double)b.z, acc);
            acc = fma((double)a.w, (double)b.w, acc);
        } else {
            double d;
            d = (double)a.x - (double)b.x; acc = fma(d, d, acc);
            d = (double)a.y - (double)b.y; acc = fma(d, d, acc);
            d = (double)a.z - (double)b.z; acc = fma(d, d, acc);
            d = (double)a.w - (double)b.w; acc = fma(d, d, acc);
        }
    }
    acc = wave_butterfly_sum(acc);
    return METRIC == 0 ? acc : -acc;
}

// The filter GEMM's error bound: |s~ - s'| <= eps for every row, s' the score the GEMM approximates.  bf16 rounding of
// both operands (2^-8 + 2^-18), fp32 accumulation of dimp products (dimp * 2^-23, a 2x margin over gamma_n), and for metric 1 the
// fp32 bias and its add.  Every product is nudged upward.  qn / gmax: upper bounds of ||q|| and of the largest ||g||.
template <int METRIC>
__device__ inline float filter_eps(float qn, float gmax, int dimp) {
    float eps = qn * gmax * (0.00390625f + 3.8147e-6f + (float)dimp * 1.1920929e-7f) * 1.00001f;
    if (METRIC == 1) eps += 1.1920929e-7f * (gmax * gmax + qn * gmax) * 1.00001f;
    return eps;
}

// What the search boundary reports for an fp64 ranking score: metric 0 the dot product, metric 1 -sqrt of the squared distance.
__device__ inline float reported_value(double rank_score, int metric) {
    if (rank_score == -INFINITY) return -INFINITY;
    return metric == MIRX_METRIC_IP ? (float)rank_score : (float)(-sqrt(fmax(-rank_score, 0.0)));
}

// tanh-form GELU (transformers "gelu_pytorch_tanh", the SigLIP MLP activation): 0.5 v (1 + tanh(u)), u = sqrt(2/pi) (v + 0.044715 v^3).
// 1 + tanh(u) = 2 / (1 + e^(-2u)) exactly, so the value is v / (1 + 2^(v (K1 + K2 v^2))) with K1 = -2 sqrt(2/pi) log2(e), K2 =
// 0.044715 K1: one v_exp_f32 and one v_rcp_f32 instead of tanhf's ~25 instructions (the Linear epilogues are VALU-bound on their
// activation).  Against float64 over [-12, 12]: 7.4e-7 absolute, 1.3e-6 relative where |value| > 1e-3 -- the tanhf form measures
// 6.7e-7 and 5e-5 (it cancels in 1 + tanh for negative arguments).
__device__ inline float gelu_tanh(float v) {
    const float a = fmaf(v * v, -0.10294324159622192f, -2.302208185195923f);
    return v * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * a));
}

// erf-form GELU (torch.nn.GELU()).  A branch-free erf (two fitted polynomials evaluated for every value so that neighbours pair
// into packed fp32 instructions, tools/fit_gelu.py) was built and measured: DINOv2 1 031 -> 1 032 img/s, ConvNeXtV2 2 049 ->
// 2 021 -- ocml's erff mostly runs ONE of its branches per wave (|z| < 1 for most activations), which is cheaper than both
// polynomials at half price.  Kept: erff.
__device__ inline float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// ---- value ranges that travel with activations (two-fp16-term kernels) ---------------------------------
// PER IMAGE: a buffer's range is one fp32 per image (a "range row" [n], zeroed once per forward).  A producer folds the
// largest |value| it wrote for image b into row[b] with an unsigned atomic max: the bit patterns of non-negative floats
// order like the floats, +inf and NaN sort above every finite value, so a non-finite activation makes THAT image's
// consumer scale NaN and its embedding NaN (loud, never a silently wrong finite number) and leaves its batch mates
// untouched.  A consumer reads row[b] and derives the power-of-two staging scale of image b: an image's arithmetic does
// not depend on what else is in the batch.
__device__ inline float range_max(float m, float v) {
    // max(m, |v|) that keeps a NaN (fmaxf would drop it)
    const float a = fabsf(v);
    return (a > m || a != a) ? a : m;
}

// every lane of the wave belongs to image `img` (wave-uniform): one atomic per wave
__device__ inline void range_publish(unsigned *__restrict__ row, int img, float vmax, int lane) {
    unsigned a = __float_as_uint(vmax);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)a, off, 64);
        a = o > a ? o : a;
    }
    if (lane == 0 && a) atomicMax(row + img, a);
}

// lanes may belong to different images (a pixel tile that straddles images; a lane that carries nothing passes a valid
// image index and vmax = 0): one atomic per DISTINCT image of the wave -- the images are peeled off one at a time (lowest
// pending lane's image, masked wave maximum): one round per distinct image, two or three for a 128-pixel tile on ResNet-50's
// 224 x 224 maps, up to 16 where the map is 1 x 1 and the 16 pixels of an accumulator column are 16 images (k_conv_t2)
__device__ inline void range_publish_lanes(unsigned *__restrict__ row, int img, float vmax, int lane) {
    const unsigned a = __float_as_uint(vmax);
    bool pending = true;
    for (;;) {
        const unsigned long long bm = __ballot(pending);           // wave-uniform
        if (!bm) break;
        const int src = __ffsll((long long)bm) - 1;
        const int cur = __shfl(img, src, 64);
        const bool mine = pending && img == cur;
        unsigned m = mine ? a : 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
            m = o > m ? o : m;
        }
        if (lane == src && m) atomicMax(row + cur, m);
        pending = pending && !mine;
    }
}

// bound >= every |value|: x_scale = 2^(14 - floor(log2 bound)) puts bound * x_scale in [2^14, 2^15) (fp16 overflows at
// 65504); inv = 1 / x_scale.  bound == 0 (or subnormal) -> 1; non-finite -> NaN.
__device__ inline void range_scales(float bound, float &x_scale, float &inv) {
    const unsigned u = __float_as_uint(bound);
    const int e = (int)((u >> 23) & 0xffu) - 127;
    if (!(bound < 3.0e38f) || (u >> 31)) {
        x_scale = inv = __uint_as_float(0x7fc00000u);
    } else if (e < -100) {
        x_scale = inv = 1.f;
    } else {
        x_scale = __uint_as_float((unsigned)(127 + 14 - e) << 23);
        inv = __uint_as_float((unsigned)(127 - 14 + e) << 23);
    }
}

// ---- term splitting -------------------------------------------------------------------------------------------------
// The two fp16 terms of a pair of fp32 values: hi = RNE(v) (one v_cvt_pk_f16_f32), lo = RNE(v - hi) where v - hi comes from
// v_fma_mix_f32, which reads the fp16 half in place (exact: the difference of a float and its fp16 rounding is a float).  The
// compiler's form of `v - float(hi)` converts hi back with an SDWA instruction per value and subtracts with a packed fp32 op:
// five instructions per pair, two of them the kind that cost 10+ cycles beside an MFMA stream; this is four plain ones.
__device__ inline void split2h_pair(float v0, float v1, unsigned &hi, unsigned &lo) {
    const f32x2 vv = {v0, v1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(vv, f16x2));
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hi), "v"(v0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hi), "v"(v1));
    const f32x2 rr = {r0, r1};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(rr, f16x2));
}

// 8 fp32 values -> two fp16x8 fragments
__device__ inline void split2h_x8(const float (&v)[8], f16x8 &h, f16x8 &l) {
    u32x4 ph, pl;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        unsigned th, tl;
        split2h_pair(v[2 * p], v[2 * p + 1], th, tl);
        ph[p] = th; pl[p] = tl;
    }
    h = __builtin_bit_cast(f16x8, ph);
    l = __builtin_bit_cast(f16x8, pl);
}

// The three bf16 terms of a pair of fp32 values: h = RNE(v), m = RNE(v - h), l = RNE(v - h - m) (both differences exact).
__device__ inline void split3b_pair(float a, float b, unsigned &h, unsigned &m, unsigned &l) {
    const f32x2 v = {a, b};
    const bf16x2 vh = __builtin_convertvector(v, bf16x2);
    const f32x2 r1 = v - __builtin_convertvector(vh, f32x2);
    const bf16x2 vm = __builtin_convertvector(r1, bf16x2);
    const f32x2 r2 = r1 - __builtin_convertvector(vm, f32x2);
    const bf16x2 vl = __builtin_convertvector(r2, bf16x2);
    h = __builtin_bit_cast(unsigned, vh);
    m = __builtin_bit_cast(unsigned, vm);
    l = __builtin_bit_cast(unsigned, vl);
}

// 8 fp32 values -> three bf16x8 fragments
__device__ inline void split3b_x8(const float (&v)[8], bf16x8 &h, bf16x8 &m, bf16x8 &l) {
    u32x4 ph, pm, pl;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        unsigned th, tm, tl;
        split3b_pair(v[2 * p], v[2 * p + 1], th, tm, tl);
        ph[p] = th; pm[p] = tm; pl[p] = tl;
    }
    h = __builtin_bit_cast(bf16x8, ph);
    m = __builtin_bit_cast(bf16x8, pm);
    l = __builtin_bit_cast(bf16x8, pl);
}

// ---- term schemes ---------------------------------------------------------------------------------------------------
// What a kernel template needs to know about "an fp32 operand as a few 16-bit terms", highest term first (k_linear_split.hip):
// T terms per operand, the MFMA fragment type, SCALED = the terms have fp16's range, so the caller's power-of-two scales apply
// (x_scale while staging, its inverse on the accumulator), the split of a pair of values into T packed pairs and of eight values
// into T fragments (k_attention_split.hip), and the product block c += a b in the scheme's term order (SWAP as above).
struct SplitBf16x3 {
    static constexpr int T = 3;
    static constexpr bool SCALED = false;
    typedef bf16x8 frag;
    __device__ static void split_pair(float v0, float v1, float, unsigned (&t)[3]) { split3b_pair(v0, v1, t[0], t[1], t[2]); }
    __device__ static void split_x8(const float (&v)[8], frag (&t)[3]) { split3b_x8(v, t[0], t[1], t[2]); }
    template <bool SWAP>
    __device__ static void product(f32x16 &c, const frag (&a)[3], const frag (&b)[3]) {
        MIRX_MFMA6_SLOTS(c, a[0], a[1], a[2], b[0], b[1], b[2], SWAP)
    }
};
struct SplitF16x2 {
    static constexpr int T = 2;
    static constexpr bool SCALED = true;
    typedef f16x8 frag;
    __device__ static void split_pair(float v0, float v1, float x_scale, unsigned (&t)[2]) {
        split2h_pair(v0 * x_scale, v1 * x_scale, t[0], t[1]);
    }
    __device__ static void split_x8(const float (&v)[8], frag (&t)[2]) { split2h_x8(v, t[0], t[1]); }
    template <bool SWAP>
    __device__ static void product(f32x16 &c, const frag (&a)[2], const frag (&b)[2]) {
        MIRX_MFMA3_SLOTS(c, a[0], a[1], b[0], b[1], SWAP)
    }
};

// Four consecutive channels `ch ..` (ch % 4 == 0) of token row `row` of a [rows, c] matrix written as "terms rows" (k_linear_t2.hip:
// per 32 features one 128-byte line, fp16 high terms | fp16 low terms of scale * value): the input format of the DMA-fed Linear.
__device__ inline void store_terms4(char *out_t, int64_t row, int c, int ch, const f32x4 &v, float scale) {
    unsigned h0, l0, h1, l1;
    split2h_pair(v[0] * scale, v[1] * scale, h0, l0);
    split2h_pair(v[2] * scale, v[3] * scale, h1, l1);
    const u32x2 hi = {h0, h1}, lo = {l0, l1};
    char *dst = out_t + row * ((int64_t)((c + 31) / 32 * 32) * 4) + (ch >> 5) * 128 + (ch & 31) * 2;
    *reinterpret_cast<u32x2 *>(dst) = hi;
    *reinterpret_cast<u32x2 *>(dst + 64) = lo;
}

// ---- the saliency maps' upsample (k_simcam.hip, k_simatt.hip) -------------------------------------------------------
// Output pixel (y, x) of an h x w map `m` (row-major) resized by F.interpolate(mode="bilinear", align_corners=False): ATen's
// upsample_bilinear2d source index max(scale * (dst + 0.5) - 0.5, 0) with scale sh = h / H, sw = w / W, the upper neighbour
// clamped to the last row / column.
__device__ inline float bilinear_half_pixel(const float *m, int h, int w, float sh, float sw, int y, int x) {
    const float fy = fmaxf(sh * ((float)y + 0.5f) - 0.5f, 0.f);
    const float fx = fmaxf(sw * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * m[y0 * w + x0] + lx * m[y0 * w + x1]) + ly * (hx * m[y1 * w + x0] + lx * m[y1 * w + x1]);
}

}  // namespace mirx
