// k_group.hip -- grouping search: the best hits PER GROUP instead of the best rows.
//
//   k_group_walk   one wavefront walks one query's ranked prefix (best first) 64 entries at a time and keeps, per group in the
//                  order the groups first appear, the first `group_size` rows -- the walk of the contract in include/mirx.h.  The
//                  open groups live in a per-wave LDS hash table.  It also says what the prefix could decide (complete / groups
//                  final), so the driver knows which queries need the fill or a deeper prefix.
//   k_group_count  eligible rows per group code (integer atomics: the sums do not depend on the order).
//   k_group_fill   completes a group whose membership is decided but whose rows the prefix did not reach: scores every member
//                  row with lane_tree_score (the ranking's own bits) and keeps the best `group_size` by (score, id).
#include <algorithm>

#include "mirx_device.h"
#include "mirx_kernels.h"

namespace mirx {

namespace {

// pow2_ceil for the launchers (mirx_device.h's is device code)
inline int pow2_ceil_host(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// ---- the walk -------------------------------------------------------------------------------------------------------
// LDS of one wave: key[P] (the group code in a slot of the hash table, -1 = free), val[P] (its group slot), and per group slot
// kept[P / 2] / need[P / 2] (rows held, rows it can hold = min(group_size, eligible rows of the group for this query)).
// P is a power of two >= 2 * limit, so the table is never more than half full and a probe always ends.
__device__ inline int walk_find(const int *key, int P, int code) {
    int i = code & (P - 1);
    for (;;) {
        const int k = key[i];
        if (k == code || k == -1) return i;
        i = (i + 1) & (P - 1);
    }
}

__global__ __launch_bounds__(256) void k_group_walk(GroupWalkArgs a) {
    extern __shared__ __attribute__((aligned(16))) int walk_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (q >= a.nq) return;                                   // (no workgroup barrier below: waves run on their own)
    const int P = a.table;
    int *key = walk_lds + (size_t)wave * (3 * P);
    int *val = key + P;
    int *kept = val + P;
    int *need = kept + (P >> 1);
    for (int i = lane; i < P; i += 64) key[i] = -1;

    const int limit = a.limit, gs = a.group_size;
    const int64_t eg = a.excl_group ? a.excl_group[q] : -1;
    int64_t live = a.live_groups;
    if (eg >= 0 && eg < a.n_groups && a.group_rows[eg] == 1) live -= 1;      // the excluded row was its group's only one
    const int T = (int)(live < (int64_t)limit ? (live < 0 ? 0 : live) : limit);
    const int64_t *row = a.ranks + q * a.row_stride;
    const int64_t *tix = a.table_index ? a.table_index + q * a.row_stride : nullptr;
    const double *sc = a.scores ? a.scores + q * a.row_stride : nullptr;
    int64_t *oid = a.out_ids + q * (int64_t)limit * gs;
    double *osc = a.out_scores ? a.out_scores + q * (int64_t)limit * gs : nullptr;
    int64_t *ocode = a.out_codes + q * limit;

    int open = 0, nfull = 0;                                 // wave-uniform: groups opened, groups holding all they can
    bool ended = false;                                      // a -1 entry: the prefix is the whole eligible ranking
    bool complete = T == 0;
    for (int64_t i0 = 0; i0 < a.depth && !complete && !ended; i0 += 64) {
        const int64_t r = i0 + lane;
        int64_t id = -1, e = -1;
        if (r < a.depth) {
            id = row[r];
            e = tix ? tix[r] : id;
        }
        const bool in_list = r < a.depth && id >= 0 && e >= 0;
        const unsigned long long endmask = __ballot(r < a.depth && !in_list);
        // entries behind the first -1 do not belong to the ranking
        const bool valid = in_list && (endmask == 0 || lane < __ffsll((long long)endmask) - 1);
        int code = -1, nd = 0;
        if (valid && e < a.n_table) {
            const int64_t c = a.group_of[e];
            if (c >= 0 && c < a.n_groups) {
                code = (int)c;
                const int64_t cnt = a.group_rows[c] - (c == eg ? 1 : 0);
                nd = (int)(cnt < (int64_t)gs ? cnt : gs);
            }
        }
        // Lanes whose row can no longer be kept whatever the lanes in front of them do: the group is open and full, or it is not
        // open and no slot is left.  Both states are absorbing, so the table as it stands at the top of the chunk decides them.
        bool pending = code >= 0 && nd > 0;
        if (pending) {
            const int h = walk_find(key, P, code);
            if (key[h] == code) pending = kept[val[h]] < need[val[h]];
            else pending = open < limit;
        }
        // the rest in lane order, each doing its own lookup at its turn: the lanes before it may have opened its group, filled
        // it, or taken the last slot
        for (;;) {
            const unsigned long long todo = __ballot(pending);
            if (todo == 0) break;
            const int src = __ffsll((long long)todo) - 1;
            int d_open = 0, d_full = 0;
            if (lane == src) {
                const int h = walk_find(key, P, code);
                int s = -1;
                if (key[h] == code) {
                    s = val[h];
                } else if (open < limit) {
                    s = open;
                    key[h] = code;
                    val[h] = s;
                    kept[s] = 0;
                    need[s] = nd;
                    ocode[s] = code;
                    d_open = 1;
                }
                if (s >= 0) {
                    const int k = kept[s];
                    if (k < need[s]) {
                        oid[(int64_t)s * gs + k] = id;
                        if (osc) osc[(int64_t)s * gs + k] = sc[r];
                        kept[s] = k + 1;
                        d_full = k + 1 == need[s] ? 1 : 0;
                    }
                }
                pending = false;
            }
            open += __shfl(d_open, src, 64);
            nfull += __shfl(d_full, src, 64);
            __builtin_amdgcn_wave_barrier();
            if (open == T && nfull == open) break;           // nothing behind this row can be kept
        }
        complete = open == T && nfull == open;
        ended = endmask != 0;
    }
    complete = complete || ended;
    // the slots the walk did not reach
    for (int i = lane; i < limit * gs; i += 64) {
        const int s = i / gs, m = i - s * gs;
        if (s >= open || m >= kept[s]) {
            oid[i] = -1;
            if (osc) osc[i] = -INFINITY;
        }
    }
    for (int s = lane; s < limit; s += 64) {
        if (s >= open) ocode[s] = -1;
        a.out_kept[q * limit + s] = s < open ? kept[s] : 0;
    }
    if (lane == 0) {
        a.out_state[q * 2] = open;
        a.out_state[q * 2 + 1] = (complete ? 1 : 0) | ((complete || open == T) ? 2 : 0);
    }
}

// ---- the counts -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_group_count(const int64_t *__restrict__ groups, const uint8_t *__restrict__ allow, int64_t n,
                                                     int64_t n_groups, unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    // whole waves enter every trip (the ballots below need all 64 lanes)
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < n; base += step) {
        const int64_t r = base + lane;
        int64_t code = -1;
        if (r < n && (!allow || allow[r] != 0)) {
            code = groups[r];
            if (code < 0 || code >= n_groups) code = -1;
        }
        // a few labels over many rows would put a whole wave on one address: the first distinct codes of the wave are added once
        // per wave, whatever is left after four rounds goes lane by lane
        bool pending = code >= 0;
        for (int round = 0; round < 4; ++round) {
            const unsigned long long bm = __ballot(pending);
            if (bm == 0) break;
            const int src = __ffsll((long long)bm) - 1;
            const int64_t cur = __shfl(code, src, 64);
            const bool mine = pending && code == cur;
            const unsigned long long mm = __ballot(mine);
            if (lane == src) atomicAdd(counts + cur, (unsigned long long)__popcll(mm));
            pending = pending && !mine;
        }
        if (pending) atomicAdd(counts + code, 1ull);
    }
}

// ---- the fill -------------------------------------------------------------------------------------------------------
// One workgroup per (query, group slot) pair: its waves score the group's member rows one row per wave, the workgroup sorts the
// (score, id) records in LDS and the first group_size go to the group's slots.
template <int METRIC>
__global__ __launch_bounds__(256) void k_group_fill(GroupFillArgs a) {
    extern __shared__ __attribute__((aligned(16))) Hit fill_lds[];
    const int p = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const int64_t q = a.pair_query[p];
    const int64_t slot = a.pair_slot[p];
    const int64_t first = a.pair_first[p];
    int64_t len = a.pair_len[p];
    if (q < 0 || q >= a.nq || slot < 0 || slot >= a.limit) return;            // workgroup-uniform
    if (len > a.max_members) len = a.max_members;                              // (the caller's promise; never read past LDS)
    if (len < 0 || first < 0 || first + len > a.n_members) len = 0;
    const int m = pow2_ceil((int)(len > 1 ? len : 1));
    const int64_t self = a.exclude ? a.exclude[q] : -1;
    const float *qrow = a.q32p + q * a.dimp;
    for (int i = wave; i < m; i += nwave) {
        Hit h{-INFINITY, INT64_MAX};                                           // padding and the excluded id: behind every row
        if (i < len) {
            const int64_t row = a.members[first + i];
            if (row >= 0 && row < a.n_rows) {
                const int64_t id = a.ids[row];
                if (!(a.exclude && id == self)) {
                    h.s = lane_tree_score<METRIC>(qrow, a.g32 + row * a.dimp, a.dimp);
                    h.id = id;
                }
            }
        }
        if (lane == 0) fill_lds[i] = h;
    }
    bitonic_lds(fill_lds, m, [](const Hit &x, const Hit &y) { return hit_before(x.s, x.id, y.s, y.id); });
    const int64_t base = (q * a.limit + slot) * a.group_size;
    for (int j = threadIdx.x; j < a.group_size; j += blockDim.x) {
        const bool have = j < m && fill_lds[j].id != INT64_MAX;
        a.out_ids[base + j] = have ? fill_lds[j].id : -1;
        a.out_f64[base + j] = have ? fill_lds[j].s : -INFINITY;
    }
}

}  // namespace

int group_walk_table(int limit) { return pow2_ceil_host(2 * limit < 64 ? 64 : 2 * limit); }

hipError_t launch_group_walk(const GroupWalkArgs &a0, hipStream_t st) {
    if (a0.nq <= 0) return hipSuccess;
    GroupWalkArgs a = a0;
    a.table = group_walk_table(a.limit);
    // 12 bytes of LDS per table slot and wave: four waves share a workgroup while that stays at 24 KiB, else one wave each
    const int waves = a.table <= 512 ? 4 : 1;
    const size_t lds = (size_t)waves * 3 * a.table * sizeof(int);
    const dim3 grid((unsigned)((a.nq + waves - 1) / waves));
    hipLaunchKernelGGL(k_group_walk, grid, dim3(64 * waves), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_group_count(const int64_t *groups, const uint8_t *allow, int64_t n, int64_t n_groups, int64_t *counts, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, (int64_t)current_device_cus() * 8);
    hipLaunchKernelGGL(k_group_count, dim3((unsigned)blocks), dim3(256), 0, st, groups, allow, n, n_groups,
                       reinterpret_cast<unsigned long long *>(counts));
    return hipGetLastError();
}

hipError_t launch_group_fill(const GroupFillArgs &a, int metric, hipStream_t st) {
    if (a.n_pairs <= 0) return hipSuccess;
    const size_t lds = (size_t)pow2_ceil_host((int)(a.max_members > 1 ? a.max_members : 1)) * sizeof(Hit);
    if (metric == MIRX_METRIC_IP) hipLaunchKernelGGL(k_group_fill<0>, dim3((unsigned)a.n_pairs), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(k_group_fill<1>, dim3((unsigned)a.n_pairs), dim3(256), lds, st, a);
    return hipGetLastError();
}

}  // namespace mirx
