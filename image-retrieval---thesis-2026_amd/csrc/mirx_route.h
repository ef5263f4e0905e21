// mirx_route.h -- which route answers a top-k search: a pure function of plain integers, no HIP, no index.
// mirx_index.hip's search_call is its one caller in the library; tests/route_probe.cpp compiles it with a host compiler alone.
// The answer of a search never depends on the route -- only its cost does.
#pragma once
#include <stdint.h>

namespace mirx {

// The constants the decision reads (mirx_api.hip's and mirx_common.h's, handed in so that this header includes neither).
struct RouteLimits {
    int64_t tier1_min_rows;      // TIER1_MIN_ROWS: fewer rows go to the exact scan
    int64_t tier1_max_k;         // TIER1_MAX_K: the most k_eff the filter route's candidate lists answer
    int64_t max_k;               // MAX_K
    int64_t deep_target_mul, deep_target_add, deep_group_rows;   // DEEP_TARGET_MUL / _ADD, DEEP_GROUP_ROWS
};

// One call, as its entry point received it.
struct RouteCall {
    bool tiers_auto;             // MIRX_OPT_TIERS is on auto
    int64_t size;                // rows of the index
    int64_t k;
    bool has_exclude;            // exclude ids were passed
    int64_t extra;               // rows a leave-group-out query may drop (the caller's hint), else 0
    bool allow_deep;             // the entry point may take the deep route (mirx_index_search_deep / _leave_out)
    int64_t tile_groups;         // threshold groups per 256-row gallery tile at the query tile of the call's widest batch
    int64_t row_bytes;           // bytes one gathered row takes (fp32 row + id)
    int64_t gather_max;          // most bytes the gathered rows of a masked call may take
};

enum class RouteList { EXACT, FILTER, DEEP };                    // who ranks: the exact scan, or candidate lists of either depth
enum class RouteRows { INDEX, NEUTRALISED, GATHERED, NONE };     // what is scanned: the index's rows, all rows with the masked
                                                                 // ones neutralised, the allowed rows gathered, nothing
struct Route {
    RouteList list;
    RouteRows rows;
};

// ---- the deep route's reach -------------------------------------------------------------------------------------
// The sampled threshold is the j-th largest of `ngroups` group maxima of every stride-th row, ngroups * stride ~ size *
// tile_groups / 256: it resolves candidate counts only up to about half the groups deep.  The deep route aims at
// target = DEEP_TARGET_MUL * k_eff + DEEP_TARGET_ADD candidates per query (k_eff, the 2 eps band below the k-th score, room for
// tau < lo) and is taken only where target <= ngroups * stride / 2, i.e. from target * DEEP_GROUP_ROWS / tile_groups rows on;
// smaller galleries go to the exact scan, where it costs little.
inline int64_t deep_target(const RouteLimits &lim, int64_t k_eff) { return lim.deep_target_mul * k_eff + lim.deep_target_add; }

inline int64_t deep_min_rows(const RouteLimits &lim, int64_t k_eff, int64_t tile_groups) {
    const int64_t rows = deep_target(lim, k_eff) * lim.deep_group_rows / tile_groups;
    return rows > lim.tier1_min_rows ? rows : lim.tier1_min_rows;
}

// What the call's arguments open before any row is counted.  k_eff = k, the excluded id and the leave-out hint: the candidates a
// list must hold.  With k + extra past MAX_K (the excluded id rides on top, as it always has at k = MAX_K) no list route is open.
struct RouteOpen {
    int64_t k_eff;
    bool deep;                   // the deep route, from deep_rows rows on
    bool filter;                 // the filter route, from TIER1_MIN_ROWS rows on
    int64_t deep_rows;
};

inline RouteOpen route_open(const RouteLimits &lim, const RouteCall &c) {
    RouteOpen o;
    o.k_eff = c.k + (c.has_exclude ? 1 : 0) + c.extra;
    o.deep = c.allow_deep && c.tiers_auto && o.k_eff > lim.tier1_max_k && c.k + c.extra <= lim.max_k;
    o.filter = c.tiers_auto && o.k_eff <= lim.tier1_max_k;
    o.deep_rows = deep_min_rows(lim, o.k_eff, c.tile_groups);
    return o;
}

// The most allowed rows a masked call can have to gather: sizes the gather and code scratch before the mask has been counted
// (at or past the row count of an open list route the rows are neutralised in place instead).
inline int64_t route_most_rows(const RouteLimits &lim, const RouteCall &c) {
    const RouteOpen o = route_open(lim, c);
    const int64_t bound = o.deep ? o.deep_rows - 1 : (o.filter ? lim.tier1_min_rows - 1 : c.size);
    return bound < c.size ? bound : c.size;
}

// The route.  masked: the call carries a row mask that leaves n_allowed of the index's rows.
inline Route route_pick(const RouteLimits &lim, const RouteCall &c, bool masked, int64_t n_allowed) {
    const RouteOpen o = route_open(lim, c);
    const int64_t rows = masked ? n_allowed : c.size;      // the rows that can rank
    // (at most one list route is open to a call: the deep one needs k_eff past TIER1_MAX_K, the filter one at most that)
    const RouteList list = o.deep && rows >= o.deep_rows            ? RouteList::DEEP
                           : o.filter && rows >= lim.tier1_min_rows ? RouteList::FILTER
                                                                    : RouteList::EXACT;
    if (!masked || n_allowed == c.size) return {list, RouteRows::INDEX};        // nothing masked: the plain search, bit for bit
    if (list != RouteList::EXACT) return {list, RouteRows::NEUTRALISED};
    if (n_allowed <= 0) return {RouteList::EXACT, RouteRows::NONE};
    return {RouteList::EXACT, n_allowed * c.row_bytes > c.gather_max ? RouteRows::NEUTRALISED : RouteRows::GATHERED};
}

}  // namespace mirx
