// route_probe.cpp -- csrc/mirx_route.h behind a pipe, for tests/test_route_cpu.py: host C++ alone, no HIP, no library.
// stdin: the six RouteLimits, then one call per line
//   tiers_auto size k has_exclude extra allow_deep masked n_allowed tile_groups row_bytes gather_max
// stdout per call: list rows most_rows deep_min_rows(k_eff, tile_groups), the enums by their numbers.
#include <cstdio>

#include "../image-retrieval---thesis-2026_amd/csrc/mirx_route.h"

int main() {
    mirx::RouteLimits lim{};
    long long v[11];
    if (std::scanf("%lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 6) return 2;
    lim.tier1_min_rows = v[0];
    lim.tier1_max_k = v[1];
    lim.max_k = v[2];
    lim.deep_target_mul = v[3];
    lim.deep_target_add = v[4];
    lim.deep_group_rows = v[5];
    for (;;) {
        int got = 0;
        while (got < 11 && std::scanf("%lld", &v[got]) == 1) ++got;
        if (got == 0) return 0;
        if (got != 11) return 3;
        mirx::RouteCall c{};
        c.tiers_auto = v[0] != 0;
        c.size = v[1];
        c.k = v[2];
        c.has_exclude = v[3] != 0;
        c.extra = v[4];
        c.allow_deep = v[5] != 0;
        c.tile_groups = v[8];
        c.row_bytes = v[9];
        c.gather_max = v[10];
        const mirx::Route r = mirx::route_pick(lim, c, v[6] != 0, v[7]);
        std::printf("%d %d %lld %lld\n", (int)r.list, (int)r.rows, (long long)mirx::route_most_rows(lim, c),
                    (long long)mirx::deep_min_rows(lim, mirx::route_open(lim, c).k_eff, c.tile_groups));
    }
}
