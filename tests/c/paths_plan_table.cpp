// The plan of the path-record kernel (csrc/rt_paths_plan.h) on a CPU, for tests/test_paths_host.py.  One line in, one out:
//   plan  lds_total lds32_total n_nodes n_obj has_tex  block chunk bpc yield refill passes park  count  slots  cu_count per_cu
#include "../../ray-tracing-fsharp_amd/csrc/rt_paths_plan.h"

#include <cstdio>
#include <iostream>
#include <string>

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what != "plan") return 2;
        rtp::Settings s{};
        rtp::SceneSize sc;
        int tex = 0, count = 0, cu = 0, perCu = 0;
        unsigned long long slots = 0;
        std::cin >> sc.lds_total >> sc.lds32_total >> sc.n_nodes >> sc.n_objects >> tex;
        std::cin >> s.block >> s.chunk >> s.blocks_per_cu >> s.yield >> s.refill >> s.passes >> s.park;
        std::cin >> count >> slots >> cu >> perCu;
        if (!std::cin) return 2;
        sc.tex = tex != 0;
        if (rtp::check_settings(s)) { printf("error=1\n"); continue; }
        rtpp::PathsPlan pl = rtpp::plan_begin(sc, s, count != 0, slots);
        rtpp::plan_finish(pl, cu, perCu);
        printf("error=0 block=%d grid=%llu chunk=%d lds_bytes=%llu lds=%d counting=%d tex=%d slots=%llu\n", pl.block, (unsigned long long) pl.grid, pl.chunk,
               (unsigned long long) pl.lds_bytes, (int) pl.lds, (int) pl.count, (int) pl.tex, (unsigned long long) pl.slots);
    }
    return 0;
}
