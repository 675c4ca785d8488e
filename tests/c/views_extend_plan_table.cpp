// Prints what csrc/rt_launch_plan.h says about the EXTENSION of a batch of views (rt_render_views_extend, rt_render_views_extend_map), for rows
// of plain integers read from standard input; tests/test_views_extend_host.py checks the lines.  One line in, one line out:
//   plan kind lds_total lds32_total n_nodes n_obj has_tex  block chunk bpc yield refill passes park  count  n_views n_rows max_w spp  cu_count per_cu
//        first_sample map
//        kind: 0 a frame shard of n_views * n_rows rows, 6 a batch of n_views views of n_rows rows -- views_plan_table.cpp's line plus the
//        extension's two words; the output is views_plan_table.cpp's, with pass A printed as it is planned (all zero for an extension)
#include "../../ray-tracing-fsharp_amd/csrc/rt_launch_plan.h"

#include <cstdio>
#include <iostream>
#include <string>

static void print_pass(const char *nm, const rtp::Pass &q) {
    printf(" %s_mode=%d %s_grid=%llu %s_lds_bytes=%llu %s_chunk=%d %s_park=%d %s_park_l=%d %s_park_l_lds=%d %s_lds_node_bytes=%d %s_lds_node_thr=%d"
           " %s_yield=%d %s_leaf_wait=%d %s_refill=%d %s_k=%d %s_total_waves=%u %s_views=%d %s_block=%d",
           nm, q.mode, nm, (unsigned long long) q.grid, nm, (unsigned long long) q.lds_bytes, nm, q.chunk, nm, q.park, nm, q.park_l, nm, q.park_l_lds,
           nm, q.lds_node_bytes, nm, q.lds_node_thr, nm, q.yield_lanes, nm, q.leaf_wait, nm, q.refill_lanes, nm, q.k, nm, q.total_waves, nm, (int) q.views,
           nm, q.block);
}

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what != "plan") return 2;
        rtp::Settings s{};
        rtp::SceneSize sc;
        rtp::Job job;
        int kind = 0, tex = 0, count = 0, cu = 0, perCu = 0, map = 0;
        unsigned long long n_views = 0, n_rows = 0;
        std::cin >> kind >> sc.lds_total >> sc.lds32_total >> sc.n_nodes >> sc.n_objects >> tex;
        std::cin >> s.block >> s.chunk >> s.blocks_per_cu >> s.yield >> s.refill >> s.passes >> s.park;
        std::cin >> count >> n_views >> n_rows >> job.max_w >> job.spp >> cu >> perCu;
        std::cin >> job.first_sample >> map;
        if (!std::cin) return 2;
        sc.tex = tex != 0;
        job.map = map != 0;
        if (kind == 6) { job.kind = rtp::Job::VIEWS; job.n_views = (uint32_t) n_views; job.n_rows = n_rows; }
        else { job.kind = rtp::Job::FRAME; job.n_rows = n_views * n_rows; }
        rtp::LaunchPlan pl = rtp::plan_begin(sc, s, count != 0, job, cu);
        const rtp::Pass first = pl.one; // what the occupancy is asked for
        rtp::plan_finish(pl, perCu);
        printf("q_lds=%d q_count=%d q_block=%d q_mode=%d q_tex=%d q_lds_bytes=%llu two_pass=%d pairs=%llu list=%llu sort=%llu pool=%llu waves=%llu pixels=%llu error=%d extend=%d",
               (int) first.lds, (int) first.count, first.block, first.mode, (int) first.tex, (unsigned long long) first.lds_bytes, (int) pl.two_pass,
               (unsigned long long) pl.pairs_bytes, (unsigned long long) pl.list_bytes, (unsigned long long) pl.sort_bytes,
               (unsigned long long) pl.pool_bytes, (unsigned long long) pl.waves, (unsigned long long) pl.pixels, pl.error ? 1 : 0, (int) pl.job.extend());
        if (!pl.two_pass) print_pass("F", pl.one);
        else if (!pl.error) { print_pass("A", pl.a); print_pass("B", pl.b); }
        printf("\n");
    }
    return 0;
}
