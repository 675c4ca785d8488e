// camera_hits_plan_table.cpp with one more input and one more kind, for tests/test_camera_hits_views_plan.py: Job::n_views, and kind 7,
// the camera hits of ONE list over a batch of views (rt_camera_hits_views: n list entries, spp = n_samples per entry, n_views views).
// One line in, one out:
//   plan  kind lds_total lds32_total n_nodes n_obj has_tex  block chunk bpc yield refill passes park  count log  n_rows max_w spp n  cu_count per_cu  first_sample n_views
// kind: 0 frame shard, 1 traceRays list, 2 hitObject list, 3 footprint list, 4 pixel list, 5 camera hits, 6 batch of views, 7 camera hits
// over a batch of views (the planner's CAMERA_HITS job with n_views >= 1).  The line printed is launch_plan_table.cpp's, key for key, so that the other kinds can be held against
// tests/golden/launch_plans.json word for word; kind 7 adds units= (the job's units at the launch's chunk) and views= (the kernels with a
// symbol of their own are asked for).
#include "../../ray-tracing-fsharp_amd/csrc/rt_launch_plan.h"

#include <cstdio>
#include <iostream>
#include <string>

static void print_pass(const char *nm, const rtp::Pass &q) {
    printf(" %s_mode=%d %s_grid=%llu %s_lds_bytes=%llu %s_chunk=%d %s_park=%d %s_park_l=%d %s_park_l_lds=%d %s_lds_node_bytes=%d %s_lds_node_thr=%d"
           " %s_yield=%d %s_leaf_wait=%d %s_refill=%d %s_k=%d %s_total_waves=%u",
           nm, q.mode, nm, (unsigned long long) q.grid, nm, (unsigned long long) q.lds_bytes, nm, q.chunk, nm, q.park, nm, q.park_l, nm, q.park_l_lds,
           nm, q.lds_node_bytes, nm, q.lds_node_thr, nm, q.yield_lanes, nm, q.leaf_wait, nm, q.refill_lanes, nm, q.k, nm, q.total_waves);
}

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what != "plan") return 2;
        rtp::Settings s{};
        rtp::SceneSize sc;
        rtp::Job job;
        int kind = 0, tex = 0, count = 0, log = 0, cu = 0, perCu = 0;
        std::cin >> kind >> sc.lds_total >> sc.lds32_total >> sc.n_nodes >> sc.n_objects >> tex;
        std::cin >> s.block >> s.chunk >> s.blocks_per_cu >> s.yield >> s.refill >> s.passes >> s.park;
        std::cin >> count >> log >> job.n_rows >> job.max_w >> job.spp >> job.n >> cu >> perCu >> job.first_sample >> job.n_views;
        if (!std::cin) return 2;
        sc.tex = tex != 0;
        if (kind < 0 || kind > 7) return 2;
        const rtp::Job::Kind kinds[8] = {rtp::Job::FRAME, rtp::Job::TRACE, rtp::Job::HIT, rtp::Job::FOOTPRINTS, rtp::Job::PIXELS, rtp::Job::CAMERA_HITS,
                                         rtp::Job::VIEWS, rtp::Job::CAMERA_HITS};
        job.kind = kinds[kind];
        if (kind == 5) job.n_views = 0; // (rt_camera_hits: no batch)
        if (kind == 7 && job.n_views == 0) return 2;
        job.ray_log = log != 0;
        rtp::LaunchPlan pl = rtp::plan_begin(sc, s, count != 0, job, cu);
        const rtp::Pass first = pl.one; // what the occupancy is asked for
        rtp::plan_finish(pl, perCu);
        printf("q_lds=%d q_count=%d q_block=%d q_mode=%d q_tex=%d q_lds_bytes=%llu two_pass=%d pairs=%llu list=%llu sort=%llu pool=%llu waves=%llu error=%d",
               (int) first.lds, (int) first.count, first.block, first.mode, (int) first.tex, (unsigned long long) first.lds_bytes, (int) pl.two_pass,
               (unsigned long long) pl.pairs_bytes, (unsigned long long) pl.list_bytes, (unsigned long long) pl.sort_bytes,
               (unsigned long long) pl.pool_bytes, (unsigned long long) pl.waves, pl.error ? 1 : 0);
        if (!pl.two_pass) print_pass("F", pl.one);
        else if (!pl.error) { print_pass("A", pl.a); print_pass("B", pl.b); }
        if (kind == 7) printf(" units=%llu views=%d", (unsigned long long) job.unit_count(pl.one.chunk), (int) pl.one.views);
        printf("\n");
    }
    return 0;
}
