// launch_plan_table.cpp with two more things, for tests/test_camera_hits_host.py: Job::first_sample as one more input, and kind 5,
// the camera hits of rt_camera_hits (n list entries, spp = n_samples per entry, first_sample = sample_first).  One line in, one out:
//   plan  kind lds_total lds32_total n_nodes n_obj has_tex  block chunk bpc yield refill passes park  count log  n_rows max_w spp n  cu_count per_cu  first_sample
// kind: 0 frame shard, 1 traceRays list, 2 hitObject list, 3 footprint list, 4 pixel list, 5 camera hits.  The line printed is
// launch_plan_table.cpp's, key for key, so that the other kinds can be held against tests/golden/launch_plans.json word for word.
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
        std::cin >> count >> log >> job.n_rows >> job.max_w >> job.spp >> job.n >> cu >> perCu >> job.first_sample;
        if (!std::cin) return 2;
        sc.tex = tex != 0;
        if (kind < 0 || kind > 5) return 2;
        const rtp::Job::Kind kinds[6] = {rtp::Job::FRAME, rtp::Job::TRACE, rtp::Job::HIT, rtp::Job::FOOTPRINTS, rtp::Job::PIXELS, rtp::Job::CAMERA_HITS};
        job.kind = kinds[kind];
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
        printf("\n");
    }
    return 0;
}
