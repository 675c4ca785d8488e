// rt_paths_plan.h -- the launch plan of the path-record kernel (rt_paths_kernels.h; rt_camera_paths, rt_trace_paths): block, run
// length, LDS bytes, route and grid, decided in ONE place over plain integers.  Plain C++17 (no HIP, no scene, no device), so
// tests/test_paths_host.py runs it on a CPU (tests/c/paths_plan_table.cpp); rtfs_amd.hip launches what it lists and
// rt_dev_last_paths_plan reports it.  Two steps, as rt_launch_plan.h's, because one device answer -- the kernel's occupancy at the
// plan's block and LDS size -- sits between them.
#pragma once
#include "rt_launch_plan.h"

namespace rtpp {

#define RTPP_CHUNK_DEFAULT 64 /* slots per run of the queue */

struct PathsPlan {
    // plan_begin
    int block = 1024;       // 256 or 1024 (a block of 512 or 768 threads runs as 1024: the two sizes that are built)
    int chunk = RTPP_CHUNK_DEFAULT; // consecutive slots a wave takes per run
    bool lds = false;       // the route: the scene staged into LDS and walked by the filter loop (timed variant, LDS-resident scene)
    bool count = false;     // the counting variant: always over the exact records in global memory
    bool tex = false;       // the scene has parameterised textures
    bool prog = false;      // ... one of them a texture program: paths_prog_kernel
    size_t lds_bytes = 0;   // dynamic LDS: the timed image of the scene, or nothing (a wave keeps no scratch in LDS)
    bool lds_resident = false; // the render's own answer for this scene and these settings, whichever route runs
    uint64_t slots = 0;
    int blocks_per_cu = 0;  // the caller's cap (0: none)
    // plan_finish
    uint64_t grid = 0;
};

// `set`: the resolved rt_render_options (checked by rtp::check_settings).  yield, refill, passes and park are not used.
// allow_lds = false: the global-memory route whatever the scene (a measurement's switch: scripts/paths_measure.py).
static inline PathsPlan plan_begin(const rtp::SceneSize &sc, const rtp::Settings &set, bool count, uint64_t slots, bool allow_lds = true) {
    PathsPlan pl;
    pl.block = set.block == 256 ? 256 : 1024;
    pl.chunk = set.chunk ? set.chunk : RTPP_CHUNK_DEFAULT;
    pl.count = count;
    pl.tex = sc.tex;
    pl.prog = sc.tex && sc.prog;
    pl.lds_resident = rtp::lds_resident(sc, set, false) && sc.lds32_total <= RT_LDS_BYTES; // the render's residency rule (below 16384 objects)
    pl.lds = !count && pl.lds_resident && allow_lds;
    pl.lds_bytes = pl.lds ? (size_t) sc.lds32_total : 0u;
    pl.slots = slots;
    pl.blocks_per_cu = set.blocks_per_cu;
    return pl;
}

// per_cu: hipOccupancyMaxActiveBlocksPerMultiprocessor for the plan's kernel, block and lds_bytes (>= 1).  The grid is persistent:
// as many blocks as the device holds at once (capped by blocks_per_cu), and never more than waves of 64 slots need.
static inline void plan_finish(PathsPlan &pl, int cu_count, int per_cu) {
    int occ = per_cu;
    if (pl.blocks_per_cu > 0 && pl.blocks_per_cu < occ) occ = pl.blocks_per_cu;
    if (occ < 1) occ = 1;
    const uint64_t fit = (uint64_t) (cu_count > 0 ? cu_count : 1) * (uint64_t) occ;
    const uint64_t need = (pl.slots + (uint64_t) pl.block - 1u) / (uint64_t) pl.block;
    pl.grid = need < fit ? need : fit;
}

} // namespace rtpp
