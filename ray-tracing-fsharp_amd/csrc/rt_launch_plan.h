// rt_launch_plan.h -- the launch plan: ONE place decides block size, unit sizes, LDS residency, the number of passes, the grids and
// the workspace sizes.  rtfs_amd.hip's enqueue path launches what the plan lists, rt_scene_get_info reports from it, so the two
// cannot disagree -- and because it is plain C++17 over plain integers (no HIP, no scene, no device) tests/test_launch_plan.py runs
// it on a CPU against the decisions recorded from the device.
//
// Two steps, because one device answer sits in the middle of the decisions:
//   plan_begin   kernel choice, block, unit size and dynamic LDS bytes of the FUSED kernel (or of the ray-list kernel);
//   (the caller asks hipOccupancyMaxActiveBlocksPerMultiprocessor for exactly that kernel, block and LDS size -- once)
//   plan_finish  the grids, fused or two passes, pass A's and pass B's placement, the workspace sizes.
// Both passes of a two-pass launch use the grid the FUSED kernel's occupancy gives: kept as measured, not queried per pass.
#pragma once
#include "rt_launch_consts.h"
#include "rt_modes.h"
#include "rt_views_plan.h"

#include <cstddef>
#include <cstdint>

namespace rtp {

// The resolved launch settings (rt_render_options over the rt_set_* defaults); 0 = "the plan decides".
struct Settings { int block, chunk, blocks_per_cu, yield, refill, passes, park; };
static inline const char *check_settings(const Settings &s) {
    if (s.block != 0 && s.block != 256 && s.block != 512 && s.block != 768 && s.block != 1024) return "block_threads must be 0, 256, 512, 768 or 1024";
    if (s.chunk < 0 || s.chunk > RTD_MAX_CHUNK) return "chunk_pixels must be in [0, 64]";
    if (s.blocks_per_cu < 0 || s.blocks_per_cu > 8) return "blocks_per_cu must be in [0, 8]";
    if (s.yield < 0 || s.yield > 64 || s.refill < 0 || s.refill > 64) return "thresholds must be in [0, 64]";
    if (s.passes < 0 || s.passes > 2) return "passes must be 0 (auto), 1 (fused) or 2 (two-pass)";
    if (s.park < -1 || s.park > RTD_MAX_PARK) return "park_lanes must be in [-1, 256]";
    return nullptr;
}

// What the plan needs to know of a scene (rth::HostScene: off.lds_total, off.lds32_total, off.n_nodes, nBounded + nUnbounded, texRecs)
struct SceneSize {
    uint64_t lds_total = 0, lds32_total = 0; // LDS part of the image: exact records (counting variant) / single-precision filter records (timed)
    int32_t n_nodes = 0;                     // records of the depth-ordered node32 section
    uint64_t n_objects = 0;
    bool tex = false;                        // has parameterised textures
    bool prog = false;                       // ... at least one of them a texture program (RT_TEXTURE_PROGRAM): the kernels with that arm run
};
// A frame shard (rtmode::FRAME_* [0..3, 9]), a caller's ray list (RAYS_TRACE [4] paths, RAYS_HIT [5] hit queries) or a caller's footprint
// list (FOOTPRINTS_* [6..8, 10]: planned as a FRAME of n pixels -- chunk widening, fused or two passes, placement, pools -- run by the
// footprint kernels) or a caller's list of a frame's pixels (PIXELS_* [11..13], rt_render_pixels: planned exactly as the FOOTPRINTS job of
// the same n) or the camera hits of such a list (CAMERA_HITS [14], rt_camera_hits: n entries x spp samples, planned by the ray lists' rules
// over n * spp rays, with units of chunk ENTRIES and the wave scratch their pix and candidate words need) or a batch of views
// (rt_render_views: n_views frames of n_rows x (2 max_w + 1) pixels, planned by the pixel rules as ONE frame of as many pixels and run by
// render_views_kernel at blocks of 256 or 1024 threads, with the units of rt_views_plan.h -- none spans two views) or the camera hits of ONE
// list for a batch of views (CAMERA_HITS with n_views >= 1, rt_camera_hits_views: planned by CAMERA_HITS' rules over n_views * n * spp rays and
// run by camera_hits_views_kernel, with rt_views_plan.h's units over the list's n entries -- n_views * ceil(n / chunk) of them.  Not a
// member of Kind: tests/test_views_host.py pins the enumeration's text; rt_dev_last_launch_plan reports such a job as kind 7)
struct Job {
    enum Kind { FRAME, TRACE, HIT, FOOTPRINTS, PIXELS, CAMERA_HITS, VIEWS } kind = FRAME;
    uint64_t n_rows = 0; int32_t max_w = 0, spp = 1; // FRAME; VIEWS: one view's
    uint32_t n_views = 0;                            // VIEWS; CAMERA_HITS: 0 = rt_camera_hits, >= 1 = the views of rt_camera_hits_views
    bool ray_log = false;                            // FRAME: rt_scene_tune's probe
    uint64_t n = 0;                                  // TRACE, HIT: rays; FOOTPRINTS, PIXELS: pixels (with spp); CAMERA_HITS: list entries (spp: n_samples)
    int32_t first_sample = 0;                        // FRAME, FOOTPRINTS, PIXELS, VIEWS: 0 = a fresh render; >= RTD_EXTEND_MIN_DONE: an EXTENSION of a buffer that
                                                     // holds this many samples per continued pixel, to spp (rt_render_extend): pass B alone
                                                     // CAMERA_HITS: sample_first, any value >= 0 (nothing is extended)
    bool map = false;                                // an extension BY MAP (rt_render_extend_map): every pixel from its own Count to its own target <= spp.
                                                     // Planned as the extension RTD_EXTEND_MIN_DONE -> spp (first_sample is that) with the map variant's scratch
    bool camera_hits_views() const { return kind == CAMERA_HITS && n_views != 0; } // camera hits over a batch of views
    bool extend() const { return kind != CAMERA_HITS && first_sample != 0; }
    uint64_t ray_count() const { // TRACE, HIT, CAMERA_HITS: what the grid is sized by
        return kind == CAMERA_HITS ? (uint64_t) (n_views ? n_views : 1u) * n * (uint64_t) spp : n;
    }
    bool list() const { return kind == FOOTPRINTS || kind == PIXELS; }  // n pixels in list order: a frame of one row to the plan
    bool views() const { return kind == VIEWS; }
    bool pixels() const { return kind == FRAME || kind == VIEWS || list(); } // planned by the pixel rules, not the ray lists'
    uint64_t view_pixels() const { return n_rows * (uint64_t) (2 * max_w + 1); }
    uint64_t pixel_count() const { return list() ? n : kind == VIEWS ? (uint64_t) n_views * view_pixels() : view_pixels(); }
    // the units of `chunk` pixels that the fused kernel or pass A hands out
    uint64_t unit_count(int chunk) const {
        if (kind == VIEWS) return rtviews::units_of(rtviews::Plan{(uint32_t) view_pixels(), (uint32_t) chunk, n_views});
        if (camera_hits_views()) return rtviews::units_of(rtviews::Plan{(uint32_t) n, (uint32_t) chunk, n_views}); // (units of list ENTRIES)
        return (pixel_count() + (uint64_t) chunk - 1) / (uint64_t) chunk;
    }
    rtmode::Pixels source() const { // where the job's kernels find their pixels
        return (kind == FRAME || kind == VIEWS) ? rtmode::Pixels::FRAME : kind == FOOTPRINTS ? rtmode::Pixels::FOOTPRINTS : (kind == PIXELS || kind == CAMERA_HITS) ? rtmode::Pixels::LIST : rtmode::Pixels::NONE;
    }
};

// One kernel launch: which render_kernel<lds, count, block, mode, tex> (mode: an rtmode::Mode), its grid and dynamic LDS, and the RenderParams fields the
// plan owns.
struct Pass {
    bool lds = false, count = false, tex = false;
    bool prog = false; // tex, and the scene holds a texture program: render_prog_kernel (rtmode::is_built_prog: blocks of 256 and 1024 only)
    bool views = false; // a batch of views: render_views_kernel<lds, count, block, mode, tex> (a frame pass; blocks of 256 and 1024 only), or,
                        // with mode CAMERA_HITS, camera_hits_views_kernel<lds, count, block>
    int block = 1024, mode = rtmode::FRAME_FUSED;
    uint64_t grid = 0;
    size_t lds_bytes = 0;
    int32_t chunk = 16, park = 0, park_l = 0, park_l_lds = 0, lds_node_bytes = 0, lds_node_thr = 0;
    int32_t yield_lanes = 0, leaf_wait = 0, refill_lanes = 0, k = 0;
    uint32_t total_waves = 0;
};
struct LaunchPlan {
    SceneSize scene; Settings set{}; Job job; int cu_count = 0; // (the inputs, kept for plan_finish)
    bool two_pass = false;
    Pass one;  // the fused kernel or the ray-list kernel; with two_pass only its (kernel, block, lds_bytes) were used, for the occupancy
    Pass a, b; // two_pass: pass A and pass B of the job's pixels (rtmode::Pass::A, ::B); the three sort kernels run between them
               // (an extension: two_pass with pass B only -- a.grid = 0, its list comes from the list-building kernel, unordered; a batch's
               // extension, rt_render_views_extend*: from the batch's list builder and the batch's ordering, by view)
    size_t pairs_bytes = 0, list_bytes = 0, sort_bytes = 0, pool_bytes = 0; // workspace sections behind the launch's scratch, in this order
    uint64_t pixels = 0, waves = 0;                                         // what the statistics report
    const char *error = nullptr; // plan_finish: the launch cannot be made (reported as RT_ERR_HIP, after the scratch was allocated: as before)
};

// `count`: the counting kernel variant stages the exact double-precision node records (112 B), the timed one the single-precision
// filter records (64 B).  wave_words: a wave's LDS scratch, rtmode::wave_words(mode, chunk); ray lists use none.
static inline size_t lds_need(const SceneSize &sc, bool lds, bool count, int block, uint32_t wave_words) {
    return (lds ? (size_t) (count ? sc.lds_total : sc.lds32_total) : 0u) + (size_t) (block / 64) * wave_words * 4u;
}
// The Lambert pool in LDS: as many 56-byte entries per wave as fit beside the scene and the waves' scratch, at most 64; with room
// for fewer than 32 the pool stays in global memory (entries of RTD_PARK_ENTRY_BYTES, L2-resident at best).  Returns the capacity
// and adds the pools' bytes to ldsBytes.
static inline int lambert_pool_lds(size_t &ldsBytes, int block) {
#ifdef RTD_NO_LDS_POOL
    return 0;
#endif
    if (ldsBytes >= RT_LDS_BYTES) return 0;
    const size_t waves = (size_t) block / 64u;
    size_t c = (RT_LDS_BYTES - ldsBytes) / (waves * RTD_PARK_L_LDS_BYTES);
    if (c > 64) c = 64;
    c &= ~(size_t) 1; // an even capacity keeps every field array 16-byte aligned
    if (c < 32) return 0;
    ldsBytes += waves * RTD_PARK_L_LDS_BYTES * c;
    return (int) c;
}
// The timed variant of a scene that is NOT LDS-resident keeps the first records of its depth-ordered node32 section in LDS
// (stage_nodes32, node_loop_glb32): what fits beside the waves' scratch (`ldsBytes` on entry) and a full Lambert pool.  Returns
// the bytes (a multiple of the record size; 0 for the counting variant, whose walk reads the exact records) and adds them.
static inline uint32_t hybrid_node_bytes(const SceneSize &sc, size_t &ldsBytes, bool lds, bool count, int block, bool pool) {
#ifdef RTD_NO_HYBRID
    return 0u;
#endif
    if (lds || count) return 0u;
    const size_t poolBytes = pool ? (size_t) (block / 64) * RTD_PARK_L_LDS_BYTES * 64u : 0u; // (a pool of 48 measured the same, of 32 2 % slower)
    if (ldsBytes + poolBytes + RTD_NODE32_BYTES > RT_LDS_BYTES) return 0u;
    size_t room = (RT_LDS_BYTES - ldsBytes - poolBytes) & ~(size_t) (RTD_NODE32_BYTES - 1);
    const size_t all = (size_t) sc.n_nodes * RTD_NODE32_BYTES;
    if (room > all) room = all;
    ldsBytes += room;
    return (uint32_t) room;
}
// Places one pass in LDS -- the scene image (if resident) and the waves' scratch (its mode's, at its unit size), then the top of the filter tree (hybrid), then the
// Lambert pool if at least 32 entries fit -- and fills the fields that follow from it.  The Lambert pool rides with the general one
// ("never park", park = 0, switches both off); where it does not fit the LDS it keeps its default size in global memory.
static inline void place_pass(Pass &q, const SceneSize &sc) {
    size_t bytes = lds_need(sc, q.lds, q.count, q.block, rtmode::wave_words(q.mode, (uint32_t) q.chunk));
    q.lds_node_bytes = (int32_t) hybrid_node_bytes(sc, bytes, q.lds, q.count, q.block, q.park > 0);
    q.lds_node_thr = RTD_HYBRID_LANES;
    q.park_l = q.park > 0 ? RTD_PARK_L_DEFAULT : 0;
    q.park_l_lds = 0;
    if (q.park > 0)
        if (const int c = lambert_pool_lds(bytes, q.block)) { q.park_l = c; q.park_l_lds = 1; }
    q.lds_bytes = bytes;
}

static inline int default_block(const Settings &s) { return s.block ? s.block : 1024; }
// Residency of a scene: LDS-resident if its image fits beside the waves' scratch at the preferred block and unit size, else the
// global-memory variant of the kernel at the same block (whose timed form keeps the top of the tree in LDS: hybrid_node_bytes; the
// waves' scratch alone always fits).
// (Until round 3 a scene that fitted only beside the scratch of a 256-thread block was kept resident with such blocks: one wave
// per SIMD -- 899 spheres, tuned: 25.1 ms against 12.3 ms for the global-memory variant at 1024 threads.)
// (an LDS-resident scene has far fewer than the 16384 objects the node loop's 14-bit queue entries can name: 48 B each of 160 KiB)
static inline bool lds_resident(const SceneSize &sc, const Settings &s, bool count) {
    return sc.n_objects < 16384u && lds_need(sc, true, count, default_block(s), rtmode::wave_words(rtmode::FRAME_FUSED, s.chunk ? s.chunk : 16)) <= RT_LDS_BYTES;
}

// Step one.  `count`: the counting kernel variant (RT_RENDER_COUNTERS).
static inline LaunchPlan plan_begin(const SceneSize &sc, const Settings &set, bool count, const Job &job, int cu_count) {
    LaunchPlan pl;
    pl.scene = sc; pl.set = set; pl.job = job; pl.cu_count = cu_count;
    Pass &q = pl.one;
    Settings eff = set; // (a footprint list asked to run at 512 or 768 threads runs at 1024: residency is decided at the block that runs)
    if ((job.list() || sc.prog || job.views()) && eff.block != 0 && eff.block != 256) eff.block = 1024; // (a scene with texture programs: likewise, frames included)
    q.lds = lds_resident(sc, eff, count); // (ray lists too: the render's decision, taken at the block the settings ask for)
    q.count = count;
    q.park = set.park < 0 ? 0 : (set.park ? set.park : RTD_PARK_DEFAULT);
    q.yield_lanes = set.yield ? set.yield : RTD_YIELD_DEFAULT;
    // the node loop runs on a little past the point where the STAGE would yield before it hands over to a leaf pass: fewer, fuller
    // leaf passes (measured on the bench frame, yield / hand-over: 52/52 110.9 ms, 52/56 109.9, 50/55 109.5, 48/56 109.5, 50/58 110.4).
    // Never above 64, the lanes of a wave: a hand-over point beyond them is one the node loop cannot reach.
    q.leaf_wait = q.yield_lanes + RTD_LEAF_WAIT_EXTRA > 64 ? 64 : q.yield_lanes + RTD_LEAF_WAIT_EXTRA;
    q.refill_lanes = set.refill ? set.refill : RTD_REFILL_DEFAULT;
    if (!job.pixels()) {
        // 24 instantiations: blocks of 256 or 1024 threads only (a launch asking for 512 or 768 runs at 1024: the block size never
        // changes a result); the hit queries shade nothing, so they have no textured variant and park nothing.
        q.block = default_block(set) == 256 ? 256 : 1024;
        q.mode = rtmode::mode_of({job.source(), job.kind == Job::CAMERA_HITS ? rtmode::Pass::CAMERA_HITS : rtmode::Pass::RAY_LIST, false, false, job.kind != Job::TRACE});
        q.tex = job.kind == Job::TRACE && sc.tex;
        q.prog = q.tex && sc.prog;
        q.chunk = set.chunk ? set.chunk : RTD_MAX_CHUNK; // rays per run of the queue (a wave takes as many runs at once as it has idle lanes)
        if (job.kind != Job::TRACE) q.park = 0;
        q.views = job.camera_hits_views();
        if (job.kind == Job::CAMERA_HITS) {
            // a unit is chunk list ENTRIES, each spp items: about a wave's worth of items per unit unless the caller says otherwise (a
            // unit is set up once and handed out without draining, so small units cost one atomic each and balance the waves best)
            if (!set.chunk) q.chunk = job.spp >= RTD_MAX_CHUNK ? 1 : (RTD_MAX_CHUNK + job.spp - 1) / job.spp;
            // (6 P words are fewer than the 18 P residency was decided with, at the caller's chunk or at 16; a wider default gives way)
            while (q.lds && q.chunk > 1 && lds_need(sc, true, count, q.block, rtmode::wave_words(q.mode, q.chunk)) > RT_LDS_BYTES) q.chunk /= 2;
        }
        place_pass(q, sc); // (the ray lists: no per-wave scratch)
        return pl;
    }
    q.block = default_block(set);
    // (the ray log of rt_scene_tune's probe: a kernel of its own, of frames only)
    q.mode = rtmode::mode_of({job.source(), rtmode::Pass::FUSED, false, job.ray_log && !job.list()});
    if (!rtmode::built_for_every_block(q.mode)) q.block = q.block == 256 ? 256 : 1024; // (a list: as the ray lists)
    q.views = job.views();
    if (q.views) q.block = q.block == 256 ? 256 : 1024; // (a batch of views: as the lists)
    q.tex = sc.tex;               // otherwise the variant compiled without the texture call: no scratch, no VGPR spills
    q.prog = sc.tex && sc.prog;
    if (q.prog) q.block = q.block == 256 ? 256 : 1024; // (the program variants: as the lists)
    const int half = job.spp / 2;
    q.k = half < 5 ? half : 5; // min 5 (spp / 2), Scene.fs:172
    // Units of the fused kernel: 16 pixels -- except for frames of few samples per pixel (always fused: the two-pass rule needs
    // at least 64 samples in phase 2).  A unit is drained before the next, and one of 16 pixels x 11 samples is three rounds of a wave that
    // then waits for its longest path: as wide as still leaves a wave seven units, the scene in LDS permitting (2401x1601 px:
    // 4 spp 8.5 -> 16.0 Gray/s, 16 spp 12.3 -> 19.6 with 64 pixels; 1201x801: 7.0 -> 9.3, 10.5 -> 12.5 with 32).
    q.chunk = set.chunk ? set.chunk : 16;
    // (an extension is the same job at the target spp with two passes forced: it never widens for "few samples")
    if (!set.chunk && set.passes != 2 && !job.extend() && job.spp <= 74) { // (below the two-pass rule's 64 samples in phase 2)
        const uint64_t px = job.pixel_count(), waves = (uint64_t) cu_count * (uint64_t) (q.block / 64);
        for (int c = 64; c > q.chunk; c /= 2)
            if (px >= 7ull * (uint64_t) c * waves && (!q.lds || lds_need(sc, true, count, q.block, rtmode::wave_words(q.mode, c)) <= RT_LDS_BYTES)) { q.chunk = c; break; }
    }
    place_pass(q, sc);
    return pl;
}

// The global-memory pools of parked paths behind a launch's workspace: general + Lambert (sized even when it lives in LDS) + textured
static inline size_t park_pool_bytes(uint64_t blocks, const Pass &q) {
    return (size_t) blocks * (size_t) (q.block / 64) * (size_t) RTD_PARK_ENTRY_BYTES * (size_t) (q.park + (q.park > 0 ? RTD_PARK_L_DEFAULT : 0) + (q.tex ? q.park : 0));
}

// Step two.  per_cu: what hipOccupancyMaxActiveBlocksPerMultiprocessor answered for (pl.one's kernel, pl.one.block, pl.one.lds_bytes), >= 1.
static inline void plan_finish(LaunchPlan &pl, int per_cu) {
    const SceneSize &sc = pl.scene;
    const Settings &set = pl.set;
    Pass &q = pl.one;
    if (set.blocks_per_cu > 0 && set.blocks_per_cu < per_cu) per_cu = set.blocks_per_cu;
    const uint64_t fullGrid = (uint64_t) pl.cu_count * (uint64_t) per_cu;
    const uint64_t wavesPerBlock = (uint64_t) q.block / 64u;
    if (!pl.job.pixels()) {
        const uint64_t wavesWanted = (pl.job.ray_count() + 63u) / 64u; // a wave's worth of rays each, at least
        const uint64_t needBlocks = (wavesWanted + wavesPerBlock - 1) / wavesPerBlock;
        q.grid = fullGrid > needBlocks ? needBlocks : fullGrid;
        pl.pool_bytes = park_pool_bytes(q.grid, q);
        pl.waves = q.grid * wavesPerBlock;
        return;
    }
    const uint64_t nLocal = pl.job.pixel_count();
    const uint64_t units = (nLocal + (uint64_t) q.chunk - 1) / (uint64_t) q.chunk;
    const uint64_t unitsOne = pl.job.views() ? pl.job.unit_count(q.chunk) : units; // (a batch of views: every view ends with a short unit)
    const uint64_t needBlocks = (unitsOne + wavesPerBlock - 1) / wavesPerBlock;
    q.grid = fullGrid > needBlocks ? needBlocks : fullGrid;
    pl.pixels = nLocal;
    // Few units per wave => the fused kernel ends with most waves waiting for a few long units (a 16-pixel unit on a glass sphere
    // takes tens of ms): render in two passes with the second one ordered longest-job-first.  Many units per wave => the fused
    // kernel's tail is ~2 % and it saves the second launch (break-even measured at ~60 units per wave: config 3 whole, 59 per wave,
    // 221 ms in two passes against 227 ms fused; config 4 whole, 507 per wave, 3.75 s against 3.66 s).  spp <= 2k+1 has no second phase at all, and with few remaining samples
    // per pixel a unit is short, so is the tail, and the second launch costs more than it removes (config 2, 100 spp: fused 3.0 ms,
    // two passes 3.5 ms; config 3's 1/8 shard, 500 spp: 51 ms against 30 ms).
    const bool ext = pl.job.extend(); // pass B alone, from sample first_sample on: planned as this job with two passes forced
    int n2 = pl.job.spp - (ext ? pl.job.first_sample : 2 * q.k + 1);
    if (pl.job.map && n2 < 1) n2 = 1; // (a map with cap == 12 continues nothing, but still classifies every pixel and writes rgb)
    // (a PIXELS job by map, which no entry point makes and the table has no mode for, keeps the plan it always had: the footprints' pass B)
    const rtmode::Pixels srcB = pl.job.map && pl.job.kind == Job::PIXELS ? rtmode::Pixels::FOOTPRINTS : pl.job.source();
    const int modeA = rtmode::mode_of({pl.job.source(), rtmode::Pass::A}), modeB = rtmode::mode_of({srcB, rtmode::Pass::B, pl.job.map});
    const auto wordsB = [&](int c) { return rtmode::wave_words(modeB, (uint32_t) c); }; // pass B's scratch per wave (a map's is larger)
    pl.two_pass = n2 > 0 && nLocal > 0 && nLocal < (1ull << 32) &&
                  (set.passes == 2 || ext || (set.passes == 0 && (n2 >= 128 || (n2 >= 64 && nLocal >= (1ull << 21))) && units < 64ull * fullGrid * wavesPerBlock));
    // (frames of 2 Mpx and more pay for the second launch from ~75 spp: 2401x1601 at 100 spp 23.1 Gray/s fused, 26.9 in two passes; 1201x801: 19.6 / 19.8)
    // (the fused launch sizes its pools by its own grid, the two-pass launch by the full grid: pass B always launches that)
    pl.pool_bytes = park_pool_bytes(pl.two_pass ? fullGrid : q.grid, q);
    pl.waves = (pl.two_pass ? fullGrid : q.grid) * wavesPerBlock;
    if (!pl.two_pass) {
        if (ext && nLocal > 0) pl.error = "an extension needs samples to add and fewer than 2^32 pixels"; // (the entry points refuse both first)
        return;
    }
    // workspace: pairs[nLocal] u64, list[nLocal] u32, hist/offsets/cursor[64] u32 (an extension: the list alone, nothing is sorted)
    // (the extension of a batch of views, rt_render_views_extend*: its list must be ordered by view, so its list builder writes pairs and the
    // batch's ordering runs -- pairs and keys as the batch's fresh render has them)
    pl.pairs_bytes = ext && !pl.job.views() ? 0u : ((size_t) nLocal * 8u + 15u) & ~(size_t) 15u;
    pl.list_bytes = ((size_t) nLocal * 4u + 15u) & ~(size_t) 15u;
    pl.sort_bytes = ext ? 0u : (3u * RTD_COST_BUCKETS * 4u + 15u) & ~(size_t) 15u;
    if (pl.job.views()) // the keys of the batch's ordering (views_sort_*_kernel), then where each view's entries end
        pl.sort_bytes = ((size_t) pl.job.n_views * (rtviews::sort_buckets(pl.job.n_views, RTD_COST_BUCKETS) + 1u) * 4u + 15u) & ~(size_t) 15u;
    // Unit sizes: pass A traces only 2k+1 samples per pixel, so its units are wide (below); pass B's largest unit is about a
    // sixteenth of a wave's share of the shard (measured best: 32 px at 1/2 frame, 16 at 1/4, 8 at 1/8 of config 3),
    // and shrinks towards the end of the cost-ordered list.
    int chunkA = set.chunk ? set.chunk : 64, chunkB = set.chunk ? set.chunk : 4;
    if (!set.chunk) {
        // pass A drains every unit before the next (its last paths run with most lanes idle), so wide units pay -- as long as a
        // wave still gets seven or so of them (measured: whole frame 64 px 5.4 ms, 32 px 6.2, 16 px 8.2; an eighth: 16 px best)
        while (chunkA > 8 && nLocal < 7ull * (uint64_t) chunkA * fullGrid * wavesPerBlock) chunkA /= 2;
        const uint64_t share = nLocal / (fullGrid * wavesPerBlock * 16u);
        while (chunkB < 32 && (uint64_t) chunkB * 3u / 2u <= share) chunkB *= 2; // nearest power of two
    }
    // both passes must fit the LDS beside the scene image, decided BEFORE anything is launched (a misfit found after
    // pass A would leave a half-rendered buffer);
    auto needA = [&](int c) { return lds_need(sc, true, q.count, q.block, rtmode::wave_words(modeA, (uint32_t) c)); };
    while (q.lds && chunkA > 1 && needA(chunkA) > RT_LDS_BYTES) chunkA /= 2;
    while (q.lds && chunkB > 1 && lds_need(sc, true, q.count, q.block, wordsB(chunkB)) > RT_LDS_BYTES) chunkB /= 2;
    if (q.lds && q.park > 0 && !set.chunk) { // ... and not so wide that the Lambert pool no longer fits beside them
        auto pool_fits = [&](int c) { size_t b = needA(c); return lambert_pool_lds(b, q.block) != 0; };
        while (chunkA > 16 && !pool_fits(chunkA) && pool_fits(chunkA / 2)) chunkA /= 2;
    }
    if (q.lds && ((!ext && needA(chunkA) > RT_LDS_BYTES) || lds_need(sc, true, q.count, q.block, wordsB(chunkB)) > RT_LDS_BYTES)) {
        pl.error = "two-pass launch does not fit the LDS";
        return;
    }
    pl.a = pl.b = q;
    pl.a.total_waves = pl.b.total_waves = (uint32_t) (fullGrid * wavesPerBlock);
    pl.a.mode = modeA; pl.a.chunk = chunkA;
    pl.b.mode = modeB; pl.b.chunk = chunkB;
    place_pass(pl.b, sc);
    pl.b.grid = fullGrid;                            // pass B always launches the full grid (its units shrink along the list)
    if (ext) { pl.a = Pass{}; pl.a.chunk = 0; return; } // no pass A: nothing of it is launched or reported
    place_pass(pl.a, sc);
    const uint64_t unitsA = pl.job.unit_count(chunkA);
    const uint64_t gridA = (unitsA + wavesPerBlock - 1) / wavesPerBlock;
    pl.a.grid = gridA > fullGrid ? fullGrid : gridA; // pass A's grid is capped by its own unit count
}

} // namespace rtp
