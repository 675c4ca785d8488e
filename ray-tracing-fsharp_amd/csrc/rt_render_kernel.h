// rt_render_kernel.h -- the persistent render megakernel for gfx950.
//
// Takes the role of Scene.render / renderPixel / traceOnce / traceRay (Scene.fs:93-236) for one shard of image rows.
//
// Execution model:
//   * One workgroup per CU-slot, the tree, object geometry and meta words staged ONCE per workgroup into LDS (<= ~146 KiB at 1024
//     threads and 16-pixel units; the material table stays in global memory), then every WAVE is an independent worker pulling
//     work units (runs of pixels) from a global queue, one atomic per unit.
//   * Inside a unit the 64 lanes are path slots in one of four states (idle / walking the tree / walk finished / waiting for
//     the general reflection); stages (refill, general reflection, node loop, leaf tests, shade) run when enough lanes want
//     them -- see Sched.
//   * Adaptive sampling (Scene.fs:172-194): phase 1 traces 2k+1 samples of every pixel, splitting the byte sums after
//     sample k; the wave compares the two integer means per pixel and ballot-compacts the pixels that must continue;
//     phase 2 traces their remaining spp-2k-1 samples -- either right away on the same wave (fused mode) or in a second
//     launch over the surviving pixels ordered longest-job-first (two-pass mode, for small shards) -- see render_kernel.
//   * Per-sample colours are summed with LDS atomics into the wave's own accumulator words; each pixel's PixelStats
//     {Count,SumRed,SumGreen,SumBlue} is written as one 16-byte store per lane (coalesced), plus the mean RGB.
//   No cross-workgroup communication exists inside a launch, so no fences are needed; queues and counters are relaxed
//   device atomics, and pass B only reads what the stream-ordered earlier launches wrote.
#pragma once
#include "rt_device.h"
#include "rt_extend_map.h"
#include "rt_job_plan.h"
#include "rt_modes.h"
#include "rt_views_plan.h"

#include <type_traits>

namespace rtd {

struct RenderParams {
    const CameraParams *cam_ptr;   // device copy of the camera: read where a camera ray is built, not held in SGPRs
    int32_t depth;                 // Camera.BounceDepth
    int32_t spp;                   // Camera.SamplesPerPixel
    int32_t max_w, max_h;
    SceneOffsets off;
    const unsigned char *scene_image; // global copy of the image described by `off`
    const TexRec *tex;
    const uint8_t *texels;
    uint64_t seed_key;
    int32_t cols;                  // 2*max_w+1
    int32_t row_first, row_stride; // image rows of this shard: row_first + i*row_stride
    int32_t n_rows;
    int32_t k;                     // firstTrial = min 5 (spp/2)   (Scene.fs:172)
    int32_t chunk;                 // pixels per work unit, <= 64
    int32_t leaf_wait;             // the node loop hands over to a leaf pass once this many lanes wait (>= yield_lanes, or a walk stage could spin)
    int32_t yield_lanes;           // see Sched: a stage yields once this many lanes wait for another stage
    int32_t refill_lanes;          // see Sched: idle lanes are refilled once this many are idle
    int32_t park;                  // entries of a wave's park pool (0: rare styles are shaded in place)
    int32_t park_l;                // entries of a wave's pool of parked LAMBERT hits (0: they are shaded where they fall)
    int32_t park_l_lds;            // 1: that pool lives in the workgroup's LDS (56-byte entries behind the waves' scratch), 0: in park_pool
    int32_t lds_node_bytes;        // LDS=false timed kernels ("hybrid"): bytes of the node32 section's first part held at the START of the LDS
    int32_t lds_node_thr;          // ... and how many lanes at those records make a trip of their own (node_loop_glb32; 1..65)
    int32_t *accum;                // [n_rows*cols][4]
    uint8_t *rgb;                  // [n_rows*cols][3] or null
    unsigned long long *counters;  // [16]: rays, aabb, prim, refl, samples, pixels_early, -, -, then stage executions (COUNT):
                                   //       [8] refill [9] node trips [10] leaf stages [11] shade stages [12] lanes refilled [13] lanes shaded
                                   //       and, 160 bytes in, [0] slow stages [1] lanes in them [2] lanes parked
    unsigned int *queue;           // work-unit counter of the fused kernel / of pass A, zeroed before launch
    unsigned char *park_pool;      // [waves of the grid][RTD_PARK_ENTRY_BYTES * (park + (park_l_lds ? 0 : park_l))]: per-wave pools of parked paths (see Sched)
    // two-pass rendering (see render_kernel): pass A appends (cost << 32 | local pixel) for every pixel that continues;
    // pass B walks `live_list` (those pixels ordered by decreasing cost) with its own queue
    unsigned long long *pairs;
    const unsigned int *live_list;
    unsigned int *live_count;      // number of pairs / list entries (device side)
    unsigned long long *queue_b;   // next unassigned list entry
    uint32_t total_waves;          // waves of the grid (guided unit sizes in pass B)
    int32_t first_b;               // pass B's first sample; 0: 2k+1 (after pass A).  An extension (rt_render_extend) passes samples_done:
                                   // the list is then extend_list_kernel's, and `accum` holds samples 0 .. first_b-1 of its pixels
    // rt_scene_tune's probe: every ray whose stream-state hash has `ray_log_mask` clear is appended
    double *ray_log;               // [ray_log_cap][6]: origin, direction; null outside a probe
    unsigned int *ray_log_count;   // rays that wanted a slot (may exceed the capacity: the probe is then repeated more thinly)
    uint32_t ray_log_cap, ray_log_mask;
    // the ray-list modes (rtmode::RAYS_TRACE [4] / RAYS_HIT [5], run_rays; rt_trace_rays / rt_hit_objects): read only there -- and, `rays` and
    // `ray_base`, in the footprint modes (FOOTPRINTS_* [6, 7, 8, 10]), where the pixels are cols = n, n_rows = 1, row_first = 0, row_stride = 1
    const double *rays;            // [ray_n][6]: origin, vector (Ray.make' is applied on the device); footprints: [n][12] origin, base, du, dv
    uint32_t *ray_rng;             // [ray_n][4]: xorshift128 states, read and written back; null: stream (seed, ray_base + i, ray_sample)
    uint8_t *ray_colour;           // [ray_n][3] (RAYS_TRACE)
    int32_t *ray_hit;              // [ray_n] (RAYS_HIT): index into rt_scene_create's array, -1 none, -2 Ray.make' failed
    double *ray_strike;            // [ray_n][3] or null (RAYS_HIT)
    const int32_t *obj_to_orig;    // object-table index -> index into rt_scene_create's array (RAYS_HIT)
    uint64_t ray_n, ray_base;      // (footprints: ray_base is stream_base)
    uint32_t ray_sample;
    // an extension by map (FRAME_PASS_B_MAP [9] / FOOTPRINTS_PASS_B_MAP [10], rt_render_extend_map): read only there and by its list builder
    const int32_t *ext_targets;    // [n_rows*cols]: the Count each pixel is to reach (the classes: extend_map_list_kernel)
    // a pixel list (PIXELS_* [11, 12, 13], rt_render_pixels): read only there.  The list's length is ray_n; cols, max_w, max_h and the camera are
    // the FRAME's, n_rows = 1, row_first = 0, row_stride = 1
    const int32_t *pixel_list;     // [ray_n]: global pixel indices r * cols + c of the frame; entry i owns accum[i] and rgb[i]
    // camera hits (CAMERA_HITS [14], rt_camera_hits): read only there.  ray_n entries, each the frame's pixel pixel_list[i] (null: pixel i); the
    // answers go to ray_hit / ray_strike (as RAYS_HIT's) and cam_rays_out, at slot i * cam_n_samples + (sample - cam_sample_first)
    double *cam_rays_out;          // [ray_n * cam_n_samples][6]: the camera ray itself, origin then unit direction; or null
    int32_t cam_sample_first, cam_n_samples;
    // a batch of views (render_views_kernel, rt_render_views; rt_views_plan.h): read only there.  n_rows, cols, max_w, max_h are ONE view's
    // (row_first = 0, row_stride = 1); accum and rgb hold the batch, view after view; cam_ptr and seed_key are unused -- a unit (a
    // pass-B range) reads the camera and the seed key of ITS view through scalar pointers.  Camera hits over a batch (rt_camera_hits_views)
    // reuse view_cams, view_keys, view_pixels, view_units and n_views beside the camera-hit fields: ray_hit, ray_strike and cam_rays_out
    // hold the batch, view after view
    const CameraParams *view_cams; // [n_views]
    const uint64_t *view_keys;     // [n_views]: seed_key() of each view's seed
    const unsigned int *view_end;  // [n_views] (pass B): the list index at which each view's entries end (views_sort_scan_kernel)
    uint32_t view_pixels;          // pixels of one view: n_rows * cols (camera hits over a batch, camera_hits_views_kernel: the list's entries, = ray_n)
    uint32_t view_units;           // units of one view in the fused kernel / pass A: rtviews::units_per_view at this launch's chunk
    uint32_t n_views, view_pad;
};

// A render job (render_job_kernel, rt_render_job_*; DESIGN.md "Render jobs"): what the stoppable variant of a frame pass reads and
// publishes beside its RenderParams.  `stop` and `progress` are words of the job's control block -- pinned, mapped, coherent host
// memory -- read and written with relaxed system-scope atomics; the kernel POLLS the stop word once per reservation and never waits on
// it.  `done` is the device's own running total of final pixels (agent scope): the mirror may regress when stores race, this cannot.
struct JobCtl {
    const uint32_t *stop;         // host: nonzero = reserve nothing more
    unsigned long long *progress; // host: mirror of *done after this wave's last addition
    unsigned long long *done;     // device: pixels that became final, summed over the job's passes
    long long limit;              // the budget of THIS pass (rt_dev_set_job_limits): units (fused, pass A) or list entries (pass B); < 0: none
};
// lane 0, in front of a reservation: has the host asked the job to stop?
RTD_INLINE bool job_stop_requested(const JobCtl &j) { return __hip_atomic_load(j.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u; }
// lane 0: n more pixels are final
RTD_INLINE void job_publish(const JobCtl &j, uint32_t n) {
    if (n == 0u) return;
    const unsigned long long total = __hip_atomic_fetch_add(j.done, (unsigned long long) n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (unsigned long long) n;
    __hip_atomic_store(j.progress, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Per-wave LDS scratch (in 4-byte words), P = pixels per work unit:
//   acc  [2][P][3]  sums of slot 0 / slot 1
//   pix  [P][4]     row, col, pixel stream key lo, hi
//   live [P]        compacted pixel slots for phase 2 (fused mode), or
//   cost [P]        rays traced for the pixel in phase 1 (pass A: the cost estimate that orders pass B; pass A has no phase 2)
//   cand [P][2]     the leaves the pixel's camera rays can reach, as two queue words (pixel_candidates, rt_device.h), or RTD_CAND_WALK
//   map  [2][P] + [2][P]  pass B of an extension by map only, behind pass B's cand: per slot the first item of each pixel of the range,
//                         then the pixel's next sample less that (run_stream<.., MAP>)
// (rtmode::wave_words(mode, P), rt_modes.h; the values RTD_WAVE_WORDS(P), _A, _MAP, _CAM: rt_launch_consts.h)

// Wave-private LDS words: adds from many lanes may land on one word (same pixel), so they are ds_add_u32; the owner
// lane later takes the sum and clears the word in one ds_wrxchg.  One wave's LDS operations execute in order.
RTD_INLINE void lds_add(RTD_AS3 uint32_t *p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
RTD_INLINE uint32_t lds_take(RTD_AS3 uint32_t *p) { return __hip_atomic_exchange(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

RTD_INLINE uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor((unsigned long long) v, off, 64);
    return v;
}
RTD_INLINE uint32_t lane_rank(unsigned long long mask) { // number of set bits of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
}

// F32: the records are the timed variant's single-precision ones -- in LDS the copy geo | meta | node32 (stage_scene<.., true>), walked
// by node_loop_lds32; in global memory the image's node32 section, whose links are byte offsets from its start (node_loop_glb32)
template <bool LDS, bool F32 = false> RTD_INLINE SceneView<LDS> make_view(const RenderParams &p, const unsigned char *lds_base) {
    SceneView<LDS> v;
    const uint32_t nodeOff = F32 ? p.off.node32 : p.off.node;
    if constexpr (LDS) {
        const RTD_AS3 unsigned char *b = (const RTD_AS3 unsigned char *) lds_base;
        if constexpr (F32) b -= p.off.geo; // the copy starts at the image's `geo` section
        v.node = (Ptrs<true>::bp) (b + nodeOff);
        v.geo = (Ptrs<true>::d2p) (b + p.off.geo);
        v.meta = (Ptrs<true>::i2p) (b + p.off.meta);
    } else {
        const unsigned char *b = p.scene_image;
        v.node = b + nodeOff;
        v.geo = (const d2 *) (b + p.off.geo);
        v.meta = (const i2 *) (b + p.off.meta);
    }
    v.mat = (const double *) (p.scene_image + p.off.mat);
    v.n_nodes = p.off.n_nodes; v.n_bounded = p.off.n_bounded; v.n_unbounded = p.off.n_unbounded;
    if constexpr (LDS) v.first = (int) (uint32_t) (uintptr_t) v.node; // links were made absolute at staging
    else v.first = 0;                                                 // links are byte offsets from v.node
    v.end = v.first + v.n_nodes * (F32 ? RTD_NODE32_BYTES : RTD_NODE_BYTES);
    v.tex = p.tex; v.texels = p.texels; v.lds_lim = 0; v.lds_thr = 65; v.narrow = (v.n_bounded + v.n_unbounded) < 16384 ? 1 : 0;
    return v;
}

struct StageStats { // wave-uniform, COUNT variant only
    uint32_t refill, trips, leaf, shade, refillLanes, shadeLanes, slow, slowLanes, parkedLanes;
    unsigned long long tRefill, tSlow, tWalk, tShade; // shader-clock cycles this wave spent inside each stage (s_memtime)
    unsigned long long loopTrips, loopLanes;            // -DRTD_STAGE_CLOCKS only: trips of the timed variant's node loop, lanes that stepped in them
    unsigned long long tLoop, tLeaf, tUnb, tCam, tLamb; // -DRTD_STAGE_CLOCKS only: node loop / leaf passes (inside tWalk), unbounded tests (inside tShade),
                                                        // new items (inside tRefill), Lambert batches (inside tSlow)
#ifdef RTD_STAGE_CLOCKS
    // the instruction census' execution counts (scripts/instruction_census.py), wave-uniform; they leave through g_census (rt_device.h)
    uint32_t turns, lambBatches, lambLanes, newRefills, newItems, unparkL, unparkA, storeBlocksL, storeLanesL, storeBlocksA,
        lightBatches, lightLanes, missLanes, ranges, flushes, leafLanes, unparkBatchesL, unparkBatchesA, slowLanesByStyle[8], slowBatchesByStyle[8];
#endif
};
#ifdef RTD_STAGE_CLOCKS
#define RTD_CENSUS(S) S
#else
#define RTD_CENSUS(S)
#endif

// Diagnostic builds (-DRTD_STAGE_CLOCKS): the per-stage cycle sums of the counting variant in the timed variant too
#ifdef RTD_STAGE_CLOCKS
#define RTD_CLK true
#else
#define RTD_CLK false
#endif

// ---- the lane scheduler shared by every render mode ------------------------------------------------------------------------
// Every lane of a wave is a path slot in one of four states: IDLE (wants a new item), WALK (somewhere in the tree walk of its
// current ray; the walk state survives while the lane is parked), DONE (tree exhausted: wants the unbounded-object tests and
// Hittable.Reflection), SLOW (its hit needs the general `reflection`: any style but an untextured light source or Lambert sphere).
// Per-ray work is heavy-tailed (tree nodes per ray: mean 24, p99 60, max 150), so running each stage until its slowest lane
// finishes leaves ~70 % of the lanes idle.  Instead a stage runs while enough lanes want it:
//   yield_lanes  the walk stage yields, and the shade stage runs, once this many walks are finished (or none is left walking)
//   leaf_wait    (yield_lanes + RTD_LEAF_WAIT_EXTRA) inside the walk stage the node loop hands over to a leaf pass once this many
//                lanes are waiting -- for a pending leaf test, or finished.  Never below yield_lanes: the stage would spin
//   refill_lanes idle lanes are given new work once this many are idle (or nothing else is runnable)
// The shade stage shades the two common cases where they fall (reflection_fast) -- about 250 instructions.  The other styles'
// code is twice as long and used to run in almost every shade stage for the two or three lanes that needed it; now such a
// path is PARKED: its state (88 bytes) goes to the wave's own pool in global memory (L2-resident: a few KB per wave in use)
// and the lane is free for other work.  When a refill finds at least as many parked paths as idle lanes (or no new items),
// the idle lanes take parked paths instead of new items and run the general `reflection` together.  A pool that is full
// (or switched off, p.park = 0) leaves the path in its lane and the general code runs for it at the next turn of the loop.
// Which lane computes what when has no effect on any result: streams are per item.
enum { L_IDLE = 0, L_WALK = 1, L_DONE = 2, L_SLOW = 3, L_LAMB = 4, L_TEX = 5 };

// LOG: the kernel may be asked to log rays (rt_scene_tune's probe): only the fused mode's instantiations carry that code -- the
// log's four kernel arguments otherwise sit in scalar registers across the whole loop of the two-pass kernels, which have none to spare
// FP: the pixels are the caller's footprints (rtmode::Pixels::FOOTPRINTS): a sample's ray comes from footprint_ray instead of camera_ray
template <bool LDS, bool COUNT, int TEX, bool LOG, bool FP = false>
struct Sched {
    const RenderParams &p;
    const SceneView<LDS> &sc;
    Counters &cnt;
    StageStats &ss;
    unsigned char *pool; // this wave's park pools in global memory: the general one, then (unless it is in LDS) the Lambert one
    RTD_AS3 unsigned char *poolLds; // this wave's Lambert pool in LDS (p.park_l_lds)
    uint32_t parked;     // entries in the general pool (wave-uniform)
    uint32_t parkedL;    // entries in the Lambert pool (wave-uniform)
    uint32_t parkedT;    // entries in the pool of hits whose colour is a parameterised texture (TEX kernels only; wave-uniform)
    const int end;
    // lane state
    int st;
    V3 o, d;
    Walk w;
    Rng rng;
    uint32_t colour, slotOff;
    int bounces;
    uint32_t pend; // queue of pending leaf tests (node_loop_lds32: two 16-bit entries; node_loop_glb32: the older full-width entry); always 0
                   // outside a walk and in the counting variant, which does not queue
    uint32_t texc; // L_SLOW lanes: the hit's texture colour if stage_tex has evaluated one, else RTD_NO_TEX
    // set by the stages for the caller's bookkeeping: this lane's path ended during the current turn, with this colour
    bool ended;
    uint32_t pend1; // node_loop_glb32's newer entry (declared apart from `pend`: as neighbours the two are stored together by one vector
                    // store, and the whole scheduler state then lives in scratch memory)
    uint32_t result;

    RTD_INLINE Sched(const RenderParams &p_, const SceneView<LDS> &sc_, Counters &cnt_, StageStats &ss_, unsigned char *pool_, RTD_AS3 unsigned char *poolLds_)
        : p(p_), sc(sc_), cnt(cnt_), ss(ss_), pool(pool_), poolLds(poolLds_), parked(0u), parkedL(0u), parkedT(0u), end(sc_.end) {
        st = L_IDLE;
        o = mk(0, 0, 0); d = mk(0, 0, 0);
        walk_begin(w, sc.first); w.off = end; // idle lanes are parked at `end`
        rng.x = rng.y = rng.z = rng.w = 0;
        colour = 0; slotOff = 0; bounces = 0; pend = 0u; pend1 = 0u; texc = RTD_NO_TEX;
        ended = false; result = 0;
    }

    // the probe of rt_scene_tune: a thinned-out log of the rays as they start (which rays: a hash of the ray's stream state, so
    // the logged SET does not depend on scheduling; the host sorts it)
    RTD_INLINE void log_ray() {
        if (!LOG) return;
        if (p.ray_log == nullptr) return; // wave-uniform: one scalar compare per ray outside a probe
        if (((((rng.x ^ rng.w) * 0x9E3779B1u) >> 8) & p.ray_log_mask) == 0u) {
            const unsigned int at = atomicAdd(p.ray_log_count, 1u);
            if (at < p.ray_log_cap) {
                double *r = p.ray_log + 6u * (size_t) at;
                r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
            }
        }
    }

    // a new (pixel, sample) item: Scene.traceOnce's ray (Scene.fs:129-150)
    RTD_INLINE bool start_item(uint64_t pkey, uint32_t sample, int row, int col, uint32_t slot_off, uint32_t cand, uint32_t cand2) {
        const unsigned long long k0 = RTD_CLK ? __builtin_amdgcn_s_memtime() : 0ull;
        struct Stamp { StageStats &ss; unsigned long long k0; RTD_INLINE ~Stamp() { if (RTD_CLK) ss.tCam += __builtin_amdgcn_s_memtime() - k0; } } stamp{ss, k0};
        rng = stream_for(pkey, sample);
        slotOff = slot_off;
        colour = RTD_WHITE;
        bounces = 0;
        bool made;
        if constexpr (FP) made = footprint_ray(p.rays + 12u * (size_t) (uint32_t) row, rng, o, d); // `row` is the footprint's list index
        else {
            const CameraParams *cp = p.cam_ptr;
            asm volatile("" : "+s"(cp)); // keep the camera's 32 dwords out of the loop-carried SGPR set
            made = camera_ray(*cp, row, col, rng, o, d);
        }
        if (made) {
            st = L_WALK;
            walk_begin(w, sc.first);
            if (!FP && !COUNT && cand != RTD_CAND_WALK) { // the tree walk of this pixel's camera rays was made once (pixel_candidates)
                w.off = end; pend = cand; pend1 = cand2;
                if (cand == 0u) st = L_DONE; // nothing in reach: straight to the unbounded objects
            }
            if (COUNT) cnt.rays++;
            log_ray();
            return true;
        }
        return false; // Scene.fs:144's ValueOption.get would throw; the sample counts as Black (adds nothing)
    }

    // ---- park pools: entry e of field f sits at base + (f * K + e) * 16 (fields 0-4) / base + 80 * K + e * 8 (field 5), K = the pool's capacity ----
    // (byte offsets are formed in 32 bits -- a wave's pools are a few KB -- so that every access is scalar base + 32-bit lane offset,
    // one add per field, instead of a 64-bit address built per field)
    RTD_INLINE void park_store(unsigned char *base, uint32_t K, uint32_t e) {
        const uint32_t at = e * 16u, kb = K * 16u;
        d2 v;
        v.x = o.x; v.y = o.y; *(d2 *) (base + at) = v;
        v.x = o.z; v.y = d.x; *(d2 *) (base + (kb + at)) = v;
        v.x = d.y; v.y = d.z; *(d2 *) (base + (2u * kb + at)) = v;
        i4 r; r.x = __double2loint(w.bestLen); r.y = __double2hiint(w.bestLen); r.z = (int) colour; r.w = (int) slotOff;
        *(i4 *) (base + (3u * kb + at)) = r;
        r.x = (int) rng.x; r.y = (int) rng.y; r.z = (int) rng.z; r.w = (int) rng.w;
        *(i4 *) (base + (4u * kb + at)) = r;
        i2 b; b.x = bounces; b.y = w.best;
        *(i2 *) (base + (5u * kb + e * 8u)) = b;
    }
    RTD_INLINE void park_load(const unsigned char *base, uint32_t K, uint32_t e, int state) {
        const uint32_t at = e * 16u, kb = K * 16u;
        const d2 a = *(const d2 *) (base + at), b = *(const d2 *) (base + (kb + at)), c = *(const d2 *) (base + (2u * kb + at));
        const i4 t = *(const i4 *) (base + (3u * kb + at)), r = *(const i4 *) (base + (4u * kb + at));
        const i2 bo = *(const i2 *) (base + (5u * kb + e * 8u));
        o = mk(a.x, a.y, b.x); d = mk(b.y, c.x, c.y);
        w.bestLen = __hiloint2double(t.y, t.x); colour = (uint32_t) t.z; slotOff = (uint32_t) t.w;
        rng.x = (uint32_t) r.x; rng.y = (uint32_t) r.y; rng.z = (uint32_t) r.z; rng.w = (uint32_t) r.w;
        bounces = bo.x; w.best = bo.y;
        w.off = end;
        st = state;
    }
    RTD_INLINE unsigned char *pool_l() const { return pool + (size_t) RTD_PARK_ENTRY_BYTES * (size_t) p.park; }
    RTD_INLINE unsigned char *pool_t() const { return pool + (size_t) RTD_PARK_ENTRY_BYTES * (size_t) (p.park + (p.park_l_lds ? 0 : p.park_l)); } // capacity p.park
    // A parked LAMBERT hit is {strike (in o), inside (bit 31 of bounces), colour, rng, slot, bounces, object}: what lambert_bounce needs.
    // In LDS: entry e of field f at base + (f * K + e) * 16 (fields 0-2), base + 48 * K + e * 8 (field 3).
    RTD_INLINE void park_store_lds(uint32_t K, uint32_t e) {
        RTD_AS3 d2 *f = (RTD_AS3 d2 *) poolLds;
        d2 v; v.x = o.x; v.y = o.y; f[e] = v;
        i4 r; r.x = __double2loint(o.z); r.y = __double2hiint(o.z); r.z = (int) colour; r.w = (int) slotOff;
        ((RTD_AS3 i4 *) poolLds)[K + e] = r;
        r.x = (int) rng.x; r.y = (int) rng.y; r.z = (int) rng.z; r.w = (int) rng.w;
        ((RTD_AS3 i4 *) poolLds)[2u * K + e] = r;
        i2 b; b.x = bounces; b.y = w.best;
        ((RTD_AS3 i2 *) (poolLds + 48u * K))[e] = b;
    }
    RTD_INLINE void park_load_lds(uint32_t K, uint32_t e) {
        const d2 a = ((const RTD_AS3 d2 *) poolLds)[e];
        const i4 t = ((const RTD_AS3 i4 *) poolLds)[K + e], r = ((const RTD_AS3 i4 *) poolLds)[2u * K + e];
        const i2 bo = ((const RTD_AS3 i2 *) (poolLds + 48u * K))[e];
        o = mk(a.x, a.y, __hiloint2double(t.y, t.x)); colour = (uint32_t) t.z; slotOff = (uint32_t) t.w;
        rng.x = (uint32_t) r.x; rng.y = (uint32_t) r.y; rng.z = (uint32_t) r.z; rng.w = (uint32_t) r.w;
        bounces = bo.x; w.best = bo.y;
        w.off = end;
        st = L_LAMB;
    }
    // How the `nIdle` idle lanes of a refill are served (wave-uniform): a FULL batch of parked Lambert hits if that pool holds one,
    // else a full batch of parked general hits, else new items; once there are no new items, whatever the pools still hold.
    RTD_INLINE void unpark_plan(uint32_t nIdle, bool haveNew, uint32_t &nUnL, uint32_t &nUnA, uint32_t &nUnT) const {
        nUnL = nUnA = nUnT = 0u;
        if (parkedL >= nIdle) nUnL = nIdle;
        else if (parked >= nIdle) nUnA = nIdle;
        else if (TEX && parkedT >= nIdle) nUnT = nIdle;
        else if (!haveNew) {
            nUnL = parkedL;
            nUnA = parked < nIdle - nUnL ? parked : nIdle - nUnL;
            if (TEX) nUnT = parkedT < nIdle - nUnL - nUnA ? parkedT : nIdle - nUnL - nUnA;
        }
    }
    // the idle lane of rank `rank` takes its parked path, if the plan gives it one
    RTD_INLINE bool unpark_lane(uint32_t rank, uint32_t nUnL, uint32_t nUnA, uint32_t nUnT) {
        // (the three counters are read HERE, unconditionally: read inside the branches, the optimiser merges the loads into one load
        // from a selected address, and the scheduler's state then lives in scratch memory instead of registers)
        const uint32_t topL = parkedL - 1u, topA = parked - 1u, topT = parkedT - 1u;
        if (rank < nUnL) {
            if (p.park_l_lds) park_load_lds((uint32_t) p.park_l, topL - rank);
            else park_load(pool_l(), (uint32_t) p.park_l, topL - rank, L_LAMB);
            return true;
        }
        if (rank < nUnL + nUnA) { park_load(pool, (uint32_t) p.park, topA - (rank - nUnL), L_SLOW); texc = RTD_NO_TEX; return true; }
        if (TEX && rank < nUnL + nUnA + nUnT) { park_load(pool_t(), (uint32_t) p.park, topT - (rank - nUnL - nUnA), L_TEX); return true; }
        return false;
    }

    // what follows Hittable.Reflection in Scene.traceRay (Scene.fs:105-112)
    RTD_INLINE void after_reflection(bool absorbed) {
        bool done = absorbed;
        uint32_t res = colour;
        if (!absorbed) {
            bounces = bounces + 1;
            if (bounces > p.depth) { done = true; res = RTD_HOTPINK; } // Scene.fs:98,114
        }
        if (done) { ended = true; result = res; st = L_IDLE; w.off = end; }
        else {
            st = L_WALK;
            walk_begin(w, sc.first);
            if (COUNT) cnt.rays++;
            log_ray();
        }
    }

    // ---- slow: the general Hittable.Reflection for the lanes whose hit is not one of the two common cases ----
    RTD_INLINE void stage_slow() {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(st == L_SLOW);
        if (m == 0ull) return;
        if (COUNT || RTD_CLK) { ss.slow++; ss.slowLanes += (uint32_t) __popcll(m); }
#ifdef RTD_STAGE_CLOCKS
#pragma unroll
        for (int sty = 0; sty < 8; ++sty) {
            const unsigned long long sm = __builtin_amdgcn_ballot_w64(st == L_SLOW && (int) (((uint32_t) sc.meta[w.best < 0 ? 0 : w.best].x >> 2) & 7u) == sty);
            ss.slowLanesByStyle[sty] += (uint32_t) __popcll(sm); ss.slowBatchesByStyle[sty] += sm != 0ull ? 1u : 0u;
        }
#endif
        if (st == L_SLOW) {
            const V3 strike = walk(o, d, w.bestLen); // Ray.walkAlong ray bestLength (Scene.fs:91)
            after_reflection(reflection<LDS, false>(sc, w.best, strike, o, d, colour, rng, TEX ? texc : RTD_NO_TEX));
        }
    }

    // ---- tex: Texture.colourAt (Texture.fs:50-67) for the lanes that took parked textured hits (or whose hit found that pool full).
    // The evaluation is long (correctly rounded acos / atan2 / sin in double-double, rt_trig.h); here it runs for a batch of lanes
    // at once, inline, and nowhere else in the kernel.  The lane goes on to the general reflection with the colour in `texc`.
    RTD_INLINE void stage_tex() {
        if (!TEX) return;
        if (__builtin_amdgcn_ballot_w64(st == L_TEX) == 0ull) return;
        if (st == L_TEX) {
            const V3 strike = walk(o, d, w.bestLen);
            texc = texture_colour_at_inline<TEX == 2>(sc.tex, sc.texels, textured(sc.meta[w.best]), strike, nullptr);
            st = L_SLOW;
        }
    }

    // ---- lamb: the Lambert bounce (Sphere.fs:202-222) for the lanes that took parked Lambert hits (or whose hit found the pool full) ----
    RTD_INLINE void stage_lamb() {
        if (__builtin_amdgcn_ballot_w64(st == L_LAMB) == 0ull) return;
        RTD_CENSUS(ss.lambBatches++; ss.lambLanes += (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(st == L_LAMB));)
        const unsigned long long k0 = RTD_CLK ? __builtin_amdgcn_s_memtime() : 0ull;
        if (st == L_LAMB) { // o holds the strike point, bit 31 of bounces "the ray came from inside" (stage_shade)
            const bool inside = bounces < 0;
            bounces &= 0x7FFFFFFF;
            lambert_bounce<LDS>(sc, w.best, sc.meta[w.best], o, inside, o, d, colour, rng);
            after_reflection(false);
        }
        if (RTD_CLK) ss.tLamb += __builtin_amdgcn_s_memtime() - k0;
    }

    // ---- walk: BoundingBox.hits over the tree image, leaf tests deferred out of the node loop ----
    // A lane steps iff w.off < end: finished walks sit at >= end, pending leaves carry RTD_LEAF (> end), idle lanes are
    // parked at `end`.  So one compare gives the active set, and waiting = busy - active.
    RTD_INLINE void stage_walk() {
        const unsigned long long walkM0 = __builtin_amdgcn_ballot_w64(st == L_WALK);
        if (walkM0 == 0ull) return;
        const int nBusy = __popcll(__builtin_amdgcn_ballot_w64(st != L_IDLE));
        const int stop = (nBusy - p.leaf_wait) > 0 ? (nBusy - p.leaf_wait) : 0; // active <= stop  <=>  waiting >= leaf_wait
        if constexpr (!COUNT) {
            // the timed variant: the hand-written single-precision filter loop with its queue of pending leaves (rt_device.h) over the
            // LDS copy of the scene, or over global memory for a scene that does not fit; the leaf pass makes the sphere test and,
            // where the hit does not imply it, the leaf's exact box test; a lane is finished when its walk is exhausted AND its
            // queue is empty
            const WalkCtx32 f = walk_ctx32(o, d, p.off.bmax);
            double bestF = (w.best < 0) ? __builtin_inf() : w.bestLen * w.bestLen; // `a = point * point` (Scene.fs:45), recomputed
            const bool implied = p.off.box_implied != 0; // (rays of this kernel are unitised: Ray.make')
            if (RTD_CLK) ss.trips++; // (diagnostic build: walk-stage entries and leaf passes; the loop's trips are not counted)
            // the lanes walking and the lanes finished, as wave masks kept up to date by the lanes that finish in a pass: one select
            // per pass instead of a select and two compares of the new state
            unsigned long long walkM = walkM0, doneM = __builtin_amdgcn_ballot_w64(st == L_DONE);
            for (;;) {
                const unsigned long long k0 = RTD_CLK ? __builtin_amdgcn_s_memtime() : 0ull;
#ifdef RTD_STAGE_CLOCKS
                unsigned nTrips = 0u, nLanes = 0u;
#define RTD_TRIP_PASS , nTrips, nLanes
#else
#define RTD_TRIP_PASS
#endif
                if constexpr (LDS) w.off = node_loop_lds32(w.off, pend, end, stop, f RTD_TRIP_PASS);
                else if (sc.narrow) w.off = node_loop_hyb16(w.off, pend, (const unsigned char *) sc.node, sc.lds_lim, sc.lds_thr, end, stop, f RTD_TRIP_PASS);
                else w.off = node_loop_glb32(w.off, pend, pend1, (const unsigned char *) sc.node, sc.lds_lim, sc.lds_thr, end, stop, f);
#ifdef RTD_STAGE_CLOCKS
                ss.loopTrips += nTrips; ss.loopLanes += nLanes;
#endif
#undef RTD_TRIP_PASS
                const unsigned long long k1 = RTD_CLK ? __builtin_amdgcn_s_memtime() : 0ull;
                if (RTD_CLK && __builtin_amdgcn_ballot_w64(pend != 0u) != 0ull) ss.leaf++;
                RTD_CENSUS(ss.leafLanes += (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(pend != 0u));)
                if (pend != 0u) {
                    int prim;
                    if (LDS || sc.narrow) {
                        prim = pend_pop(pend);
                        if (pend == 0u) { pend = pend1; pend1 = 0u; } // a camera ray's third and fourth candidate (start_item)
                    } else prim = pend_pop_wide(pend, pend1);
                    leaf_test_object_exact<LDS>(sc, o, d, bestF, w, prim, implied);
                }
                if (RTD_CLK) { ss.tLoop += k1 - k0; ss.tLeaf += __builtin_amdgcn_s_memtime() - k1; }
                const bool fin = (st == L_WALK) && (w.off >= end) && pend == 0u;
                if (fin) st = L_DONE;
                // (a ballot per compare, joined as masks: the ballot of a conjunction is first made a 0/1 value per lane and compared again)
                const unsigned long long finM = walkM & __builtin_amdgcn_ballot_w64(w.off >= end) & __builtin_amdgcn_ballot_w64(pend == 0u);
                walkM &= ~finM; doneM |= finM;
                if (walkM == 0ull || __popcll(doneM) >= p.yield_lanes) break;
            }
            return;
        }
        WalkCtx c = walk_ctx(d, w); // cheap to re-derive; keeps 9 doubles out of the parked state
        for (;;) {
            for (;;) {
                const bool act = w.off < end;
                const int nAct = __popcll(__builtin_amdgcn_ballot_w64(act));
                if (nAct <= stop) break;
                if (COUNT) ss.trips++;
                if (act) {
                    if (COUNT) cnt.aabb++;
                    node_step<LDS>(sc, o, c, w);
                }
            }
            if (COUNT && __builtin_amdgcn_ballot_w64((w.off & RTD_LEAF) != 0) != 0ull) ss.leaf++;
            if (w.off & RTD_LEAF) {
                if (COUNT) cnt.prim++;
                leaf_test<LDS>(sc, o, d, c, w);
            }
            const bool fin = (st == L_WALK) && (w.off >= end);
            if (fin) st = L_DONE;
            const int nWalk = __popcll(__builtin_amdgcn_ballot_w64(st == L_WALK));
            const int nDone = __popcll(__builtin_amdgcn_ballot_w64(st == L_DONE));
            if (nWalk == 0 || nDone >= p.yield_lanes) break;
        }
    }

    // ---- shade: the rest of Scene.hitObject (Scene.fs:77-91), then Hittable.Reflection for the common cases; the others park ----
    RTD_INLINE void stage_shade() {
        const unsigned long long dm = __builtin_amdgcn_ballot_w64(st == L_DONE);
        if (dm == 0ull) return;
        if (COUNT || RTD_CLK) { ss.shade++; ss.shadeLanes += (uint32_t) __popcll(dm); }
        if (st == L_DONE) {
            const unsigned long long k0 = RTD_CLK ? __builtin_amdgcn_s_memtime() : 0ull;
            unbounded_tests<LDS, COUNT>(sc, o, d, w, cnt);
            if (RTD_CLK) ss.tUnb += __builtin_amdgcn_s_memtime() - k0;
            RTD_CENSUS(ss.missLanes += (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(w.best < 0));)
            if (w.best < 0) { ended = true; result = RTD_BLACK; st = L_IDLE; w.off = end; } // "never heard from again": Black (Scene.fs:102-104)
            else {
                if (COUNT) cnt.refl++;
                const i2 m = sc.meta[w.best];
                if (fast_style(m)) {
                    if (p.park_l > 0 && (((uint32_t) m.x >> 2) & 7u) != 0u) {
                        // an untextured Lambert sphere: parked as {strike, inside} and bounced in full batches (stage_lamb)
                        const bool inside = lambert_inside<LDS>(sc, w.best, m, o);
                        o = walk(o, d, w.bestLen); // Ray.walkAlong ray bestLength (Scene.fs:91)
                        bounces |= inside ? (int) 0x80000000u : 0;
                        st = L_LAMB;
                    } else {
                        RTD_CENSUS({ const uint32_t nl = (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(true)); ss.lightBatches++; ss.lightLanes += nl; })
                        const V3 strike = walk(o, d, w.bestLen); // Ray.walkAlong ray bestLength (Scene.fs:91)
                        after_reflection(reflection_fast<LDS>(sc, w.best, m, strike, o, d, colour, rng));
                    }
                } else if (TEX && textured(m) >= 0) st = L_TEX;
                else { st = L_SLOW; texc = RTD_NO_TEX; }
            }
        }
        if (TEX && p.park > 0) {
            const unsigned long long tm = __builtin_amdgcn_ballot_w64(st == L_TEX);
            if (tm != 0ull) {
                const uint32_t room = (uint32_t) p.park - parkedT, want = (uint32_t) __popcll(tm);
                const uint32_t rank = lane_rank(tm);
                if (st == L_TEX && rank < room) { park_store(pool_t(), (uint32_t) p.park, parkedT + rank); st = L_IDLE; w.off = end; }
                parkedT += want < room ? want : room;
            }
        }
        if (p.park > 0) {
            const unsigned long long sm = __builtin_amdgcn_ballot_w64(st == L_SLOW);
            if (sm != 0ull) {
                const uint32_t room = (uint32_t) p.park - parked, want = (uint32_t) __popcll(sm);
                const uint32_t rank = lane_rank(sm);
                if (st == L_SLOW && rank < room) { park_store(pool, (uint32_t) p.park, parked + rank); st = L_IDLE; w.off = end; }
                const uint32_t n = want < room ? want : room;
                parked += n;
                if (COUNT || RTD_CLK) ss.parkedLanes += n;
                RTD_CENSUS(ss.storeBlocksA++;)
            }
        }
        if (p.park_l > 0) {
            const unsigned long long lm = __builtin_amdgcn_ballot_w64(st == L_LAMB);
            if (lm != 0ull) {
                const uint32_t room = (uint32_t) p.park_l - parkedL, want = (uint32_t) __popcll(lm);
                const uint32_t rank = lane_rank(lm);
                if (st == L_LAMB && rank < room) {
                    if (p.park_l_lds) park_store_lds((uint32_t) p.park_l, parkedL + rank);
                    else park_store(pool_l(), (uint32_t) p.park_l, parkedL + rank);
                    st = L_IDLE; w.off = end;
                }
                parkedL += want < room ? want : room;
                RTD_CENSUS(ss.storeBlocksL++; ss.storeLanesL += want < room ? want : room;)
            }
        }
    }

    // PixelStats.add (Pixel.fs:97-101) for a lane whose path ended this turn; Count is implied by the item count
    RTD_INLINE void add_result(RTD_AS3 uint32_t *acc3) const {
        if (result != 0u) {
            lds_add(acc3 + 0, result & 0xFFu);
            lds_add(acc3 + 1, (result >> 8) & 0xFFu);
            lds_add(acc3 + 2, (result >> 16) & 0xFFu);
        }
    }
};

// Trace `total` items of the current unit.  Item i belongs to pixel slot map[i / per] (or i / per when map is null)
// and is sample s_base + i % per of that pixel; its colour is added to accumulator slot (sample < split ? 0 : 1).
template <bool LDS, bool COUNT, bool COST, int TEX, bool LOG, bool FP>
RTD_INLINE void run_items(const RenderParams &p, const SceneView<LDS> &sc, unsigned char *pool, RTD_AS3 unsigned char *poolLds, RTD_AS3 uint32_t *acc, const RTD_AS3 uint32_t *pix,
                          const RTD_AS3 uint32_t *cand, const RTD_AS3 uint32_t *live, bool use_live, uint32_t total, uint32_t per, uint32_t s_base,
                          uint32_t split, Counters &cnt, StageStats &ss) {
    Sched<LDS, COUNT, TEX, LOG, FP> L(p, sc, cnt, ss, pool, poolLds);
    uint32_t next = 0; // wave-uniform
    const bool fastDiv = total < (1u << 22) && per < (1u << 23); // see div_uniform
    const float perRcp = 1.0f / (float) per;
    for (;;) {
        L.ended = false;
        const unsigned long long t0 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        // ---- refill: idle lanes take parked paths or the next items of the unit ----
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(L.st == L_IDLE);
        const bool haveNew = next < total;
        if (idle != 0ull && (haveNew || (L.parked | L.parkedL | L.parkedT) != 0u) && (__popcll(idle) >= p.refill_lanes || ~idle == 0ull)) {
            const uint32_t nIdle = (uint32_t) __popcll(idle);
            const uint32_t rank = lane_rank(idle);
            uint32_t nUnL, nUnA, nUnT;
            L.unpark_plan(nIdle, haveNew, nUnL, nUnA, nUnT);
            const uint32_t nUn = nUnL + nUnA + nUnT;
            if (COUNT || RTD_CLK) { ss.refill++; ss.refillLanes += nIdle; }
            if (L.st == L_IDLE) {
                if (!L.unpark_lane(rank, nUnL, nUnA, nUnT)) {
                    const uint32_t item = next + (rank - nUn);
                    if (item < total) {
                        uint32_t j = fastDiv ? div_uniform(item, per, perRcp) : item / per;
                        uint32_t s = s_base + (item - j * per);
                        uint32_t slot = use_live ? live[j] : j;
                        int row = (int) pix[slot * 4 + 0], col = (int) pix[slot * 4 + 1];
                        uint64_t pkey = (uint64_t) pix[slot * 4 + 2] | ((uint64_t) pix[slot * 4 + 3] << 32);
                        // low half: acc word, high half: pixel slot
                        L.start_item(pkey, s, row, col, (((s < split) ? 0u : (uint32_t) p.chunk * 3u) + slot * 3u) | (slot << 16), FP ? RTD_CAND_WALK : cand[slot * 2],
                                     FP ? RTD_CAND_WALK : cand[slot * 2 + 1]); // (footprint rays walk the tree: no pixel candidates)
                    }
                }
            }
            L.parked -= nUnA;
            L.parkedL -= nUnL;
            L.parkedT -= nUnT;
            next += nIdle - nUn;
            next = __builtin_amdgcn_readfirstlane(next);
        }
        if (__builtin_amdgcn_ballot_w64(L.st != L_IDLE) == 0ull) {
            if (next >= total && (L.parked | L.parkedL | L.parkedT) == 0u) break;
            continue;
        }
        const unsigned long long t1 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_tex();
        L.stage_slow();
        L.stage_lamb();
        const unsigned long long t2 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_walk();
        const unsigned long long t3 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_shade();
        if (COUNT || RTD_CLK) { const unsigned long long t4 = __builtin_amdgcn_s_memtime(); ss.tRefill += t1 - t0; ss.tSlow += t2 - t1; ss.tWalk += t3 - t2; ss.tShade += t4 - t3; }
        if (L.ended) {
            L.add_result(acc + (L.slotOff & 0xFFFFu));
            if (COST) lds_add(acc + 10u * (uint32_t) p.chunk + (L.slotOff >> 16), (uint32_t) L.bounces + 1u); // ~ Scene.hitObject calls of this path
        }
    }
}

// The ray-list modes: rtmode::RAYS_TRACE is Scene.traceRay (Scene.fs:93-114), RAYS_HIT Scene.hitObject (Scene.fs:62-91), for the caller's rays
// [0, p.ray_n).  A wave takes runs of p.chunk ray indices from the global queue -- as many runs at once as it has idle lanes for --
// and a lane's new item is ray i: Ray.make' of the caller's (origin, vector), its rng state (the caller's, or the stream keyed
// (seed, ray_base + i, ray_sample), as a render keys (pixel, sample)), colour White.  The walk starts at the root (no pixel
// candidates: those are a camera's), and every stage is Sched's, so parked paths carry the ray index in slotOff as they carry a
// pixel's accumulator word in a render.  Where a render adds an ended path's colour to its pixel, the ray's colour and final rng
// state are stored; RAYS_HIT instead stores (hit, strike) once the walk and the unbounded tests are done, and shades nothing.
template <bool LDS, bool COUNT, int TEX, bool HIT>
RTD_INLINE void run_rays(const RenderParams &p, const SceneView<LDS> &sc, unsigned char *pool, RTD_AS3 unsigned char *poolLds, Counters &cnt, StageStats &ss) {
    const int lane = threadIdx.x & 63;
    const uint32_t P = (uint32_t) p.chunk;
    Sched<LDS, COUNT, TEX, false> L(p, sc, cnt, ss, pool, poolLds);
    uint64_t next = 0, stop = 0; // wave-uniform: rays [next, stop) of the wave's current runs are not handed out yet
    bool exhausted = false;
    // a path's (or a query's) result, at its ray's index
    auto emit = [&](bool made) {
        const uint64_t i = (uint64_t) L.slotOff;
        if (HIT) {
            p.ray_hit[i] = !made ? -2 : (L.w.best < 0 ? -1 : p.obj_to_orig[L.w.best]);
            if (p.ray_strike) {
                const V3 sp = walk(L.o, L.d, L.w.bestLen);
                const double nanv = __builtin_nan("");
                const bool none = !made || L.w.best < 0;
                p.ray_strike[i * 3 + 0] = none ? nanv : sp.x;
                p.ray_strike[i * 3 + 1] = none ? nanv : sp.y;
                p.ray_strike[i * 3 + 2] = none ? nanv : sp.z;
            }
        } else {
            const uint32_t c = made ? L.result : RTD_BLACK;
            p.ray_colour[i * 3 + 0] = (uint8_t) c;
            p.ray_colour[i * 3 + 1] = (uint8_t) (c >> 8);
            p.ray_colour[i * 3 + 2] = (uint8_t) (c >> 16);
            if (p.ray_rng) {
                uint32_t *r = p.ray_rng + i * 4;
                r[0] = L.rng.x; r[1] = L.rng.y; r[2] = L.rng.z; r[3] = L.rng.w;
            }
        }
    };
    for (;;) {
        L.ended = false;
        const unsigned long long t0 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        // ---- refill: idle lanes take parked paths or the next rays; a new run is taken when the current one is used up ----
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(L.st == L_IDLE);
        const uint32_t nIdle = (uint32_t) __popcll(idle);
        if (nIdle != 0u && (next < stop || !exhausted || (L.parked | L.parkedL | L.parkedT) != 0u) && ((int) nIdle >= p.refill_lanes || nIdle == 64u)) {
            if (next >= stop && !exhausted) {
                const uint32_t want = (nIdle + P - 1u) / P; // runs
                uint32_t unit = 0;
                if (lane == 0) unit = atomicAdd(p.queue, want);
                unit = __builtin_amdgcn_readfirstlane(unit);
                const uint64_t first = (uint64_t) unit * P;
                if (first >= p.ray_n) exhausted = true;
                else { next = first; stop = first + (uint64_t) want * P; stop = stop < p.ray_n ? stop : p.ray_n; }
            }
            const uint32_t avail = (uint32_t) (stop - next < 64u ? stop - next : 64u);
            const uint32_t rank = lane_rank(idle);
            uint32_t nUnL, nUnA, nUnT;
            L.unpark_plan(nIdle, avail != 0u, nUnL, nUnA, nUnT);
            const uint32_t nUn = nUnL + nUnA + nUnT;
            if (COUNT || RTD_CLK) { ss.refill++; ss.refillLanes += nIdle; }
            const uint32_t rest = nIdle - nUn;
            const uint32_t take = rest < avail ? rest : avail;
            if (L.st == L_IDLE) {
                if (!L.unpark_lane(rank, nUnL, nUnA, nUnT) && rank - nUn < take) {
                    const uint64_t i = next + (rank - nUn);
                    const double *r = p.rays + i * 6;
                    L.o = mk(r[0], r[1], r[2]);
                    const V3 v = mk(r[3], r[4], r[5]);
                    if (p.ray_rng) { const uint32_t *g = p.ray_rng + i * 4; L.rng.x = g[0]; L.rng.y = g[1]; L.rng.z = g[2]; L.rng.w = g[3]; }
                    else L.rng = stream_for(pixel_key(p.seed_key, p.ray_base + i), p.ray_sample);
                    L.slotOff = (uint32_t) i;
                    L.colour = RTD_WHITE;
                    L.bounces = 0;
                    if (unitise(v, L.d)) { // Ray.make' (Ray.fs:26-34)
                        L.st = L_WALK;
                        walk_begin(L.w, sc.first);
                        if (COUNT) cnt.rays++;
                    } else emit(false); // ValueNone: no walk; Black (traceRay) or -2 (hitObject)
                }
            }
            L.parked -= nUnA;
            L.parkedL -= nUnL;
            L.parkedT -= nUnT;
            next += take;
        }
        if (__builtin_amdgcn_ballot_w64(L.st != L_IDLE) == 0ull) {
            if (next >= stop && exhausted && (L.parked | L.parkedL | L.parkedT) == 0u) break;
            continue;
        }
        const unsigned long long t1 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        if (!HIT) {
            L.stage_tex();
            L.stage_slow();
            L.stage_lamb();
        }
        const unsigned long long t2 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_walk();
        const unsigned long long t3 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        if (HIT) { // the rest of Scene.hitObject (Scene.fs:77-91): the unbounded objects, then the answer
            if (__builtin_amdgcn_ballot_w64(L.st == L_DONE) != 0ull && L.st == L_DONE) {
                unbounded_tests<LDS, COUNT>(sc, L.o, L.d, L.w, cnt);
                emit(true);
                L.st = L_IDLE; L.w.off = L.end;
            }
        } else L.stage_shade();
        if (COUNT || RTD_CLK) { const unsigned long long t4 = __builtin_amdgcn_s_memtime(); ss.tRefill += t1 - t0; ss.tSlow += t2 - t1; ss.tWalk += t3 - t2; ss.tShade += t4 - t3; }
        if (!HIT && L.ended) emit(true);
    }
}

// The set-up of a unit's pixel by lane `lane`: writes the four words pix[lane * 4 ..] (row, col, stream key lo, hi) of local pixel
// `local` and answers, as pixel_candidates (rt_device.h) does, the pixel's two candidate words -- the first returned, the second in
// `second` -- which the caller stores where it keeps them (pass B behind its two slots, the others at cand[lane * 2]).  The sources
// differ only in how the global pixel g and its (r, c) are found:
//   Pixels::FRAME       lp counts the shard's pixels row by row: image row row_first + (lp / cols) * row_stride
//   Pixels::LIST        g = pixel_list[lp]; OPTIONAL_LIST (camera hits): a null list is every pixel of the frame, g = lp
// (A footprint has no frame and no candidates: footprint_setup below.)
// Three things about the form keep the callers' code as it is when the lines stand in the caller, and are to be kept: `local` comes in
// the caller's width (pass B's list entries are 32-bit and are widened HERE, so that the division is still narrowed to 32 bits); the
// second word lives in the caller, as pixel_candidates' own does (so a footprint, which has none, has a function of its own); each
// store's address is formed at the store (pix and lane, not pix + lane * 4).  (profiles/r17/device_code.txt)
template <bool LDS, bool COUNT, rtmode::Pixels SRC, bool OPTIONAL_LIST = false, typename LP>
RTD_INLINE uint32_t pixel_setup(const RenderParams &p, const SceneView<LDS> &sc, LP local, RTD_AS3 uint32_t *pix, int lane, uint32_t &second) {
    static_assert(SRC == rtmode::Pixels::FRAME || SRC == rtmode::Pixels::LIST, "a pixel of the frame");
    const unsigned long long lp = (unsigned long long) local;
    uint32_t r, c;
    uint64_t g; // global pixel index
    if constexpr (SRC == rtmode::Pixels::LIST) {
        const uint32_t gl = (!OPTIONAL_LIST || p.pixel_list) ? (uint32_t) p.pixel_list[lp] : (uint32_t) lp;
        r = gl / (uint32_t) p.cols;
        c = gl - r * (uint32_t) p.cols;
        g = (uint64_t) gl;
    } else {
        const uint32_t lr = (uint32_t) (lp / (unsigned long long) p.cols);
        c = (uint32_t) (lp - (unsigned long long) lr * (unsigned long long) p.cols);
        r = (uint32_t) p.row_first + lr * (uint32_t) p.row_stride;
        g = (uint64_t) r * (uint64_t) p.cols + c;
    }
    const uint64_t pkey = pixel_key(p.seed_key, g);
    pix[lane * 4 + 0] = (uint32_t) (p.max_h - (int) r - 1); // the row flipped, the column centred (Scene.fs:219,226)
    pix[lane * 4 + 1] = (uint32_t) ((int) c - p.max_w);
    pix[lane * 4 + 2] = (uint32_t) pkey;
    pix[lane * 4 + 3] = (uint32_t) (pkey >> 32);
    const CameraParams *cp = p.cam_ptr;
    asm volatile("" : "+s"(cp)); // read the camera here: its words must not sit in SGPRs across the caller's loop
    return pixel_candidates<LDS, !COUNT>(sc, *cp, p.max_h - (int) r - 1, (int) c - p.max_w, second);
}

// ... and of a footprint: the list index where a frame keeps (row, col), the stream of (seed, stream_base + index), and no candidates --
// a footprint's camera rays walk the tree from the root (run_items)
template <typename LP> RTD_INLINE void footprint_setup(const RenderParams &p, LP local, RTD_AS3 uint32_t *pix, int lane) {
    const unsigned long long lp = (unsigned long long) local;
    const uint64_t pkey = pixel_key(p.seed_key, p.ray_base + lp);
    pix[lane * 4 + 0] = (uint32_t) lp;
    pix[lane * 4 + 1] = 0u;
    pix[lane * 4 + 2] = (uint32_t) pkey;
    pix[lane * 4 + 3] = (uint32_t) (pkey >> 32);
}

// A batch of views (render_views_kernel): the camera and the seed key of `view` into the copy of the kernel's parameters that the unit's (the
// range's) set-up and its new items read.  Scalar pointers: the view is wave-uniform.  (A function template, so that the kernels without
// views, where the copy is a reference to the const parameters, never see the assignments.)
template <bool VIEWS, class Params> RTD_INLINE void set_view(Params &pu, const RenderParams &p, uint32_t view) {
    if constexpr (VIEWS) {
        pu.cam_ptr = p.view_cams + view;
        pu.seed_key = p.view_keys[view];
    }
}

// Camera hits (rtmode::CAMERA_HITS [14], rt_camera_hits): Scene.hitObject (Scene.fs:62-91) of the ray Scene.traceOnce (Scene.fs:129-143) gives sample s
// of a frame's pixel, for samples [cam_sample_first, cam_sample_first + cam_n_samples) of the caller's list entries [0, p.ray_n) -- the
// pixel modes' unit set-up (pixel_setup) feeding RAYS_HIT's tail.  A wave takes a unit of p.chunk entries from the global queue and writes, once per
// entry, its pix words (row, col, stream key) and its two candidate words to the wave's scratch -- the frame's own set-up code, with
// g = pixel_list ? pixel_list[lp] : lp -- then hands the unit's npx * cam_n_samples items to idle lanes through Sched::start_item,
// the item's output slot in slotOff.  A started item has copied what it needs of the scratch, so the next unit is taken as soon as the
// last item is handed out: nothing drains at a unit's end.  There is no shading, so no park pool and no stage but the walk; a lane
// whose walk is done runs the unbounded tests and stores (hit, strike, ray).  In the timed variant a camera ray starts from its
// pixel's candidates exactly as a frame's does; the counting variant walks from the root.
// VIEWS (a batch of views, camera_hits_views_kernel, rt_camera_hits_views): the ONE list of p.view_pixels entries is answered for each of
// p.n_views cameras.  A unit is p.chunk entries inside one view (rtviews::unit_of: the last unit of a view is short), `pu` is the kernel's
// parameters with the camera and the seed key of the unit being HANDED OUT -- pixel_setup and start_item read them, a started item has
// copied what it needs -- and the unit's first item has slot (view * entries + first) * cam_n_samples.
template <bool LDS, bool COUNT, bool VIEWS = false>
RTD_INLINE void run_camera_hits(const RenderParams &p, const SceneView<LDS> &sc, unsigned char *pool, RTD_AS3 unsigned char *poolLds, RTD_AS3 uint32_t *wv, Counters &cnt,
                                StageStats &ss) {
    const int lane = threadIdx.x & 63;
    const uint32_t P = (uint32_t) p.chunk;
    const uint32_t per = (uint32_t) p.cam_n_samples;
    RTD_AS3 uint32_t *pix = wv;           // [P][4]
    RTD_AS3 uint32_t *cand = wv + 4u * P; // [P][2]
    std::conditional_t<VIEWS, RenderParams, const RenderParams &> pu = p;
    Sched<LDS, COUNT, false, false> L(pu, sc, cnt, ss, pool, poolLds);
    // wave-uniform: items [next, total) of the current unit are not handed out yet; the unit's first item has output slot slot0
    uint32_t next = 0, total = 0, slot0 = 0;
    bool exhausted = false;
    const bool fastDiv = (uint64_t) P * (uint64_t) per < (1ull << 22) && per < (1u << 23); // a unit holds at most P * per items; see div_uniform
    const float perRcp = 1.0f / (float) per;
    // a query's answer, at its slot (n * n_samples <= INT32_MAX: every index below fits 64-bit arithmetic on a 32-bit slot)
    auto emit = [&](bool made) {
        const uint64_t i = (uint64_t) L.slotOff;
        const double nanv = __builtin_nan("");
        const bool none = !made || L.w.best < 0;
        p.ray_hit[i] = !made ? -2 : (L.w.best < 0 ? -1 : p.obj_to_orig[L.w.best]);
        if (p.ray_strike) {
            const V3 sp = walk(L.o, L.d, L.w.bestLen); // Ray.walkAlong ray bestLength (Scene.fs:91)
            p.ray_strike[i * 3 + 0] = none ? nanv : sp.x;
            p.ray_strike[i * 3 + 1] = none ? nanv : sp.y;
            p.ray_strike[i * 3 + 2] = none ? nanv : sp.z;
        }
        if (p.cam_rays_out) {
            double *r = p.cam_rays_out + i * 6;
            r[0] = made ? L.o.x : nanv; r[1] = made ? L.o.y : nanv; r[2] = made ? L.o.z : nanv;
            r[3] = made ? L.d.x : nanv; r[4] = made ? L.d.y : nanv; r[5] = made ? L.d.z : nanv;
        }
    };
    for (;;) {
        const unsigned long long t0 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        // ---- refill: idle lanes take the next items of the unit; a new unit is taken when the current one is handed out ----
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(L.st == L_IDLE);
        const uint32_t nIdle = (uint32_t) __popcll(idle);
        if (nIdle != 0u && (next < total || !exhausted) && ((int) nIdle >= p.refill_lanes || nIdle == 64u)) {
            if (next >= total && !exhausted) {
                uint32_t unit = 0;
                if (lane == 0) unit = atomicAdd(p.queue, 1u);
                unit = __builtin_amdgcn_readfirstlane(unit);
                if constexpr (VIEWS) { // the unit's view, its entries inside the list, the view's camera and seed key (all wave-uniform)
                    if ((unsigned long long) unit >= (unsigned long long) p.n_views * p.view_units) exhausted = true;
                    else {
                        const rtviews::Plan pl{p.view_pixels, P, p.n_views};
                        const rtviews::Unit u = rtviews::unit_of(pl, p.view_units, unit);
                        set_view<VIEWS>(pu, p, u.view);
                        __builtin_amdgcn_wave_barrier(); // (the last unit's words have all been read)
                        if ((uint32_t) lane < u.npx) { // a busy lane too: nothing of its path's state is touched
                            uint32_t c2;
                            const uint32_t c1 = pixel_setup<LDS, COUNT, rtmode::Pixels::LIST, true>(pu, sc, u.first + (uint32_t) lane, pix, lane, c2);
                            cand[lane * 2] = c1;
                            cand[lane * 2 + 1] = c2;
                        }
                        __builtin_amdgcn_wave_barrier();
                        next = 0u; total = u.npx * per; slot0 = rtviews::first_slot(pl, u.view, u.first, per);
                    }
                } else { // (the lines rt_camera_hits' kernels have always had, kept apart so that they compile to what they did)
                const unsigned long long first = (unsigned long long) unit * P;
                if (first >= p.ray_n) exhausted = true;
                else {
                    const uint32_t npx = (uint32_t) ((p.ray_n - first < (unsigned long long) P) ? (p.ray_n - first) : (unsigned long long) P);
                    __builtin_amdgcn_wave_barrier(); // (the last unit's words have all been read)
                    if ((uint32_t) lane < npx) { // a busy lane too: nothing of its path's state is touched
                        const unsigned long long lp = first + (uint32_t) lane;
                        uint32_t c2;
                        const uint32_t c1 = pixel_setup<LDS, COUNT, rtmode::Pixels::LIST, true>(p, sc, lp, pix, lane, c2);
                        cand[lane * 2] = c1;
                        cand[lane * 2 + 1] = c2;
                    }
                    __builtin_amdgcn_wave_barrier();
                    next = 0u; total = npx * per; slot0 = (uint32_t) first * per;
                }
                }
            }
            const uint32_t avail = total - next;
            const uint32_t take = nIdle < avail ? nIdle : avail;
            const uint32_t rank = lane_rank(idle);
            if (COUNT || RTD_CLK) { ss.refill++; ss.refillLanes += nIdle; }
            if (L.st == L_IDLE && rank < take) {
                const uint32_t item = next + rank;
                const uint32_t j = fastDiv ? div_uniform(item, per, perRcp) : item / per;
                const uint32_t s = (uint32_t) p.cam_sample_first + (item - j * per);
                const int row = (int) pix[j * 4 + 0], col = (int) pix[j * 4 + 1];
                const uint64_t pkey = (uint64_t) pix[j * 4 + 2] | ((uint64_t) pix[j * 4 + 3] << 32);
                if (!L.start_item(pkey, s, row, col, slot0 + item, cand[j * 2], cand[j * 2 + 1])) emit(false); // ValueNone: no walk; -2
            }
            next += take;
        }
        if (__builtin_amdgcn_ballot_w64(L.st != L_IDLE) == 0ull) {
            if (next >= total && exhausted) break;
            continue;
        }
        const unsigned long long t1 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_walk();
        const unsigned long long t2 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        // the rest of Scene.hitObject (Scene.fs:77-91): the unbounded objects, then the answer
        if (__builtin_amdgcn_ballot_w64(L.st == L_DONE) != 0ull && L.st == L_DONE) {
            unbounded_tests<LDS, COUNT>(sc, L.o, L.d, L.w, cnt);
            emit(true);
            L.st = L_IDLE; L.w.off = L.end;
        }
        if (COUNT || RTD_CLK) { const unsigned long long t3 = __builtin_amdgcn_s_memtime(); ss.tRefill += t1 - t0; ss.tWalk += t2 - t1; ss.tShade += t3 - t2; }
    }
}

// Pass B (rtmode::Pass::B): phase 2 for the pixels of the cost-ordered list, STREAMED.  A wave reserves a run of list entries ("range"),
// hands out its npx*n2 items, and while the last paths of that range are still in flight it already reserves the next range and
// hands out its items: two accumulator slots alternate, a range is flushed (its sums added to what pass A left in `accum`) when
// its last path has ended.  There is no dependency between ranges, so no lane waits at a range boundary -- which is what makes
// small ranges (good load balance across waves) affordable.  Lane states and stage scheduling are Sched's.
// MAP (an extension by map, rt_render_extend_map): every pixel of the list has a range of samples of its own, Count .. target-1.  When
// a range is reserved lane j reads its pixel's Count and target, the counts n2_j = target - Count are prefix-summed across the wave,
// and the wave's scratch keeps per pixel its first item and (Count - first item); an item finds its pixel by rtm::map_find_pixel
// (at most six LDS reads, no division) and is sample (Count - first item) + item; flush leaves Count = target.  n1 and n2 are unused.
// PX (a pixel list, rt_render_pixels): list entry lp is the frame's pixel p.pixel_list[lp]; everything but that look-up is the frame's.
// JOB (a render job, render_job_kernel): in front of a reservation lane 0 polls the job's stop word -- set: nothing is reserved, exactly as when
// the list is exhausted, and the ranges already reserved are finished and flushed as usual -- and clips the reservation to the job's
// budget; a flushed range's pixels are final and are published (job_publish).
// VIEWS (a batch of views, render_views_kernel): the list holds batch pixels ordered by view, and a range never spans two views -- a
// reservation is handed out as ranges clipped at the end of the view of their first entry (rtviews::range_in_view), the rest kept for the
// next range.  `pv` is the kernel's parameters with the camera and the seed key of the range being HANDED OUT: pixel_setup and
// start_item read them, and only the current range hands out items; a draining range needs neither.
template <bool LDS, bool COUNT, int TEX, bool FP, bool MAP = false, bool PX = false, bool JOB = false, bool VIEWS = false>
RTD_INLINE void run_stream(const RenderParams &p, const SceneView<LDS> &sc, unsigned char *pool, RTD_AS3 unsigned char *poolLds, RTD_AS3 uint32_t *wv, uint32_t n1, uint32_t n2, Counters &cnt,
                           StageStats &ss, uint64_t &sampleCount, const JobCtl *job = nullptr) {
    const int lane = threadIdx.x & 63;
    const uint32_t P = (uint32_t) p.chunk;
    const uint32_t SW = 7u * P; // words per slot: acc [P][3] then pix [P][4]
    const unsigned long long nList = (unsigned long long) *p.live_count;
    std::conditional_t<VIEWS, RenderParams, const RenderParams &> pv = p;
    Sched<LDS, COUNT, TEX, false, FP> L(pv, sc, cnt, ss, pool, poolLds); // slotOff: word offset from wv of the path's accumulator triple (>= SW: slot 1)
    unsigned long long restFirst = 0; // VIEWS, wave-uniform: what is left of the last reservation beyond the view of its first ranges
    uint32_t restN = 0, viewBase = 0; // ... and the first batch pixel of the current range's view

    // wave-uniform: the range being handed out (cur) and the one draining (prev)
    unsigned long long curFirst = 0, prevFirst = 0;
    uint32_t curNpx = 0, curNext = 0, curTotal = 0, curOut = 0, curSlot = 1;
    uint32_t prevNpx = 0, prevOut = 0, prevSlot = 0;
    bool exhausted = false;
    const bool fastDiv = (uint64_t) P * (uint64_t) n2 < (1ull << 22) && n2 < (1u << 23); // a range holds at most P * n2 items; see div_uniform
    const float perRcp = 1.0f / (float) n2;

    auto flush = [&](unsigned long long first, uint32_t npx, uint32_t slot) {
        RTD_AS3 uint32_t *acc = wv + slot * SW;
        if ((uint32_t) lane < npx) { // this wave is the only writer of these pixels
            const unsigned long long lp = (unsigned long long) p.live_list[first + (uint32_t) lane];
            const i4 prev = ((const i4 *) p.accum)[lp];
            i4 out;
            uint32_t add = n2;
            if constexpr (MAP) add = (uint32_t) (p.ext_targets[lp] - prev.x); // (the list holds only pixels with Count < target)
            out.x = prev.x + (int) add;
            out.y = prev.y + (int) lds_take(acc + lane * 3 + 0);
            out.z = prev.z + (int) lds_take(acc + lane * 3 + 1);
            out.w = prev.w + (int) lds_take(acc + lane * 3 + 2);
            sampleCount += (uint64_t) add;
            ((i4 *) p.accum)[lp] = out;
            if (p.rgb) {
                p.rgb[lp * 3 + 0] = (uint8_t) (out.y / out.x);
                p.rgb[lp * 3 + 1] = (uint8_t) (out.z / out.x);
                p.rgb[lp * 3 + 2] = (uint8_t) (out.w / out.x);
            }
        }
        __builtin_amdgcn_wave_barrier();
        RTD_CENSUS(ss.flushes++;)
        if constexpr (JOB) { if (lane == 0) job_publish(*job, npx); }
    };

    for (;;) {
        L.ended = false;
        RTD_CENSUS(ss.turns++;)
        const unsigned long long t0 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        // ---- ranges: flush what has drained, reserve the next one when the current one has no items left ----
        if (prevNpx != 0u && prevOut == 0u) { flush(prevFirst, prevNpx, prevSlot); prevNpx = 0u; }
        if (curNext >= curTotal && prevNpx == 0u) {
            if (curNpx != 0u) { // the current range becomes the draining one (or is flushed at once if nothing is in flight)
                if (curOut == 0u) flush(curFirst, curNpx, curSlot);
                else { prevFirst = curFirst; prevNpx = curNpx; prevOut = curOut; prevSlot = curSlot; }
                curNpx = 0u; curNext = curTotal = curOut = 0u;
            }
            if (!exhausted) {
                unsigned long long first = 0;
                uint32_t npx = 0;
                if (VIEWS && restN != 0u) { first = restFirst; npx = restN; }
                else if (lane == 0) { // guided self-scheduling over the cost-ordered list: big ranges first, single pixels at the end
                    const unsigned long long seen = __hip_atomic_load(p.queue_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    bool open = seen < nList;
                    if constexpr (JOB) open = open && !job_stop_requested(*job);
                    if (open) {
                        unsigned long long want = (nList - seen) / (2ull * p.total_waves);
                        want = want < 1ull ? 1ull : (want > (unsigned long long) P ? (unsigned long long) P : want);
                        first = atomicAdd(p.queue_b, want);
                        if constexpr (JOB) npx = (uint32_t) rtjob::clip_reservation(first, want, nList, job->limit);
                        else if (first < nList) npx = (uint32_t) ((nList - first < want) ? (nList - first) : want);
                    }
                }
                npx = __builtin_amdgcn_readfirstlane(npx);
                if (npx == 0u) exhausted = true;
                else {
                    first = ((unsigned long long) __builtin_amdgcn_readfirstlane((uint32_t) (first >> 32)) << 32) |
                            __builtin_amdgcn_readfirstlane((uint32_t) first);
                    if constexpr (VIEWS) { // the range ends with its view; the camera and the seed key of that view
                        const uint32_t view = rtviews::view_of(p.view_pixels, (uint32_t) __builtin_amdgcn_readfirstlane((int) p.live_list[first]));
                        const uint32_t take = rtviews::range_in_view(first, npx, (unsigned long long) p.view_end[view]);
                        restFirst = first + take; restN = npx - take; npx = take;
                        viewBase = view * p.view_pixels;
                        set_view<VIEWS>(pv, p, view);
                    }
                    if (prevNpx != 0u) curSlot = prevSlot ^ 1u; // the draining range keeps its slot
                    RTD_AS3 uint32_t *acc = wv + curSlot * SW;
                    RTD_AS3 uint32_t *pix = acc + 3u * P;
                    for (uint32_t i = (uint32_t) lane; i < 3u * P; i += 64u) acc[i] = 0u;
                    if ((uint32_t) lane < npx) {
                        if constexpr (FP) footprint_setup(p, p.live_list[first + (uint32_t) lane], pix, lane);
                        else {
                            uint32_t c2;
                            uint32_t c1;
                            if constexpr (VIEWS) c1 = pixel_setup<LDS, COUNT, rtmode::Pixels::FRAME>(pv, sc, p.live_list[first + (uint32_t) lane] - viewBase, pix, lane, c2);
                            else c1 = pixel_setup<LDS, COUNT, PX ? rtmode::Pixels::LIST : rtmode::Pixels::FRAME>(p, sc, p.live_list[first + (uint32_t) lane], pix, lane, c2);
                            wv[14u * P + (curSlot * P + lane) * 2u] = c1;
                            wv[14u * P + (curSlot * P + lane) * 2u + 1u] = c2;
                        }
                    }
                    uint32_t total = npx * n2;
                    if constexpr (MAP) { // the pixels' own ranges: n2_j prefix-summed across the wave
                        uint32_t have = 0u, add = 0u;
                        if ((uint32_t) lane < npx) {
                            const unsigned long long lp = (unsigned long long) p.live_list[first + (uint32_t) lane];
                            const int c = ((const i4 *) p.accum)[lp].x, t = p.ext_targets[lp];
                            have = (uint32_t) c;
                            add = t > c ? (uint32_t) (t - c) : 0u;
                        }
                        uint32_t upTo = add; // inclusive
#pragma unroll
                        for (int off = 1; off < 64; off <<= 1) {
                            const uint32_t v = (uint32_t) __shfl_up((int) upTo, off, 64);
                            if (lane >= off) upTo += v;
                        }
                        total = (uint32_t) __builtin_amdgcn_readlane((int) upTo, 63); // <= 64 * 8e6 < 2^32
                        if ((uint32_t) lane < npx) {
                            wv[18u * P + curSlot * P + lane] = upTo - add;
                            wv[20u * P + curSlot * P + lane] = have - (upTo - add);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    curFirst = first; curNpx = npx; curNext = 0u; curTotal = total; curOut = 0u;
                    RTD_CENSUS(ss.ranges++;)
                }
            }
        }
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(L.st == L_IDLE);
        if (curNpx == 0u && prevNpx == 0u && exhausted && idle == ~0ull) break; // parked paths keep their range open, so none is left

        // ---- refill: parked paths, or items of the current range ----
        {
            const uint32_t nIdle = (uint32_t) __popcll(idle);
            const uint32_t avail = curTotal - curNext;
            if (nIdle != 0u && (avail != 0u || (L.parked | L.parkedL | L.parkedT) != 0u) && ((int) nIdle >= p.refill_lanes || nIdle == 64u)) {
                const uint32_t rank = lane_rank(idle);
                uint32_t nUnL, nUnA, nUnT;
                L.unpark_plan(nIdle, avail != 0u, nUnL, nUnA, nUnT);
                const uint32_t nUn = nUnL + nUnA + nUnT;
                if (COUNT || RTD_CLK) { ss.refill++; ss.refillLanes += nIdle; }
                const uint32_t rest = nIdle - nUn;
                const uint32_t take = rest < avail ? rest : avail;
                bool started = false;
                if (L.st == L_IDLE) {
                    if (!L.unpark_lane(rank, nUnL, nUnA, nUnT) && rank - nUn < take) {
                        const uint32_t item = curNext + (rank - nUn);
                        uint32_t j, smp;
                        if constexpr (MAP) {
                            j = rtm::map_find_pixel((const RTD_AS3 uint32_t *) (wv + 18u * P + curSlot * P), curNpx, item);
                            smp = wv[20u * P + curSlot * P + j] + item;
                        } else {
                            j = fastDiv ? div_uniform(item, n2, perRcp) : item / n2;
                            smp = n1 + (item - j * n2);
                        }
                        const RTD_AS3 uint32_t *pix = wv + curSlot * SW + 3u * P;
                        const int row = (int) pix[j * 4 + 0], col = (int) pix[j * 4 + 1];
                        const uint64_t pkey = (uint64_t) pix[j * 4 + 2] | ((uint64_t) pix[j * 4 + 3] << 32);
                        started = L.start_item(pkey, smp, row, col, curSlot * SW + j * 3u, FP ? RTD_CAND_WALK : wv[14u * P + (curSlot * P + j) * 2u],
                                               FP ? RTD_CAND_WALK : wv[14u * P + (curSlot * P + j) * 2u + 1u]);
                    }
                }
                L.parked -= nUnA;
                L.parkedL -= nUnL;
                L.parkedT -= nUnT;
                curNext += take;
                curOut += (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(started));
                RTD_CENSUS(ss.newRefills += take != 0u ? 1u : 0u; ss.newItems += take; ss.unparkL += nUnL; ss.unparkA += nUnA;
                            ss.unparkBatchesL += nUnL != 0u ? 1u : 0u; ss.unparkBatchesA += nUnA != 0u ? 1u : 0u;)
            }
        }
        if (__builtin_amdgcn_ballot_w64(L.st != L_IDLE) == 0ull) continue;

        const unsigned long long t1 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_tex();
        L.stage_slow();
        L.stage_lamb();
        const unsigned long long t2 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_walk();
        const unsigned long long t3 = (COUNT || RTD_CLK) ? __builtin_amdgcn_s_memtime() : 0ull;
        L.stage_shade();
        if (COUNT || RTD_CLK) { const unsigned long long t4 = __builtin_amdgcn_s_memtime(); ss.tRefill += t1 - t0; ss.tSlow += t2 - t1; ss.tWalk += t3 - t2; ss.tShade += t4 - t3; }
        if (L.ended) L.add_result(wv + L.slotOff);
        const bool inCur = (curNpx != 0u) && ((L.slotOff >= SW) == (curSlot == 1u));
        curOut -= (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(L.ended && inCur));
        prevOut -= (uint32_t) __popcll(__builtin_amdgcn_ballot_w64(L.ended && !inCur));
    }
}

// Stages the LDS part of the scene image into the workgroup's LDS, 16 B per lane per trip, coalesced, and makes the node links
// absolute LDS addresses: a walk position then IS the record's address (no add per visit).  Returns the bytes used.
// F32 = false (the counting variant): node | geo | meta, the exact double-precision records, walked by the compiled node_step.
// F32 = true (the timed variant): geo | meta | node32, the single-precision filter records in their queue form (rt_scene.h),
// walked by node_loop_lds32.
template <int BLOCK, bool F32>
RTD_INLINE uint32_t stage_scene(const RenderParams &p, unsigned char *smem) {
    const uint32_t sceneBytes = F32 ? p.off.lds32_total : p.off.lds_total;
    const d2 *src = (const d2 *) (p.scene_image + (F32 ? p.off.geo : 0u));
    RTD_AS3 d2 *dst = (RTD_AS3 d2 *) smem;
    for (uint32_t i = threadIdx.x; i < sceneBytes / 16u; i += BLOCK) dst[i] = src[i];
    __syncthreads();
    RTD_AS3 unsigned char *nodes = (RTD_AS3 unsigned char *) smem + (F32 ? p.off.node32 - p.off.geo : p.off.node);
    const int first = (int) (uint32_t) (uintptr_t) nodes;
    for (int i = threadIdx.x; i < p.off.n_nodes; i += BLOCK) {
        if (F32) {
            RTD_AS3 i2 *lk = (RTD_AS3 i2 *) (nodes + i * RTD_NODE32_BYTES + 48);
            i2 v = *lk; // on_hit, on_miss
            v.x += first;
            v.y += first;
            *lk = v;
        } else {
            RTD_AS3 i2 *lk = (RTD_AS3 i2 *) (nodes + i * RTD_NODE_BYTES + 96);
            i2 v = *lk;
            v.x += first; // a Leaf's RTD_LEAF flag (bit 30) is above every LDS address and survives the add
            v.y += first;
            *lk = v;
        }
    }
    __syncthreads();
    return sceneBytes;
}

// "Hybrid" (the timed variant of a scene that does not fit the LDS): the first p.lds_node_bytes of the node32 section -- its records
// are ordered by depth -- go to the START of the workgroup's LDS, links untouched (byte offsets from the section's start), so that a
// walk position below that limit is an LDS address as it is (node_loop_glb32).  Needs the dynamic LDS to start at address 0;
// returns the bytes staged, 0 (nothing in LDS, every visit from global memory) if it does not.
template <int BLOCK>
RTD_INLINE uint32_t stage_nodes32(const RenderParams &p, unsigned char *smem) {
    if ((uint32_t) (uintptr_t) (RTD_AS3 unsigned char *) smem != 0u) return 0u; // (the reservation stays unused; the host cannot know)
    const uint32_t bytes = (uint32_t) p.lds_node_bytes;
    const d2 *src = (const d2 *) (p.scene_image + p.off.node32);
    RTD_AS3 d2 *dst = (RTD_AS3 d2 *) smem;
    for (uint32_t i = threadIdx.x; i < bytes / 16u; i += BLOCK) dst[i] = src[i];
    __syncthreads();
    return bytes;
}

// MODE: one of rtmode::Mode (rt_modes.h: the table of the fifteen modes, what each does and what follows from it).  The parameter stays
// an int so that every kernel keeps its symbol; everything the kernel asks of it is read from the mode's description D.
// TEX: the scene has parameterised textures (see `reflection`).
// JOB: the stoppable variant of a frame pass (render_job_kernel below).  In front of a unit's reservation lane 0 polls the job's stop word:
// set, the wave reserves nothing and leaves as it does when the queue is exhausted; a unit at or beyond the job's budget is not
// rendered.  A fused unit's pixels are final when the unit ends, a pass-A unit's early-stopping pixels when its decision is made.
template <bool LDS, bool COUNT, int BLOCK, int MODE, bool TEX>
__global__ void __launch_bounds__(BLOCK) render_kernel(const RenderParams p) {
    constexpr bool JOB = false, VIEWS = false;
    const JobCtl *const job = nullptr;
#include "rt_render_body.inc"
}

// The stoppable variant of the frame passes (rtmode::FRAME_FUSED, FRAME_PASS_A, FRAME_PASS_B), under a symbol of its own: the timed variant
// only, at blocks of 256 and 1024 threads.  PASS: the mode's number.
template <bool LDS, int BLOCK, int PASS, bool TEX>
__global__ void __launch_bounds__(BLOCK) render_job_kernel(const RenderParams p, const JobCtl job_ctl) {
    static_assert(PASS == rtmode::FRAME_FUSED || PASS == rtmode::FRAME_PASS_A || PASS == rtmode::FRAME_PASS_B, "a frame pass");
    constexpr bool COUNT = false, JOB = true, VIEWS = false;
    constexpr int MODE = PASS;
    const JobCtl *const job = &job_ctl;
#include "rt_render_body.inc"
}

// The variants of both for a scene that holds at least one texture program (RT_TEXTURE_PROGRAM): the textured kernels with the program arm
// of texture_colour_at_inline compiled in, under symbols of their own, so that every kernel above stays exactly what it was.  Built for
// blocks of 256 and 1024 threads and for the modes that have a textured variant (rtmode::is_built_prog).  TEX = 2 inside the body: what is
// true of a textured kernel (the texture park pool, stage_tex) is true of these.
template <bool LDS, bool COUNT, int BLOCK, int MODE>
__global__ void __launch_bounds__(BLOCK) render_prog_kernel(const RenderParams p) {
    constexpr int TEX = 2;
    constexpr bool JOB = false, VIEWS = false;
    const JobCtl *const job = nullptr;
#include "rt_render_body.inc"
}
template <bool LDS, int BLOCK, int PASS>
__global__ void __launch_bounds__(BLOCK) render_prog_job_kernel(const RenderParams p, const JobCtl job_ctl) {
    static_assert(PASS == rtmode::FRAME_FUSED || PASS == rtmode::FRAME_PASS_A || PASS == rtmode::FRAME_PASS_B, "a frame pass");
    constexpr int TEX = 2;
    constexpr bool COUNT = false, JOB = true, VIEWS = false;
    constexpr int MODE = PASS;
    const JobCtl *const job = &job_ctl;
#include "rt_render_body.inc"
}

// A batch of views (rt_render_views; rt_views_plan.h, DESIGN.md "Batches of views"): the three frame passes under symbols of their own, so
// that every kernel above stays exactly what it was.  A unit (fused, pass A) and a pass-B range lie inside ONE view and read that view's
// camera and seed key through scalar pointers; everything else is the frame's.  Both variants (timed and counting), plain and textured
// scenes, blocks of 256 and 1024 threads; no texture programs.  PASS: the mode's number.
template <bool LDS, bool COUNT, int BLOCK, int PASS, bool TEX>
__global__ void __launch_bounds__(BLOCK) render_views_kernel(const RenderParams p) {
    // (FRAME_PASS_B_MAP: pass B of a batch's extension by map, rt_render_views_extend_map -- run_stream with MAP and VIEWS both on)
    static_assert(PASS == rtmode::FRAME_FUSED || PASS == rtmode::FRAME_PASS_A || PASS == rtmode::FRAME_PASS_B || PASS == rtmode::FRAME_PASS_B_MAP, "a frame pass");
    constexpr bool JOB = false, VIEWS = true;
    constexpr int MODE = PASS;
    const JobCtl *const job = nullptr;
#include "rt_render_body.inc"
}

// Camera hits over a batch of views (rt_camera_hits_views; DESIGN.md "Camera hits over a batch of views"): rtmode::CAMERA_HITS under a symbol of its
// own, so that every kernel above stays exactly what it was.  A unit is chunk entries of the shared list inside ONE view and reads that
// view's camera and seed key through scalar pointers (run_camera_hits<.., VIEWS>).  Both variants, blocks of 256 and 1024 threads; nothing
// is shaded, so there is no textured form.
template <bool LDS, bool COUNT, int BLOCK>
__global__ void __launch_bounds__(BLOCK) camera_hits_views_kernel(const RenderParams p) {
    constexpr int MODE = rtmode::CAMERA_HITS;
    constexpr bool TEX = false, JOB = false, VIEWS = true;
    const JobCtl *const job = nullptr;
#include "rt_render_body.inc"
}

// ---- a job's finishing kernels (rt_job_plan.h is the definition; these write what it says) ----
// What the job's kernels left, where the finishing kernels and rt_render_job_wait find it.  In the job's control block (host memory).
struct JobResult {
    long long n_present, complete;      // present pixels; 1: every pixel is present
    long long done_a, done_b, n_list;   // the counters, clamped (rtjob::clamp_done); the live list's length (0 for the fused kernel)
    unsigned long long samples;         // counters[4] at the job's end: every sample traced, discarded ones included
};
// One thread, first: the counters' final values become done_a / done_b (device words the next kernels read, and the result's)
__global__ void job_seal_kernel(const unsigned int *queue, const unsigned long long *queue_b, const unsigned int *live_count, rtjob::Plan pl, long long limit_a,
                                long long limit_b, unsigned long long *done /* [3]: done_a, done_b, n_present */, JobResult *res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t n_list = pl.passes == 2 ? (uint64_t) *live_count : 0u;
    done[0] = rtjob::clamp_done((uint64_t) *queue, rtjob::units_of(pl), limit_a);
    done[1] = pl.passes == 2 ? rtjob::clamp_done((uint64_t) *queue_b, n_list, limit_b) : 0u;
    done[2] = 0u;
    res->done_a = (long long) done[0]; res->done_b = (long long) done[1]; res->n_list = (long long) n_list;
}
// present[lp] from the prefix of units, for every local pixel
__global__ void __launch_bounds__(256) job_units_kernel(rtjob::Plan pl, const unsigned long long *done, uint8_t *present) {
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull, done_a = done[0];
    for (unsigned long long lp = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; lp < pl.n_local; lp += stride) present[lp] = rtjob::unit_done(pl, lp, done_a) ? 1u : 0u;
}
// ... less the live list's entries that pass B did not reach (two passes; the list holds local pixels below n_local, each once)
__global__ void __launch_bounds__(256) job_pending_kernel(const unsigned int *list, const unsigned int *live_count, const unsigned long long *done, uint8_t *present) {
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull, n_list = (unsigned long long) *live_count, done_b = done[1];
    for (unsigned long long i = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; i < n_list; i += stride)
        if (rtjob::entry_pending(i, done_b)) present[list[i]] = 0u;
}
// The absent pixels' PixelStats and colour zeroed (pass A's partial sums are discarded: the output does not depend on where the stop
// fell inside a pixel), the present ones counted.
__global__ void __launch_bounds__(256) job_zero_kernel(unsigned long long n_local, const uint8_t *present, int32_t *accum, uint8_t *rgb, unsigned long long *done) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n_local + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    unsigned long long n = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long lp = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        const bool in = lp < n_local, here = in && present[lp] != 0u;
        if (in && !here) {
            i4 z; z.x = z.y = z.z = z.w = 0;
            ((i4 *) accum)[lp] = z;
            if (rgb) { rgb[lp * 3 + 0] = 0u; rgb[lp * 3 + 1] = 0u; rgb[lp * 3 + 2] = 0u; }
        }
        n += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(here));
    }
    if (lane == 0 && n != 0ull) atomicAdd(&done[2], n);
}
// One thread, last: the result, and the exact count as the progress mirror's final value
__global__ void job_result_kernel(unsigned long long n_local, const unsigned long long *done, const unsigned long long *counters, JobResult *res,
                                  unsigned long long *progress, uint32_t *finished) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    res->n_present = (long long) done[2];
    res->complete = done[2] == n_local ? 1 : 0;
    res->samples = counters[4];
    __hip_atomic_store(progress, done[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(finished, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); // last: a host that sees it sees the count
}
// rt_render_job_finish: the absent pixels' list holds LOCAL pixels (rt_missing_pixels_device's kernels over `present`); the pixel-list
// launch wants the frame's
__global__ void __launch_bounds__(256) job_global_list_kernel(unsigned long long n, const int32_t *local, rtjob::Shard shard, int32_t *global) {
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; i < n; i += stride)
        global[i] = (int32_t) rtjob::global_pixel(shard, (uint64_t) (uint32_t) local[i]);
}
// ... and its results go back by local pixel: the 16-byte PixelStats, the colour, and the presence byte (every entry is a different pixel)
__global__ void __launch_bounds__(256) job_scatter_kernel(unsigned long long n, const int32_t *local, const int32_t *accum_list, const uint8_t *rgb_list,
                                                          int32_t *accum, uint8_t *rgb, uint8_t *present) {
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        const unsigned long long lp = (unsigned long long) (uint32_t) local[i];
        ((i4 *) accum)[lp] = ((const i4 *) accum_list)[i];
        if (rgb) { rgb[lp * 3 + 0] = rgb_list[i * 3 + 0]; rgb[lp * 3 + 1] = rgb_list[i * 3 + 1]; rgb[lp * 3 + 2] = rgb_list[i * 3 + 2]; }
        present[lp] = 1u;
    }
}


// ---- extending a rendered buffer (rt_render_extend): pass B's list from the stored PixelStats, instead of pass A and the sort ----
// A pixel of a buffer rendered (or last extended) with `done` >= RTD_EXTEND_MIN_DONE samples holds Count == done (it continues: it
// needs samples done .. spp-1) or Count == RTD_EARLY_COUNT (it stopped early and is final at every such spp).  Any other Count is
// FOREIGN: the buffer is not what the arguments say.  One coalesced 16-byte load per lane; per wave one agent-scope atomicAdd
// reserves the list entries of its continuing pixels (pass A's compaction), one counts its final pixels where pass A counts
// them (counters[5]), one its foreign ones.  The list's order is whatever the compaction gives: no result depends on it.
__global__ void __launch_bounds__(256) extend_list_kernel(const int32_t *accum, unsigned long long n, int32_t done, unsigned int *live_list,
                                                          unsigned int *live_count, unsigned long long *counters, unsigned int *foreign) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    unsigned long long nFinal = 0ull, nForeign = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long i = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        int count = RTD_EARLY_COUNT;
        if (i < n) count = ((const i4 *) accum)[i].x;
        const bool cont = i < n && count == done, foreignPx = i < n && count != done && count != RTD_EARLY_COUNT;
        const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(cont);
        const uint32_t nLive = (uint32_t) __popcll(liveMask);
        if (nLive > 0u) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(live_count, nLive);
            base = __builtin_amdgcn_readfirstlane(base);
            if (cont) live_list[base + lane_rank(liveMask)] = (unsigned int) i;
        }
        nForeign += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(foreignPx));
        nFinal += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(i < n && count == RTD_EARLY_COUNT));
    }
    if (lane == 0) {
        if (nFinal != 0ull) atomicAdd(&counters[5], nFinal);
        if (nForeign != 0ull) atomicAdd(foreign, (unsigned int) nForeign); // (n < 2^32: the sum cannot wrap to 0)
    }
}
// One wave, between the list and pass B: a buffer with even one foreign pixel is left as it is -- pass B reads its list length from
// `live_count`, so zeroing that continues NO pixel -- and `malformed` tells collect_stats (RT_ERR_INVALID_ARGUMENT).
__global__ void extend_seal_kernel(const unsigned int *foreign, unsigned int *live_count, unsigned int *malformed) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && *foreign != 0u) { *live_count = 0u; *malformed = 1u; }
}
// After the seal (so that a malformed buffer gets no byte written): PixelStats.mean of the FINAL pixels; pass B writes the others'.
__global__ void __launch_bounds__(256) extend_final_rgb_kernel(const int32_t *accum, unsigned long long n, const unsigned int *malformed, uint8_t *rgb) {
    if (*malformed != 0u) return;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        const i4 v = ((const i4 *) accum)[i];
        if (v.x != RTD_EARLY_COUNT) continue;
        rgb[i * 3 + 0] = (uint8_t) (v.y / v.x);
        rgb[i * 3 + 1] = (uint8_t) (v.z / v.x);
        rgb[i * 3 + 2] = (uint8_t) (v.w / v.x);
    }
}

// ---- a pixel list (rt_render_pixels): is every entry a pixel of the frame? ----
// extend_list_kernel's shape: one 4-byte load per lane, a ballot, one agent-scope atomicAdd per wave that saw an entry outside
// [0, frame_pixels) (frame_pixels <= INT32_MAX, so a negative entry is a large unsigned one).  The check guards MEANING, not memory:
// every store of a list render is indexed by list position.  For an extension `bad` is LaunchScratch::ext_foreign and the extension's
// own seal does the rest.
__global__ void __launch_bounds__(256) pixel_list_check_kernel(const int32_t *list, unsigned long long n, uint32_t frame_pixels, unsigned int *bad) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    unsigned long long nBad = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long i = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        uint32_t g = 0u;
        if (i < n) g = (uint32_t) list[i];
        nBad += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(i < n && g >= frame_pixels));
    }
    if (lane == 0 && nBad != 0ull) atomicAdd(bad, (unsigned int) nBad); // (n < 2^31: the sum cannot wrap to 0)
}
// One wave, between the check and a FRESH list render: with even one bad entry the unit counter is poisoned -- unit * chunk is then at
// or beyond n <= INT32_MAX for every wave that ever asks (the waves of a grid add far less than 2^31 to it), so the fused kernel and
// pass A start no unit, pass A appends nothing, the sort and pass B see an empty list, and neither accum nor rgb is written --
// and `malformed` tells collect_stats (RT_ERR_INVALID_ARGUMENT).
__global__ void pixel_list_seal_kernel(const unsigned int *bad, unsigned int *queue, unsigned int *malformed) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && *bad != 0u) { *queue = 0x80000000u; *malformed = 1u; }
}

// ---- extending by map (rt_render_extend_map): the list from the stored Counts AND the caller's per-pixel targets ----
// extend_list_kernel's shape -- one coalesced 16-byte load of the PixelStats plus one 4-byte load of the target per lane, ballot,
// lane_rank, one agent-scope atomicAdd per wave -- with the classes of a map: Count == 11 FINAL (whatever the target); Count >= 12 and
// Count < target <= cap CONTINUED; Count >= 12 and target <= Count LEFT as it is; Count < 11 or target > cap MALFORMED (counted in
// `foreign`: the seal then continues no pixel).  `cap` >= 12, so a continued pixel has 12 <= Count < target <= cap.
__global__ void __launch_bounds__(256) extend_map_list_kernel(const int32_t *accum, const int32_t *targets, unsigned long long n, int32_t cap,
                                                              unsigned int *live_list, unsigned int *live_count, unsigned long long *counters,
                                                              unsigned int *foreign) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    unsigned long long nFinal = 0ull, nForeign = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long i = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        int count = RTD_EARLY_COUNT, target = 0;
        if (i < n) { count = ((const i4 *) accum)[i].x; target = targets[i]; }
        const bool fin = i < n && count == RTD_EARLY_COUNT;
        const bool foreignPx = i < n && !fin && (count < RTD_EARLY_COUNT || target > cap);
        const bool cont = i < n && !fin && !foreignPx && target > count;
        const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(cont);
        const uint32_t nLive = (uint32_t) __popcll(liveMask);
        if (nLive > 0u) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(live_count, nLive);
            base = __builtin_amdgcn_readfirstlane(base);
            if (cont) live_list[base + lane_rank(liveMask)] = (unsigned int) i;
        }
        nForeign += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(foreignPx));
        nFinal += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(fin));
    }
    if (lane == 0) {
        if (nFinal != 0ull) atomicAdd(&counters[5], nFinal);
        if (nForeign != 0ull) atomicAdd(foreign, (unsigned int) nForeign); // (n < 2^32: the sum cannot wrap to 0)
    }
}
// extend_final_rgb_kernel for a map: PixelStats.mean of the FINAL pixels and of those LEFT as they are (Count >= target); pass B writes
// the continued ones'.  After the seal, before pass B: the Counts read here are the ones the list was built from.
__global__ void __launch_bounds__(256) extend_map_rest_rgb_kernel(const int32_t *accum, const int32_t *targets, unsigned long long n,
                                                                  const unsigned int *malformed, uint8_t *rgb) {
    if (*malformed != 0u) return;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; i < n; i += stride) {
        const i4 v = ((const i4 *) accum)[i];
        if (v.x != RTD_EARLY_COUNT && targets[i] > v.x) continue;
        rgb[i * 3 + 0] = (uint8_t) (v.y / v.x);
        rgb[i * 3 + 1] = (uint8_t) (v.z / v.x);
        rgb[i * 3 + 2] = (uint8_t) (v.w / v.x);
    }
}

// ---- ordering of the pass-B list: bucket sort of (cost, pixel) pairs, heaviest first -------------------------------------------
// 64 buckets over rays per phase-1 sample (x4); order inside a bucket is arbitrary (it only changes which wave traces what).
RTD_INLINE uint32_t cost_bucket(unsigned long long pair, uint32_t n1) {
    const uint32_t cost = (uint32_t) (pair >> 32);
    const uint32_t b = (cost * 4u) / n1;
    return b >= RTD_COST_BUCKETS ? RTD_COST_BUCKETS - 1u : b;
}
// Both kernels: one workgroup owns a contiguous slice of the list and counts it in LDS first, so the global atomics are one
// per (workgroup, bucket) -- per-item global atomics on 64 addresses serialise (measured: 0.78 ms for 174 k pairs when most
// pixels share a bucket).  The order inside a bucket is arbitrary; no result depends on it.
RTD_INLINE void sort_slice(unsigned int n, unsigned int &lo, unsigned int &hi) {
    const unsigned int per = (n + gridDim.x - 1u) / gridDim.x;
    lo = blockIdx.x * per;
    hi = lo + per < n ? lo + per : n;
    if (lo > n) lo = n;
}
__global__ void sort_hist_kernel(const unsigned long long *pairs, const unsigned int *count, uint32_t n1, unsigned int *hist) {
    __shared__ unsigned int local[RTD_COST_BUCKETS];
    if (threadIdx.x < RTD_COST_BUCKETS) local[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int lo, hi;
    sort_slice(*count, lo, hi);
    for (unsigned int i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&local[cost_bucket(pairs[i], n1)], 1u);
    __syncthreads();
    if (threadIdx.x < RTD_COST_BUCKETS && local[threadIdx.x] != 0u) atomicAdd(&hist[threadIdx.x], local[threadIdx.x]);
}
__global__ void sort_offsets_kernel(const unsigned int *hist, unsigned int *offsets) { // descending cost: bucket 63 first
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned int run = 0;
        for (int b = RTD_COST_BUCKETS - 1; b >= 0; --b) { offsets[b] = run; run += hist[b]; }
    }
}
__global__ void sort_scatter_kernel(const unsigned long long *pairs, const unsigned int *count, uint32_t n1, const unsigned int *offsets,
                                    unsigned int *cursor, unsigned int *list) {
    __shared__ unsigned int local[RTD_COST_BUCKETS], base[RTD_COST_BUCKETS];
    if (threadIdx.x < RTD_COST_BUCKETS) local[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int lo, hi;
    sort_slice(*count, lo, hi);
    for (unsigned int i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&local[cost_bucket(pairs[i], n1)], 1u);
    __syncthreads();
    if (threadIdx.x < RTD_COST_BUCKETS) { // reserve this workgroup's range of every bucket it holds items of
        const unsigned int c = local[threadIdx.x];
        base[threadIdx.x] = offsets[threadIdx.x] + (c != 0u ? atomicAdd(&cursor[threadIdx.x], c) : 0u);
        local[threadIdx.x] = 0u;
    }
    __syncthreads();
    for (unsigned int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const unsigned long long pr = pairs[i];
        const uint32_t b = cost_bucket(pr, n1);
        list[base[b] + atomicAdd(&local[b], 1u)] = (unsigned int) (pr & 0xFFFFFFFFull);
    }
}

// ---- ordering of a batch's pass-B list (rt_render_views): by view, inside a view heaviest first -------------------------------------
// A pair's low word is the batch pixel G, whose view is G / pixels_per_view; the key is rtviews::sort_key(view, buckets, cost bucket).
// A counting sort over n_keys = n_views * buckets keys: count, one workgroup's exclusive scan (which also writes where each view's
// entries END -- what clips pass B's ranges), scatter.  As in the frame's two kernels above, a workgroup owns a contiguous slice of the
// pairs and counts it in LDS first, so that the global atomics are one per (workgroup, key it holds) -- per-item global atomics on the
// few keys of a batch of few views serialise (measured at one view of 2401x1601, 500 spp: 9.4 ms each for the count and the scatter, beside a pass B of 97.6 ms).  That needs the keys to fit
// the LDS: `lds_keys` is n_keys where they do (at most VIEWS_SORT_LDS_KEYS: the scatter holds two words per key), else 0 -- a batch
// of that many views spreads its pairs over that many addresses, and the atomics go to global memory item by item.
enum { VIEWS_SORT_LDS_KEYS = 8192 };
RTD_INLINE uint32_t views_pair_key(unsigned long long pr, uint32_t n1, uint32_t pixels_per_view, uint32_t buckets) {
    return rtviews::sort_key(rtviews::view_of(pixels_per_view, (uint32_t) pr), buckets, cost_bucket(pr, n1));
}
__global__ void __launch_bounds__(256) views_sort_hist_kernel(const unsigned long long *pairs, const unsigned int *count, uint32_t n1, uint32_t pixels_per_view,
                                                              uint32_t buckets, uint32_t lds_keys, unsigned int *hist) {
    extern __shared__ unsigned int views_local[]; // [lds_keys]
    unsigned int lo, hi;
    sort_slice(*count, lo, hi);
    if (lds_keys == 0u) {
        for (unsigned int i = lo + threadIdx.x; i < hi; i += 256u) atomicAdd(&hist[views_pair_key(pairs[i], n1, pixels_per_view, buckets)], 1u);
        return;
    }
    for (uint32_t k = threadIdx.x; k < lds_keys; k += 256u) views_local[k] = 0u;
    __syncthreads();
    for (unsigned int i = lo + threadIdx.x; i < hi; i += 256u) atomicAdd(&views_local[views_pair_key(pairs[i], n1, pixels_per_view, buckets)], 1u);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < lds_keys; k += 256u)
        if (views_local[k] != 0u) atomicAdd(&hist[k], views_local[k]);
}
// One workgroup of 256 threads: counts -> first list index of every key, in place; view_end[v] = the end of view v's last key
__global__ void __launch_bounds__(256) views_sort_scan_kernel(unsigned int *hist, uint32_t n_views, uint32_t buckets, unsigned int *view_end) {
    __shared__ unsigned int part[256];
    const unsigned long long n = (unsigned long long) n_views * buckets, per = (n + 255ull) / 256ull;
    const unsigned long long lo = threadIdx.x * per < n ? threadIdx.x * per : n, hi = lo + per < n ? lo + per : n;
    unsigned int sum = 0u;
    for (unsigned long long i = lo; i < hi; ++i) sum += hist[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0u;
        for (int t = 0; t < 256; ++t) { const unsigned int c = part[t]; part[t] = run; run += c; }
    }
    __syncthreads();
    unsigned int run = part[threadIdx.x];
    for (unsigned long long i = lo; i < hi; ++i) {
        const unsigned int c = hist[i];
        hist[i] = run;
        run += c;
        if ((i + 1ull) % buckets == 0ull) view_end[i / buckets] = run;
    }
}
// cursor: the scan's result, every key's first list index; advanced by what each workgroup reserves (or, without LDS, item by item)
__global__ void __launch_bounds__(256) views_sort_scatter_kernel(const unsigned long long *pairs, const unsigned int *count, uint32_t n1, uint32_t pixels_per_view,
                                                                 uint32_t buckets, uint32_t lds_keys, unsigned int *cursor, unsigned int *list) {
    extern __shared__ unsigned int views_local[]; // [lds_keys] counts, then [lds_keys] this workgroup's first index of every key
    unsigned int lo, hi;
    sort_slice(*count, lo, hi);
    if (lds_keys == 0u) {
        for (unsigned int i = lo + threadIdx.x; i < hi; i += 256u) {
            const unsigned long long pr = pairs[i];
            list[atomicAdd(&cursor[views_pair_key(pr, n1, pixels_per_view, buckets)], 1u)] = (unsigned int) (pr & 0xFFFFFFFFull);
        }
        return;
    }
    unsigned int *base = views_local + lds_keys;
    for (uint32_t k = threadIdx.x; k < lds_keys; k += 256u) views_local[k] = 0u;
    __syncthreads();
    for (unsigned int i = lo + threadIdx.x; i < hi; i += 256u) atomicAdd(&views_local[views_pair_key(pairs[i], n1, pixels_per_view, buckets)], 1u);
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < lds_keys; k += 256u) { // reserve this workgroup's range of every key it holds items of
        const unsigned int c = views_local[k];
        base[k] = c != 0u ? atomicAdd(&cursor[k], c) : 0u;
        views_local[k] = 0u;
    }
    __syncthreads();
    for (unsigned int i = lo + threadIdx.x; i < hi; i += 256u) {
        const unsigned long long pr = pairs[i];
        const uint32_t k = views_pair_key(pr, n1, pixels_per_view, buckets);
        list[base[k] + atomicAdd(&views_local[k], 1u)] = (unsigned int) (pr & 0xFFFFFFFFull);
    }
}

// ---- continuing a batch of views (rt_render_views_extend, rt_render_views_extend_map): the PAIRS of the batch's ordering from the stored PixelStats ----
// extend_list_kernel and extend_map_list_kernel over the batch's n = n_views * pixels_per_view pixels, with the same classes, the same
// count of final pixels (counters[5]) and of foreign ones (`foreign`) -- but pass B of a batch wants its list ordered by view and
// view_end[] filled, which a compaction of one atomic per wave does not give.  So the continued pixels leave as pairs (cost << 32 | batch
// pixel), as pass A's do, and views_sort_hist / _scan / _scatter order them: by view, inside a view by decreasing cost.  The cost word is
// the samples to add -- the same for every pixel of a uniform extension, target - Count under a map (a view's longest jobs first); the
// host passes the sort kernels a divisor that spreads 0 .. cap over the cost buckets.  A view with no continued pixel gets no pair, so
// its keys count nothing and view_end[v] == view_end[v - 1]: no list entry is of that view and no range opens in it.  The seal
// (extend_seal_kernel) runs behind the ordering and before anything that writes; no result depends on the order.
__global__ void __launch_bounds__(256) views_extend_list_kernel(const int32_t *accum, unsigned long long n, int32_t done, int32_t target, unsigned long long *pairs,
                                                                unsigned int *live_count, unsigned long long *counters, unsigned int *foreign) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    const unsigned long long cost = (unsigned long long) (uint32_t) (target - done) << 32;
    unsigned long long nFinal = 0ull, nForeign = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long i = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        int count = RTD_EARLY_COUNT;
        if (i < n) count = ((const i4 *) accum)[i].x;
        const bool cont = i < n && count == done, foreignPx = i < n && count != done && count != RTD_EARLY_COUNT;
        const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(cont);
        const uint32_t nLive = (uint32_t) __popcll(liveMask);
        if (nLive > 0u) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(live_count, nLive);
            base = __builtin_amdgcn_readfirstlane(base);
            if (cont) pairs[base + lane_rank(liveMask)] = cost | (unsigned long long) (uint32_t) i; // (base + rank < n: every pixel is appended at most once)
        }
        nForeign += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(foreignPx));
        nFinal += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(i < n && count == RTD_EARLY_COUNT));
    }
    if (lane == 0) {
        if (nFinal != 0ull) atomicAdd(&counters[5], nFinal);
        if (nForeign != 0ull) atomicAdd(foreign, (unsigned int) nForeign); // (n < 2^31: the sum cannot wrap to 0)
    }
}
__global__ void __launch_bounds__(256) views_extend_map_list_kernel(const int32_t *accum, const int32_t *targets, unsigned long long n, int32_t cap,
                                                                    unsigned long long *pairs, unsigned int *live_count, unsigned long long *counters,
                                                                    unsigned int *foreign) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    unsigned long long nFinal = 0ull, nForeign = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long i = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        int count = RTD_EARLY_COUNT, target = 0;
        if (i < n) { count = ((const i4 *) accum)[i].x; target = targets[i]; }
        const bool fin = i < n && count == RTD_EARLY_COUNT;
        const bool foreignPx = i < n && !fin && (count < RTD_EARLY_COUNT || target > cap);
        const bool cont = i < n && !fin && !foreignPx && target > count;
        const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(cont);
        const uint32_t nLive = (uint32_t) __popcll(liveMask);
        if (nLive > 0u) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(live_count, nLive);
            base = __builtin_amdgcn_readfirstlane(base);
            if (cont) pairs[base + lane_rank(liveMask)] = ((unsigned long long) (uint32_t) (target - count) << 32) | (unsigned long long) (uint32_t) i;
        }
        nForeign += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(foreignPx));
        nFinal += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(fin));
    }
    if (lane == 0) {
        if (nFinal != 0ull) atomicAdd(&counters[5], nFinal);
        if (nForeign != 0ull) atomicAdd(foreign, (unsigned int) nForeign); // (n < 2^31: the sum cannot wrap to 0)
    }
}

// The per-view cameras and seed keys of a batch into the launch's scratch, VIEWS_INIT_CAMERAS views per launch as kernel arguments: no
// copy from pageable host memory, nothing of the caller's is read after the call (launch_init_kernel's reasons)
enum { VIEWS_INIT_CAMERAS = 24 };
struct ViewsInit { CameraParams cam[VIEWS_INIT_CAMERAS]; uint64_t key[VIEWS_INIT_CAMERAS]; uint32_t first, n; };
static_assert(sizeof(ViewsInit) <= 4096, "kernel arguments");
__global__ void views_init_kernel(CameraParams *cams, uint64_t *keys, const ViewsInit v) {
    if (threadIdx.x < v.n) { cams[v.first + threadIdx.x] = v.cam[threadIdx.x]; keys[v.first + threadIdx.x] = v.key[threadIdx.x]; }
}

} // namespace rtd
