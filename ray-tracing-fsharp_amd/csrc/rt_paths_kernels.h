// rt_paths_kernels.h -- path records (DESIGN.md "Path records"; rt_camera_paths, rt_trace_paths): Scene.traceRay (Scene.fs:93-114) with
// every vertex of the path written down.  A kernel beside render_kernel, not a mode of it: the scene arrives as the render's own
// RenderParams (image, offsets, textures: stage_scene and make_view read nothing else of it), everything of the job in PathParams.
//
// A SLOT is one path: sample s of list entry i (camera paths, slot i * n_samples + (s - sample_first)) or the caller's ray i (ray paths).
// The grid is persistent and every lane owns one path at a time.  What a path does per vertex is rtd::trace_ray's loop body
// (rt_device.h), statement for statement: Scene.hitObject, Ray.walkAlong, Hittable.Reflection, the bounce count.
#pragma once
#include "rt_render_kernel.h"

namespace rtd {

enum { PATH_MISS = 0, PATH_STOPPED = 1, PATH_BOUNCE_LIMIT = 2, PATH_NO_RAY = 3 }; // rt_path_end (include/rtfs_amd.h)
#define RTD_PATH_SUMMARY_WORDS 16

struct PathParams {
    // the source.  Camera paths: entry i is the frame's pixel pixel_list[i] (null: pixel i), stream (seed, g, s).  Ray paths (rays != null):
    // the caller's (origin, vector) through Ray.make', stream the caller's state (rng) or (seed, ray_base + i, ray_sample)
    const CameraParams *cam;
    const int32_t *pixel_list;
    const double *rays;            // [slots][6]; null: camera paths
    uint32_t *rng;                 // [slots][4] read, written back advanced; or null
    uint64_t seed_key, ray_base;
    uint32_t ray_sample;
    int32_t sample_first, n_samples;
    int32_t cols, max_w, max_h;
    int32_t depth;                 // maxCount
    int32_t chunk;                 // slots per run of the queue
    int32_t max_vertices;          // K: records kept per slot (0: none, the per-record pointers are not read)
    uint64_t slots;
    unsigned int *queue;           // next run (LaunchScratch::queue; poisoned by pixel_list_seal_kernel: no run is ever taken)
    unsigned long long *counters;  // LaunchScratch::counters [0..3] (COUNT)
    const int32_t *obj_to_orig;
    // the outputs; any may be null
    int32_t *n_vertices, *end;     // [slots]
    uint8_t *colour;               // [slots][3]
    double *first_ray;             // [slots][6] (camera paths)
    int32_t *hit_index;            // [slots * K]
    double *strike;                // [slots * K][3]
    uint8_t *colour_after;         // [slots * K][3]
    double *ray_after;             // [slots * K][6]
    int32_t *summary;              // [entries][16] (camera paths), zeroed on the launch's stream in front of the kernel
};

// Zeroes the summary behind the list's seal: a malformed list leaves every output as it was.
__global__ void __launch_bounds__(256) paths_summary_zero_kernel(int32_t *summary, unsigned long long words, const unsigned int *malformed) {
    if (malformed && *malformed != 0u) return;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long) blockIdx.x * 256ull + threadIdx.x; i < words; i += stride) summary[i] = 0;
}

RTD_INLINE void path_store_rgb(uint8_t *at, uint32_t c) { at[0] = (uint8_t) c; at[1] = (uint8_t) (c >> 8); at[2] = (uint8_t) (c >> 16); }

// The summary of the lanes whose path ended in this trip (`fin`): sixteen order-free integers per list entry.  Where all of them belong
// to one entry (the usual case with 64 samples or more per entry) the wave adds up first and one lane makes the atomics.
RTD_INLINE void path_summarise(const PathParams &q, bool fin, uint32_t entry, int nv, int end, uint32_t albedo, uint32_t colour) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(fin);
    if (mask == 0ull) return;
    const int lead = __builtin_ctzll(mask);
    const uint32_t e0 = (uint32_t) __shfl((int) entry, lead, 64);
    const bool uniform = __builtin_amdgcn_ballot_w64(fin && entry != e0) == 0ull;
    int v[RTD_PATH_SUMMARY_WORDS];
#pragma unroll
    for (int k = 0; k < RTD_PATH_SUMMARY_WORDS; ++k) v[k] = 0;
    if (fin) {
        v[0] = 1; v[1] = nv; v[2] = nv;
        v[3] = end == PATH_MISS; v[4] = end == PATH_STOPPED; v[5] = end == PATH_BOUNCE_LIMIT; v[6] = end == PATH_NO_RAY;
        if (nv >= 1) { v[7] = 1; v[8] = (int) (albedo & 0xFFu); v[9] = (int) ((albedo >> 8) & 0xFFu); v[10] = (int) ((albedo >> 16) & 0xFFu); }
        v[12] = 1; v[13] = (int) (colour & 0xFFu); v[14] = (int) ((colour >> 8) & 0xFFu); v[15] = (int) ((colour >> 16) & 0xFFu);
    }
    if (uniform) {
#pragma unroll
        for (int k = 0; k < RTD_PATH_SUMMARY_WORDS; ++k) {
            if (k == 11) continue;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const int o = __shfl_xor(v[k], off, 64);
                v[k] = k == 2 ? (o > v[k] ? o : v[k]) : v[k] + o;
            }
        }
    }
    if (uniform ? ((int) (threadIdx.x & 63) == lead) : fin) {
        int32_t *at = q.summary + (size_t) entry * RTD_PATH_SUMMARY_WORDS;
#pragma unroll
        for (int k = 0; k < RTD_PATH_SUMMARY_WORDS; ++k) {
            if (k == 11 || v[k] == 0) continue;
            if (k == 2) atomicMax(at + k, v[k]); else atomicAdd(at + k, v[k]);
        }
    }
}

// LDS: the timed variant of an LDS-resident scene -- the scene staged as the render stages it, Scene.hitObject by the filter loop
// (node_loop_lds32), the exact leaf tests between its runs, the unbounded objects last: rt_dev_hit_object_lds' loop.  Otherwise
// hit_object<false, COUNT> over the exact records in global memory: plain, exact, and -- this route has no filter loop -- the tree of
// a scene that does not fit the LDS is walked record by record in double precision.  COUNT is never combined with LDS.
// There are no pixel candidates: a camera ray walks the tree as every other ray does, and no result can depend on that.
// The source of a slot -- a frame's pixel sample or the caller's ray -- is a wave-uniform branch of the refill (q.rays), not a template
// parameter: half the instantiations for one scalar test a refill.
template <bool LDS, bool COUNT, bool TEX, int BLOCK>
__global__ void __launch_bounds__(BLOCK) paths_kernel(const RenderParams p, const PathParams q) {
    static_assert(!(LDS && COUNT), "the counting variant reads the exact records in global memory");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (LDS) (void) stage_scene<BLOCK, true>(p, smem);
    const SceneView<LDS> sc = make_view<LDS, LDS>(p, smem);
    const int lane = threadIdx.x & 63;
    const uint32_t P = (uint32_t) q.chunk;
    const uint32_t K = (uint32_t) q.max_vertices;
    const bool camera = q.rays == nullptr;
    const double nanv = __builtin_nan("");
    Counters cnt; cnt.rays = cnt.aabb = cnt.prim = cnt.refl = 0;

    // the lane's path
    bool live = false;
    uint32_t slot = 0u, entry = 0u, colour = RTD_WHITE, albedo = 0u;
    int nv = 0, bounces = 0;
    V3 o = mk(0.0, 0.0, 0.0), d = mk(1.0, 0.0, 0.0);
    Rng rng; rng.x = rng.y = rng.z = rng.w = 0u;
    // wave-uniform: slots [next, stop) of the wave's current runs are not handed out yet
    uint64_t next = 0, stop = 0;
    bool exhausted = false;

    // a path's end: the per-slot outputs, once, and the records it did not reach
    auto retire = [&](int end, uint32_t result) {
        const size_t i = (size_t) slot;
        if (q.n_vertices) q.n_vertices[i] = nv;
        if (q.end) q.end[i] = end;
        if (q.colour) path_store_rgb(q.colour + i * 3, result);
        if (q.rng) { uint32_t *r = q.rng + i * 4; r[0] = rng.x; r[1] = rng.y; r[2] = rng.z; r[3] = rng.w; }
        for (uint32_t j = (uint32_t) nv; j < K; ++j) { // (nv may exceed K: nothing to fill then)
            const size_t r = i * K + j;
            if (q.hit_index) q.hit_index[r] = -1;
            if (q.strike) { q.strike[r * 3] = nanv; q.strike[r * 3 + 1] = nanv; q.strike[r * 3 + 2] = nanv; }
            if (q.colour_after) path_store_rgb(q.colour_after + r * 3, 0u);
            if (q.ray_after) for (int a = 0; a < 6; ++a) q.ray_after[r * 6 + a] = nanv;
        }
        live = false;
    };

    // Bounded by construction: a trip either takes slots from the finite queue or advances EVERY live lane by one vertex, and a path has at
    // most depth + 1 of them.  Nothing here spins or waits on another wave: the only traffic between waves is the queue's atomicAdd and
    // the summary's integer atomics.
    for (;;) {
        // ---- (a) refill: lanes whose path ended take the next slots; as many runs are taken at once as the wave has idle lanes for ----
        const unsigned long long idle = __builtin_amdgcn_ballot_w64(!live);
        const uint32_t nIdle = (uint32_t) __popcll(idle);
        if (nIdle != 0u && (next < stop || !exhausted)) {
            if (next >= stop) {
                const uint32_t want = (nIdle + P - 1u) / P; // runs
                uint32_t unit = 0;
                if (lane == 0) unit = atomicAdd(q.queue, want);
                unit = __builtin_amdgcn_readfirstlane(unit);
                const uint64_t first = (uint64_t) unit * P;
                if (first >= q.slots) exhausted = true;
                else { next = first; stop = first + (uint64_t) want * P; stop = stop < q.slots ? stop : q.slots; }
            }
            const uint32_t avail = (uint32_t) (stop - next < 64u ? stop - next : 64u);
            const uint32_t take = nIdle < avail ? nIdle : avail;
            const uint32_t rank = lane_rank(idle);
            bool fin = false;
            if (!live && rank < take) {
                slot = (uint32_t) (next + rank); // (slots <= INT32_MAX)
                colour = RTD_WHITE; nv = 0; bounces = 0; albedo = 0u;
                bool made;
                if (camera) {
                    entry = slot / (uint32_t) q.n_samples;
                    const uint32_t s = (uint32_t) q.sample_first + (slot - entry * (uint32_t) q.n_samples);
                    const uint32_t g = q.pixel_list ? (uint32_t) q.pixel_list[entry] : entry;
                    const uint32_t r = g / (uint32_t) q.cols, c = g - r * (uint32_t) q.cols;
                    rng = stream_for(pixel_key(q.seed_key, (uint64_t) g), s);
                    made = camera_ray(*q.cam, q.max_h - (int) r - 1, (int) c - q.max_w, rng, o, d); // Scene.traceOnce's ray (Scene.fs:129-143): GetTwo
                    if (q.first_ray) {
                        double *f = q.first_ray + (size_t) slot * 6;
                        f[0] = made ? o.x : nanv; f[1] = made ? o.y : nanv; f[2] = made ? o.z : nanv;
                        f[3] = made ? d.x : nanv; f[4] = made ? d.y : nanv; f[5] = made ? d.z : nanv;
                    }
                } else {
                    const double *r = q.rays + (size_t) slot * 6;
                    o = mk(r[0], r[1], r[2]);
                    if (q.rng) { const uint32_t *g = q.rng + (size_t) slot * 4; rng.x = g[0]; rng.y = g[1]; rng.z = g[2]; rng.w = g[3]; }
                    else rng = stream_for(pixel_key(q.seed_key, q.ray_base + slot), q.ray_sample);
                    made = unitise(mk(r[3], r[4], r[5]), d); // Ray.make' (Ray.fs:26-34)
                }
                if (made) live = true;
                else { d = mk(1.0, 0.0, 0.0); retire(PATH_NO_RAY, RTD_BLACK); fin = true; } // ValueNone: Black, no vertex, nothing more drawn
            }
            next += take;
            if (q.summary) path_summarise(q, fin, entry, 0, PATH_NO_RAY, 0u, RTD_BLACK);
        }
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) {
            if (next >= stop && exhausted) break;
            continue;
        }

        // ---- (b) Scene.hitObject (Scene.fs:62-91) for every live lane ----
        int obj = -1;
        double t = nanv;
        if constexpr (LDS) {
            // node_loop_lds32 is wave-cooperative: all 64 lanes enter it, the idle ones with an exhausted walk and an empty queue.  Every
            // ray here left Ray.make' or Reflection as a unit vector, which is what the `implied` shortcut of the leaf test asks for.
            Walk w;
            walk_begin(w, sc.first);
            if (!live) w.off = sc.end;
            const WalkCtx32 f = walk_ctx32(o, d, p.off.bmax);
            double bestF = __builtin_inf();
            const bool implied = p.off.box_implied != 0;
            uint32_t pend = 0u;
            for (;;) {
#ifdef RTD_STAGE_CLOCKS
                unsigned nTrips = 0u, nLanes = 0u;
                w.off = node_loop_lds32(w.off, pend, sc.end, 0, f, nTrips, nLanes);
#else
                w.off = node_loop_lds32(w.off, pend, sc.end, 0, f); // until no lane of the wave can step: walks exhausted or queues full
#endif
                if (__builtin_amdgcn_ballot_w64(pend != 0u) == 0ull) break;
                if (pend != 0u) leaf_test_object_exact<true>(sc, o, d, bestF, w, pend_pop(pend), implied);
            }
            if (live) unbounded_tests<true, false>(sc, o, d, w, cnt);
            obj = w.best; t = w.bestLen;
        } else {
            if (live) obj = hit_object<false, COUNT>(sc, o, d, t, cnt);
        }

        // ---- (c) the vertex: record, Hittable.Reflection, record; the lanes whose path ended retire ----
        bool fin = false;
        int end = PATH_MISS;
        uint32_t result = RTD_BLACK;
        if (live) {
            if (obj < 0) { retire(PATH_MISS, RTD_BLACK); fin = true; }
            else {
                const V3 sp = walk(o, d, t); // Ray.walkAlong ray bestLength (Scene.fs:91)
                if (COUNT) cnt.refl++;
                const bool absorbed = reflection<LDS, TEX>(sc, obj, sp, o, d, colour, rng);
                if ((uint32_t) nv < K) {
                    const size_t r = (size_t) slot * K + (uint32_t) nv;
                    if (q.hit_index) q.hit_index[r] = q.obj_to_orig[obj];
                    if (q.strike) { q.strike[r * 3] = sp.x; q.strike[r * 3 + 1] = sp.y; q.strike[r * 3 + 2] = sp.z; }
                    if (q.colour_after) path_store_rgb(q.colour_after + r * 3, colour);
                    if (q.ray_after) {
                        double *a = q.ray_after + r * 6;
                        a[0] = absorbed ? nanv : o.x; a[1] = absorbed ? nanv : o.y; a[2] = absorbed ? nanv : o.z;
                        a[3] = absorbed ? nanv : d.x; a[4] = absorbed ? nanv : d.y; a[5] = absorbed ? nanv : d.z;
                    }
                }
                if (nv == 0) albedo = colour;
                nv = nv + 1;
                if (absorbed) { end = PATH_STOPPED; result = colour; retire(end, result); fin = true; }
                else {
                    bounces = bounces + 1;
                    if (bounces > q.depth) { end = PATH_BOUNCE_LIMIT; result = RTD_HOTPINK; retire(end, result); fin = true; }
                }
            }
        }
        if (q.summary) path_summarise(q, fin, entry, nv, end, albedo, result);
    }

    if (COUNT) {
        const uint64_t a = wave_sum_u64(cnt.rays), b = wave_sum_u64(cnt.aabb), c = wave_sum_u64(cnt.prim), dd = wave_sum_u64(cnt.refl);
        if (lane == 0) {
            atomicAdd(&q.counters[0], (unsigned long long) a);
            atomicAdd(&q.counters[1], (unsigned long long) b);
            atomicAdd(&q.counters[2], (unsigned long long) c);
            atomicAdd(&q.counters[3], (unsigned long long) dd);
        }
    }
}

} // namespace rtd
