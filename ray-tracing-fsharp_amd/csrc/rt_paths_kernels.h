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
#include "rt_paths_body.inc"
}
// ... for a scene that holds a texture program (RT_TEXTURE_PROGRAM): reflection<LDS, 2> evaluates it (texture_colour_at_prog); a symbol of its own
template <bool LDS, bool COUNT, int BLOCK>
__global__ void __launch_bounds__(BLOCK) paths_prog_kernel(const RenderParams p, const PathParams q) {
    constexpr int TEX = 2;
#include "rt_paths_body.inc"
}

} // namespace rtd
