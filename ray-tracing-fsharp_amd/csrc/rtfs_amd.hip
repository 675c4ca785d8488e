// rtfs_amd.hip -- C ABI entry points of librtfs_amd.so (declared in include/rtfs_amd.h).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see Makefile).
// There is NO CPU fallback: every compute entry point returns RT_ERR_NO_DEVICE when no HIP device is visible.
#include "../../include/rtfs_amd.h"
#include "rt_device.h"
#include "rt_job_kernels.h"
#include "rt_job_plan.h"
#include "rt_jpeg_kernels.h"
#include "rt_launch_plan.h"
#include "rt_output.h"
#include "rt_paths_kernels.h"
#include "rt_paths_plan.h"
#include "rt_pixel_map_kernels.h"
#include "rt_png_kernels.h"
#include "rt_render_kernel.h"
#include "rt_scene.h"
#include "rt_scene_kernels.h"
#include "rt_scene_plan.h"
#include "rt_surface_kernels.h"
#include "rt_surface_plan.h"
#include "rt_texture_kernels.h"
#include "rt_texture_plan.h"
#include "rt_tree_kernels.h"
#include "rt_tree_plan.h"
#include "rt_walk_kernels.h"
#include "rt_walk_plan.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <system_error>
#include <tuple>
#include <utility>
#include <vector>

using namespace rtd;

// ------------------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) noexcept {
    try { g_err = msg; } catch (...) { g_err.clear(); } // (no memory left for the message: the code still tells)
    return code;
}
#define HIP_TRY(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) return fail(RT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));               \
    } while (0)
#define RT_TRY(expr) /* a step that has already called fail(): its code is the caller's */                              \
    do {                                                                                                                \
        const int rc_ = (expr);                                                                                         \
        if (rc_ != RT_OK) return rc_;                                                                                   \
    } while (0)

// No exception crosses the C boundary: an entry point that fills host containers or starts threads runs its body through
// this, and whatever escapes it -- std::bad_alloc, std::system_error from a thread that could not be started -- becomes
// RT_ERR_HOST (`err`: the value the entry point returns for it).
template <class R = int, class F> static R guarded(const char *entry, F &&body, R err = RT_ERR_HOST) noexcept {
    const char *why = "host resources exhausted";
    try {
        return body();
    } catch (const std::bad_alloc &) {
        why = "host memory exhausted";
    } catch (const std::system_error &) {
        why = "host resources exhausted (a thread could not be started)";
    } catch (...) {
    }
    try { g_err = std::string(entry) + ": " + why; } catch (...) { g_err.clear(); }
    return err;
}

static int visible_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void) hipGetLastError(); return 0; }
    return n;
}
// Makes `device` current for the lifetime of the guard and puts the caller's device back afterwards (a torch caller that
// renders on another device than its current one must not find its later work redirected).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int enter(int device) {
        const int n = visible_devices();
        if (n <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible: the render path has no CPU fallback");
        if (device < 0 || device >= n) return fail(RT_ERR_INVALID_ARGUMENT, "device index out of range");
        if (hipGetDevice(&prev) != hipSuccess) { (void) hipGetLastError(); prev = -1; }
        if (prev != device) {
            hipError_t e = hipSetDevice(device);
            if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
            switched = true;
        }
        return RT_OK;
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void) hipSetDevice(prev); }
};

// ------------------------------------------------------------------------------------------------------------
// scene handle: host image + lazily created per-device copies
// ------------------------------------------------------------------------------------------------------------
struct DeviceScene {
    unsigned char *image = nullptr;
    TexRec *tex = nullptr;
    uint8_t *texels = nullptr;
    int32_t *obj_to_orig = nullptr; // HostScene::objToOrig (the ray-list hit queries answer in rt_scene_create's indices)
    int32_t *orig_to_obj = nullptr; // its inverse, made on the device by the first surface query (surface_inverse_map); freed with the scene
    int cu_count = 0;
};

// What rt_scene_create_device leaves on its device instead of filling HostScene's arrays: one allocation with the records, both trees
// (prim = rank) and the leaf boxes by rank.  ensure_host_mirror fetches them once, with the image and the object table of that device's
// DeviceScene, and frees the allocation.
struct MirrorSource {
    int device = -1;
    unsigned char *keep = nullptr;
    size_t n = 0, nb = 0, nn = 0;
    size_t records_at = 0, tree_at[3] = {0, 0, 0}, walk_at[3] = {0, 0, 0}, leaf_at = 0; // skip, prim, boxes
};
struct rt_scene {
    rth::HostScene host;
    std::map<int, DeviceScene> dev;
    std::mutex mu;
    std::atomic<bool> mirrored{true}; // false: host.hittables, tree, walkTree, leafBoxes, objToOrig, origToObj and image are still on src.device
                                      // (src.keep set), or host.texelBlob is still on texDevice (texelsOnHost false), or both
    MirrorSource src;
    bool texelsOnHost = true; // false: host.texelBlob is empty and the host.texelBytes bytes are dev[texDevice].texels (the rt_scene_create_*textures
    int texDevice = -1;       // routes, and any scene after rt_scene_set_texels_device); ensure_host_mirror fetches them
};
static int ensure_host_mirror_locked(rt_scene *s); // (s->mu held)
static int ensure_host_mirror(const rt_scene *scene) {
    rt_scene *s = const_cast<rt_scene *>(scene);
    if (s->mirrored.load(std::memory_order_acquire)) return RT_OK;
    std::lock_guard<std::mutex> lock(s->mu);
    return ensure_host_mirror_locked(s);
}

// Process-wide DEFAULTS of the launch settings (rt_set_*): read once per call, and only for the rt_render_options fields a
// caller leaves at 0.
static std::atomic<int> g_block_threads{0}, g_chunk_pixels{0}, g_blocks_per_cu{0}, g_yield_lanes{0}, g_refill_lanes{0};
static std::atomic<int> g_passes{0}; // 0 auto, 1 fused kernel, 2 two-pass (A, sort, B)
static std::atomic<int> g_park_lanes{0};
static std::atomic<int> g_walk_tree{RT_WALK_TREE_SAH};
static thread_local unsigned long long g_last_stage_stats[16] = {0};
static thread_local int64_t g_last_launch_plan[RT_LAUNCH_PLAN_WORDS] = {0};
static thread_local int64_t g_last_paths_plan[8] = {0};
static thread_local int64_t g_last_surface_plan[8] = {0};
// rt_dev_last_texture_plan: [0..4] of this thread's last rt_scene_create_*textures call; [5..7] (kernel launches, texel bytes host->device,
// texel bytes device->host) count on from it through rt_scene_set_texels_device and the lazy fetch of the texels
static thread_local int64_t g_last_texture_plan[8] = {0};

// (s->mu held, `device` current.)  placed: the scene's texel blob already on `device` (the scene's to free once this has succeeded), or NULL:
// uploaded from the host's.
static int device_scene_locked(rt_scene *s, int device, DeviceScene **out, uint8_t *placed = nullptr) {
    auto it = s->dev.find(device);
    if (it != s->dev.end()) { *out = &it->second; return RT_OK; }
    if (!placed) RT_TRY(ensure_host_mirror_locked(s)); // (a scene made on another device: its image and its texels come through the host)
    DeviceScene d;
    const rth::HostScene &h = s->host;
    HIP_TRY(hipMalloc((void **) &d.image, h.image.size()));
    HIP_TRY(hipMemcpy(d.image, h.image.data(), h.image.size(), hipMemcpyHostToDevice));
    if (!h.texRecs.empty()) {
        HIP_TRY(hipMalloc((void **) &d.tex, h.texRecs.size() * sizeof(TexRec)));
        HIP_TRY(hipMemcpy(d.tex, h.texRecs.data(), h.texRecs.size() * sizeof(TexRec), hipMemcpyHostToDevice));
    }
    if (placed) d.texels = placed;
    else if (!h.texelBlob.empty()) {
        HIP_TRY(hipMalloc((void **) &d.texels, h.texelBlob.size()));
        HIP_TRY(hipMemcpy(d.texels, h.texelBlob.data(), h.texelBlob.size(), hipMemcpyHostToDevice));
    }
    if (!h.objToOrig.empty()) {
        HIP_TRY(hipMalloc((void **) &d.obj_to_orig, h.objToOrig.size() * sizeof(int32_t)));
        HIP_TRY(hipMemcpy(d.obj_to_orig, h.objToOrig.data(), h.objToOrig.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    d.cu_count = prop.multiProcessorCount;
    try {
        *out = &s->dev.emplace(device, d).first->second;
    } catch (const std::bad_alloc &) {
        (void) hipFree(d.image); (void) hipFree(d.tex); if (!placed) (void) hipFree(d.texels); (void) hipFree(d.obj_to_orig);
        return fail(RT_ERR_HOST, "host memory exhausted");
    }
    return RT_OK;
}
static int device_scene(rt_scene *s, int device, DeviceScene **out) {
    std::lock_guard<std::mutex> lock(s->mu);
    return device_scene_locked(s, device, out);
}

// ------------------------------------------------------------------------------------------------------------
// launch plan: ONE place decides block size, unit sizes, LDS residency, the number of passes, the grids and the workspace sizes --
// rt_launch_plan.h, plain C++ over plain integers (tests/test_launch_plan.py runs it on a CPU).  enqueue() launches what it lists
// and rt_scene_get_info reports from it, so the two cannot disagree.  Here: only how its inputs are gathered.
// ------------------------------------------------------------------------------------------------------------
using rtp::Settings;
using rtp::check_settings;
static Settings resolve_settings(const rt_render_options *o) {
    rt_render_options v{};
    if (o) memcpy(&v, o, o->struct_size < sizeof(v) ? o->struct_size : sizeof(v));
    Settings s;
    s.block = v.block_threads ? v.block_threads : g_block_threads.load();
    s.chunk = v.chunk_pixels ? v.chunk_pixels : g_chunk_pixels.load();
    s.blocks_per_cu = v.blocks_per_cu ? v.blocks_per_cu : g_blocks_per_cu.load();
    s.yield = v.yield_lanes ? v.yield_lanes : g_yield_lanes.load();
    s.refill = v.refill_lanes ? v.refill_lanes : g_refill_lanes.load();
    s.passes = v.passes ? v.passes : g_passes.load();
    s.park = v.park_lanes ? v.park_lanes : g_park_lanes.load();
    return s;
}
static rtp::SceneSize scene_size(const rth::HostScene &h) {
    rtp::SceneSize sc;
    sc.lds_total = h.off.lds_total; sc.lds32_total = h.off.lds32_total;
    sc.n_nodes = h.off.n_nodes;
    sc.n_objects = h.nBounded + h.nUnbounded;
    sc.tex = !h.texRecs.empty();
    sc.prog = h.hasPrograms;
    return sc;
}
// The decision a timed render with default options takes (rt_scene_info.lds_resident, the pixel_candidates hook)
static bool default_lds_resident(const rth::HostScene &h) { return rtp::lds_resident(scene_size(h), resolve_settings(nullptr), false); }

// ------------------------------------------------------------------------------------------------------------
// launch
// ------------------------------------------------------------------------------------------------------------
typedef void (*render_fn)(const RenderParams);

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the FUNCTION, which every thread of the process shares: set per launch
// to that launch's own size, another thread could lower it between the setting and the launch.  It is set once per (function,
// device), to the most any launch may ask for -- the LDS budget less the function's static LDS; a launch's occupancy and grid
// still come from its own size (hipOccupancyMaxActiveBlocksPerMultiprocessor takes it explicitly).
static int allow_full_lds(const void *fn) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int device = -1;
    HIP_TRY(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({fn, device})) return RT_OK;
    hipFuncAttributes a{};
    HIP_TRY(hipFuncGetAttributes(&a, fn));
    if (a.sharedSizeBytes >= RT_LDS_BYTES) return fail(RT_ERR_HIP, "kernel's static LDS fills the budget");
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) (RT_LDS_BYTES - a.sharedSizeBytes)));
    try { done.insert({fn, device}); } catch (const std::bad_alloc &) {} // (set again next time)
    return RT_OK;
}
// The SET of instantiated render_kernel<...> is part of the build (compile time, code size): rtmode::is_built (rt_modes.h) says which
// (mode, block, tex) exist.  The plan never asks for one of the others; if it did, the launch fails (no kernel is substituted).
template <bool LDS, bool COUNT, int BLOCK, int MODE, bool TEX> static render_fn kernel_if_built() {
    if constexpr (rtmode::is_built(MODE, BLOCK, TEX)) return render_kernel<LDS, COUNT, BLOCK, MODE, TEX>;
    else return nullptr;
}
template <int BLOCK, int MODE, bool TEX> static render_fn pick_variant(bool lds, bool count) {
    if (lds) return count ? kernel_if_built<true, true, BLOCK, MODE, TEX>() : kernel_if_built<true, false, BLOCK, MODE, TEX>();
    return count ? kernel_if_built<false, true, BLOCK, MODE, TEX>() : kernel_if_built<false, false, BLOCK, MODE, TEX>();
}
template <int MODE, bool TEX> static render_fn pick_mode(const rtp::Pass &q) {
    return q.block == 1024 ? pick_variant<1024, MODE, TEX>(q.lds, q.count) : q.block == 768 ? pick_variant<768, MODE, TEX>(q.lds, q.count) :
           q.block == 512  ? pick_variant<512, MODE, TEX>(q.lds, q.count)  : pick_variant<256, MODE, TEX>(q.lds, q.count);
}
// q.mode against every mode of the table in turn.  tex: the scene has parameterised textures (otherwise the variant compiled without
// the texture call: no scratch, no VGPR spills)
// ... and the variants with the arm of texture programs (q.prog: the scene holds one), rtmode::is_built_prog
template <bool LDS, bool COUNT, int BLOCK, int MODE> static render_fn prog_kernel_if_built() {
    if constexpr (rtmode::is_built_prog(MODE, BLOCK)) return render_prog_kernel<LDS, COUNT, BLOCK, MODE>;
    else return nullptr;
}
template <int BLOCK, int MODE> static render_fn pick_prog_variant(bool lds, bool count) {
    if (lds) return count ? prog_kernel_if_built<true, true, BLOCK, MODE>() : prog_kernel_if_built<true, false, BLOCK, MODE>();
    return count ? prog_kernel_if_built<false, true, BLOCK, MODE>() : prog_kernel_if_built<false, false, BLOCK, MODE>();
}
static_assert(rtmode::is_built_prog(rtmode::FRAME_FUSED, 256) && rtmode::is_built_prog(rtmode::FRAME_PASS_B, 1024) && !rtmode::is_built_prog(rtmode::FRAME_FUSED, 512) &&
              !rtmode::is_built_prog(rtmode::RAYS_HIT, 1024), "the program variants: blocks of 256 and 1024, the modes that shade (rt_launch_plan.h plans exactly these)");
template <int MODE> static render_fn pick_prog_mode(const rtp::Pass &q) { // (another block: nullptr, and the launch fails -- no kernel is substituted)
    return q.block == 1024 ? pick_prog_variant<1024, MODE>(q.lds, q.count) : q.block == 256 ? pick_prog_variant<256, MODE>(q.lds, q.count) : nullptr;
}
// ... and the kernels of a batch of views (q.views; render_views_kernel): the three frame passes, both variants, plain and textured, at
// blocks of 256 and 1024 -- 48 kernels.  Anything else (a texture program, another block): nullptr, and the launch fails
template <int BLOCK, int PASS, bool TEX> static render_fn pick_views_variant(bool lds, bool count) {
    if (lds) return count ? render_views_kernel<true, true, BLOCK, PASS, TEX> : render_views_kernel<true, false, BLOCK, PASS, TEX>;
    return count ? render_views_kernel<false, true, BLOCK, PASS, TEX> : render_views_kernel<false, false, BLOCK, PASS, TEX>;
}
template <int PASS> static render_fn pick_views_pass(const rtp::Pass &q) {
    if (q.block == 256) return q.tex ? pick_views_variant<256, PASS, true>(q.lds, q.count) : pick_views_variant<256, PASS, false>(q.lds, q.count);
    return q.tex ? pick_views_variant<1024, PASS, true>(q.lds, q.count) : pick_views_variant<1024, PASS, false>(q.lds, q.count);
}
// ... and the camera hits of such a batch (camera_hits_views_kernel): both variants at blocks of 256 and 1024 -- 8 kernels
template <int BLOCK> static render_fn pick_camera_hits_views(bool lds, bool count) {
    if (lds) return count ? camera_hits_views_kernel<true, true, BLOCK> : camera_hits_views_kernel<true, false, BLOCK>;
    return count ? camera_hits_views_kernel<false, true, BLOCK> : camera_hits_views_kernel<false, false, BLOCK>;
}
static render_fn pick_views_kernel(const rtp::Pass &q) {
    if (q.prog || (q.block != 256 && q.block != 1024)) return nullptr;
    if (q.mode == rtmode::CAMERA_HITS) return q.tex ? nullptr : q.block == 256 ? pick_camera_hits_views<256>(q.lds, q.count) : pick_camera_hits_views<1024>(q.lds, q.count);
    return q.mode == rtmode::FRAME_FUSED ? pick_views_pass<rtmode::FRAME_FUSED>(q) : q.mode == rtmode::FRAME_PASS_A ? pick_views_pass<rtmode::FRAME_PASS_A>(q) :
           q.mode == rtmode::FRAME_PASS_B ? pick_views_pass<rtmode::FRAME_PASS_B>(q) :
           q.mode == rtmode::FRAME_PASS_B_MAP ? pick_views_pass<rtmode::FRAME_PASS_B_MAP>(q) : nullptr; // (pass B of a batch's extension by map: 16 more)
}
template <int MODE = rtmode::FRAME_FUSED> static render_fn pick_kernel(const rtp::Pass &q) {
    if (MODE == rtmode::FRAME_FUSED && q.views) return pick_views_kernel(q);
    if constexpr (MODE < rtmode::MODE_COUNT)
        return q.mode == MODE ? (q.prog ? pick_prog_mode<MODE>(q) : q.tex ? pick_mode<MODE, true>(q) : pick_mode<MODE, false>(q)) : pick_kernel<MODE + 1>(q);
    else return nullptr;
}

// Per-launch scratch, stream-ordered (hipMallocAsync on the launch stream), RT_SCRATCH_BYTES of it; the launch's workspace (pass B's
// list, the park pools) follows.  The kernels reach it through RenderParams' pointers and index `counters` past its sixteen
// words (counters[20..31] is `stage`), so every member is pinned to the byte offset they use.
struct LaunchScratch {
    unsigned long long counters[16]; // rays, aabb, prim, refl, samples, pixels_early, -, first wave start; [8..13] stage executions, [14] wave lifetimes, [15] last wave end
    unsigned int queue, pad0;        // RenderParams::queue: next work unit of the fused kernel / pass A, next run of a ray list
    unsigned long long queue_b;      // pass B: next unassigned list entry
    unsigned int live_count;         // pass A -> B: number of pairs / list entries
    unsigned int ext_foreign, ext_malformed, pad1; // an extension: pixels whose Count the arguments do not explain (extend_list_kernel); 1 = nothing was continued (extend_seal_kernel)
                                                   // a pixel list: ext_foreign also counts entries outside the frame (pixel_list_check_kernel); 1 = nothing was rendered
    unsigned long long stage[12];    // counters[20..31]: slow stages, lanes in them, lanes parked, cycles in refill / slow / walk / shade;
                                     // diagnostic builds (RTD_STAGE_CLOCKS): cycles in loop / leaf / unbounded / new items / lambert
    CameraParams cam;                // RenderParams::cam_ptr
};
static_assert(offsetof(LaunchScratch, queue) == 128 && offsetof(LaunchScratch, queue_b) == 136 && offsetof(LaunchScratch, live_count) == 144, "queues");
static_assert(offsetof(LaunchScratch, ext_foreign) == 148 && offsetof(LaunchScratch, ext_malformed) == 152, "zeroed by launch_init_kernel with the queues");
static_assert(offsetof(LaunchScratch, stage) == 20 * sizeof(unsigned long long) && offsetof(LaunchScratch, stage) == 160, "stage counters are counters[20..31]");
static_assert(offsetof(LaunchScratch, cam) == 256 && sizeof(LaunchScratch) <= RT_SCRATCH_BYTES, "camera must fit the scratch slot");

// Zeroes a launch's counters and queues and writes its camera: one tiny launch instead of a memset plus a copy from
// pageable host memory (which may block the host until earlier work on the stream has finished).
__global__ void launch_init_kernel(unsigned char *scratch, const CameraParams cam) {
    if (threadIdx.x < (unsigned) (offsetof(LaunchScratch, cam) / 4)) ((unsigned int *) scratch)[threadIdx.x] = 0u; // everything in front of the camera
    if (threadIdx.x == 0) *(CameraParams *) (scratch + offsetof(LaunchScratch, cam)) = cam;
}
static_assert(offsetof(LaunchScratch, cam) / 4 <= 64, "launch_init_kernel runs 64 threads");

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char *rt_last_error(void) { return g_err.c_str(); }
int rt_device_count(void) { return visible_devices(); }

size_t rt_abi_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(rt_hittable);
    case 1: return sizeof(rt_texture);
    case 2: return sizeof(rt_camera);
    case 3: return sizeof(rt_scene_info);
    case 4: return sizeof(rt_stats);
    case 5: return sizeof(rt_render_options);
    case 6: return sizeof(rt_scene_options);
    case 7: return sizeof(rt_tune_info);
    case 9: return sizeof(rt_path_outputs); // (8 stays unused: bindings probe it as "no such struct")
    case 10: return sizeof(rt_jpeg_info);
    case 11: return sizeof(rt_jpeg_stats);
    case 12: return sizeof(rt_texels_source);
    case 13: return sizeof(rt_surface_outputs);
    default: return 0;
    }
}

size_t rt_abi_offsetof(int which, int field) {
#define RT_OFFS(T, ...) { static const size_t o[] = {__VA_ARGS__}; return (field >= 0 && (size_t) field < sizeof(o) / sizeof(o[0])) ? o[field] : (size_t) -1; }
#define F(T, m) offsetof(T, m)
    switch (which) {
    case 0: RT_OFFS(rt_hittable, F(rt_hittable, kind), F(rt_hittable, style), F(rt_hittable, point), F(rt_hittable, normal), F(rt_hittable, radius),
                    F(rt_hittable, albedo), F(rt_hittable, fuzz), F(rt_hittable, ior), F(rt_hittable, prob), F(rt_hittable, rgb), F(rt_hittable, reserved),
                    F(rt_hittable, texture))
    case 1: RT_OFFS(rt_texture, F(rt_texture, kind), F(rt_texture, rgb), F(rt_texture, ramp_src), F(rt_texture, reserved), F(rt_texture, even),
                    F(rt_texture, odd), F(rt_texture, grid_size), F(rt_texture, width), F(rt_texture, height), F(rt_texture, texels),
                    F(rt_texture, map_centre), F(rt_texture, map_radius))
    case 2: RT_OFFS(rt_camera, F(rt_camera, view_origin), F(rt_camera, view_dir), F(rt_camera, xaxis_origin), F(rt_camera, xaxis_dir),
                    F(rt_camera, yaxis_origin), F(rt_camera, yaxis_dir), F(rt_camera, viewport_width), F(rt_camera, viewport_height),
                    F(rt_camera, focal_length), F(rt_camera, samples_per_pixel), F(rt_camera, bounce_depth))
    case 3: RT_OFFS(rt_scene_info, F(rt_scene_info, n_bounded), F(rt_scene_info, n_unbounded), F(rt_scene_info, n_nodes), F(rt_scene_info, tree_depth),
                    F(rt_scene_info, n_textures), F(rt_scene_info, lds_resident), F(rt_scene_info, walk_tree), F(rt_scene_info, walk_tree_depth),
                    F(rt_scene_info, scene_bytes), F(rt_scene_info, texel_bytes), F(rt_scene_info, walk_tree_nodes), F(rt_scene_info, leaf_box_implied))
    case 4: RT_OFFS(rt_stats, F(rt_stats, rays), F(rt_stats, aabb_tests), F(rt_stats, prim_tests), F(rt_stats, reflections), F(rt_stats, samples),
                    F(rt_stats, pixels), F(rt_stats, pixels_early), F(rt_stats, kernel_ms), F(rt_stats, total_ms))
    case 5: RT_OFFS(rt_render_options, F(rt_render_options, struct_size), F(rt_render_options, block_threads), F(rt_render_options, chunk_pixels),
                    F(rt_render_options, blocks_per_cu), F(rt_render_options, yield_lanes), F(rt_render_options, refill_lanes),
                    F(rt_render_options, passes), F(rt_render_options, park_lanes))
    case 6: RT_OFFS(rt_scene_options, F(rt_scene_options, struct_size), F(rt_scene_options, walk_tree))
    case 7: RT_OFFS(rt_tune_info, F(rt_tune_info, struct_size), F(rt_tune_info, tuned), F(rt_tune_info, probe_rows), F(rt_tune_info, probe_rays),
                    F(rt_tune_info, nodes_before), F(rt_tune_info, nodes_after), F(rt_tune_info, box_tests_before), F(rt_tune_info, box_tests_after),
                    F(rt_tune_info, probe_ms), F(rt_tune_info, build_ms))
    case 9: RT_OFFS(rt_path_outputs, F(rt_path_outputs, struct_size), F(rt_path_outputs, max_vertices), F(rt_path_outputs, n_vertices), F(rt_path_outputs, end),
                    F(rt_path_outputs, colour), F(rt_path_outputs, first_ray), F(rt_path_outputs, hit_index), F(rt_path_outputs, strike),
                    F(rt_path_outputs, colour_after), F(rt_path_outputs, ray_after), F(rt_path_outputs, summary))
    case 13: RT_OFFS(rt_surface_outputs, F(rt_surface_outputs, struct_size), F(rt_surface_outputs, normal), F(rt_surface_outputs, inside),
                     F(rt_surface_outputs, colour), F(rt_surface_outputs, tint), F(rt_surface_outputs, uv))
    default: return (size_t) -1;
    }
#undef F
#undef RT_OFFS
}

int rt_texture_program_check(const uint8_t *program, size_t n) {
    int where = -1;
    const int why = rtxp::check(program, n, &where);
    if (why == rtxp::OK) return RT_OK;
    return fail(RT_ERR_INVALID_ARGUMENT, std::string("program: ") + (where >= 0 ? (why == rtxp::NONFINITE_CONST ? "constant " : "instruction ") + std::to_string(where) + ": " : std::string()) +
                                             rtxp::reason_text(why));
}

int rt_set_launch_config(int32_t block_threads, int32_t chunk_pixels, int32_t blocks_per_cu) {
    Settings s{block_threads, chunk_pixels, blocks_per_cu, 0, 0, 0, 0};
    if (const char *m = check_settings(s)) return fail(RT_ERR_INVALID_ARGUMENT, m);
    g_block_threads = block_threads;
    g_chunk_pixels = chunk_pixels;
    g_blocks_per_cu = blocks_per_cu;
    return RT_OK;
}

int rt_last_stage_stats(uint64_t out[16]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int i = 0; i < 16; ++i) out[i] = g_last_stage_stats[i];
    return RT_OK;
}

int rt_dev_last_launch_plan(int64_t out[RT_LAUNCH_PLAN_WORDS]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int i = 0; i < RT_LAUNCH_PLAN_WORDS; ++i) out[i] = g_last_launch_plan[i];
    return RT_OK;
}

int rt_set_walk_tree(int32_t kind) {
    if (kind != RT_WALK_TREE_SAH && kind != RT_WALK_TREE_REFERENCE) return fail(RT_ERR_INVALID_ARGUMENT, "walk tree must be RT_WALK_TREE_SAH or RT_WALK_TREE_REFERENCE");
    g_walk_tree = kind;
    return RT_OK;
}
int rt_set_passes(int32_t passes) {
    if (const char *m = check_settings(Settings{0, 0, 0, 0, 0, passes, 0})) return fail(RT_ERR_INVALID_ARGUMENT, m);
    g_passes = passes;
    return RT_OK;
}
int rt_set_park(int32_t park_lanes) {
    if (const char *m = check_settings(Settings{0, 0, 0, 0, 0, 0, park_lanes})) return fail(RT_ERR_INVALID_ARGUMENT, m);
    g_park_lanes = park_lanes;
    return RT_OK;
}

int rt_set_schedule(int32_t yield_lanes, int32_t refill_lanes) {
    if (const char *m = check_settings(Settings{0, 0, 0, yield_lanes, refill_lanes, 0, 0})) return fail(RT_ERR_INVALID_ARGUMENT, m);
    g_yield_lanes = yield_lanes;
    g_refill_lanes = refill_lanes;
    return RT_OK;
}

int rt_camera_make_basic(int32_t spp, double focal, double aspect, const double origin[3], const double view_direction[3],
                         const double view_up[3], rt_camera *out) {
    if (!origin || !view_direction || !view_up || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!rth::camera_make_basic(spp, focal, aspect, origin, view_direction, view_up, out))
        return fail(RT_ERR_INVALID_ARGUMENT, "degenerate camera frame (the reference's ValueOption.get would throw)");
    return RT_OK;
}

int rt_scene_create_ex(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                       const rt_scene_options *options, rt_scene **out) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    int walk = -1;
    if (options && options->struct_size >= offsetof(rt_scene_options, walk_tree) + sizeof(int32_t)) walk = options->walk_tree;
    if (walk == -1) walk = g_walk_tree.load();
    if (walk != RT_WALK_TREE_SAH && walk != RT_WALK_TREE_REFERENCE) return fail(RT_ERR_INVALID_ARGUMENT, "walk_tree must be RT_WALK_TREE_SAH, RT_WALK_TREE_REFERENCE or -1");
    return guarded("rt_scene_create", [&]() {
        std::unique_ptr<rt_scene> s(new rt_scene());
        int status = RT_OK;
        std::string msg = rth::build_scene(hittables, n_hittables, textures, n_textures, walk, s->host, status);
        if (status != RT_OK) return fail(status, msg);
        *out = s.release();
        return (int) RT_OK;
    });
}
int rt_scene_create(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures, rt_scene **out) {
    return rt_scene_create_ex(hittables, n_hittables, textures, n_textures, nullptr, out);
}

void rt_scene_destroy(rt_scene *s) {
    if (!s) return;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) { (void) hipGetLastError(); prev = -1; }
    for (auto &kv : s->dev) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        (void) hipFree(kv.second.image);
        (void) hipFree(kv.second.tex);
        (void) hipFree(kv.second.texels);
        (void) hipFree(kv.second.obj_to_orig);
        (void) hipFree(kv.second.orig_to_obj);
    }
    if (s->src.keep && hipSetDevice(s->src.device) == hipSuccess) (void) hipFree(s->src.keep);
    if (prev >= 0 && (!s->dev.empty() || s->src.keep)) (void) hipSetDevice(prev);
    delete s;
}

int rt_scene_get_info(const rt_scene *s, rt_scene_info *out) {
    if (!s || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    const rth::HostScene &h = s->host;
    out->n_bounded = h.off.n_bounded;
    out->n_unbounded = h.off.n_unbounded;
    out->n_nodes = (int32_t) rtt::node_count(h.nBounded); // (= tree.skip.size(), which a scene made on the device fills only with its host mirror)
    out->walk_tree_nodes = h.off.n_nodes;
    out->leaf_box_implied = h.off.box_implied;
    out->tree_depth = h.tree.depth;
    out->walk_tree = h.walkKind;
    out->walk_tree_depth = h.walkTree.depth;
    out->n_textures = (int32_t) h.texRecs.size();
    out->lds_resident = default_lds_resident(h) ? 1 : 0; // the decision a render with default options takes
    out->scene_bytes = (int64_t) h.off.total;
    out->texel_bytes = (int64_t) h.texelBytes; // (the blob itself may still be on a device)
    return RT_OK;
}

static int copy_tree(const rth::HostScene &h, const rth::FlatTree &t, int32_t *skip, int32_t *prim, double *boxes) {
    const size_t nn = t.skip.size();
    for (size_t i = 0; i < nn; ++i) {
        if (skip) skip[i] = t.skip[i];
        if (prim) prim[i] = t.prim[i] < 0 ? -1 : h.objToOrig[(size_t) t.prim[i]];
        if (boxes) for (int a = 0; a < 3; ++a) { boxes[i * 6 + (size_t) a * 2] = t.box[i].mn[a]; boxes[i * 6 + (size_t) a * 2 + 1] = t.box[i].mx[a]; }
    }
    return RT_OK;
}
int rt_scene_get_tree(const rt_scene *s, int32_t *skip, int32_t *prim, double *boxes) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "NULL scene");
    RT_TRY(ensure_host_mirror(s));
    return copy_tree(s->host, s->host.tree, skip, prim, boxes);
}
int rt_scene_get_walk_tree(const rt_scene *s, int32_t *skip, int32_t *prim, double *boxes) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "NULL scene");
    RT_TRY(ensure_host_mirror(s));
    return copy_tree(s->host, s->host.walkTree, skip, prim, boxes);
}

int rt_scene_get_filter_tree(const rt_scene *s, float *boxes, int32_t *links) {
    if (!s) return fail(RT_ERR_INVALID_ARGUMENT, "NULL scene");
    if (!boxes || !links) return fail(RT_ERR_INVALID_ARGUMENT, "NULL output");
    RT_TRY(ensure_host_mirror(s));
    const rth::HostScene &h = s->host;
    const unsigned char *sec = h.image.data() + h.off.node32;
    for (int32_t p = 0; p < h.off.n_nodes; ++p) {
        const float *fx = (const float *) (sec + (size_t) p * RTD_NODE32_BYTES);
        const int32_t *lk = (const int32_t *) (sec + (size_t) p * RTD_NODE32_BYTES + 48);
        for (int a = 0; a < 3; ++a) { boxes[(size_t) p * 6 + 2 * a] = fx[a * 4]; boxes[(size_t) p * 6 + 2 * a + 1] = fx[a * 4 + 1]; }
        const uint32_t e = (uint32_t) lk[2];
        const uint32_t obj = (e & RTD_PEND_WIDE) ? (e & ~RTD_PEND_WIDE) : (e & (RTD_PEND_MARK - 1u));
        links[(size_t) p * 5 + 0] = lk[0] / RTD_NODE32_BYTES;
        links[(size_t) p * 5 + 1] = lk[1] / RTD_NODE32_BYTES;
        links[(size_t) p * 5 + 2] = lk[2];
        links[(size_t) p * 5 + 3] = lk[3];
        links[(size_t) p * 5 + 4] = e == 0u ? -1 : (obj < h.objToOrig.size() ? h.objToOrig[obj] : -2);
    }
    return RT_OK;
}

// The argument checks more than one family of entry points makes, each stated once.  The first fault found decides the code and the
// text of rt_last_error(), so every check_* function below lists its pieces in the order its entry points have always tested them.
static int check_options(const rt_render_options *options) { // (null: the rt_set_* defaults, which are checked as well)
    if (options && options->struct_size < sizeof(uint32_t)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_options.struct_size is not set");
    if (const char *m = check_settings(resolve_settings(options))) return fail(RT_ERR_INVALID_ARGUMENT, m);
    return RT_OK;
}
static int check_spp(int32_t spp) {
    if (spp < 1) return fail(RT_ERR_INVALID_ARGUMENT, "samples_per_pixel must be >= 1");
    if (spp > 8000000) return fail(RT_ERR_INVALID_ARGUMENT, "samples_per_pixel too large for int32 sums (255*spp)");
    return RT_OK;
}
static int check_depth(int32_t bounce_depth) {
    if (bounce_depth < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bounce_depth must be >= 0");
    if (bounce_depth > 0xFFFFFF) return fail(RT_ERR_INVALID_ARGUMENT, "bounce_depth too large");
    return RT_OK;
}
static int check_count(size_t n, const char *what) { // a list of `what`: "rays", "footprints", "list entries"
    if (n > (size_t) INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, std::string("more than INT32_MAX ") + what);
    return RT_OK;
}
static int check_list_frame(int32_t max_w, int32_t max_h) { // a pixel list's entries are int32 indices into the frame
    if ((uint64_t) (2 * max_w + 1) * (uint64_t) (2 * max_h + 1) > (uint64_t) INT32_MAX)
        return fail(RT_ERR_INVALID_ARGUMENT, "a pixel list indexes frames of at most INT32_MAX pixels");
    return RT_OK;
}
static int check_extend_shard(int32_t max_w, int32_t n_rows) { // the extension's list of continued pixels holds uint32 indices
    if ((uint64_t) n_rows * (uint64_t) (2 * max_w + 1) >= (1ull << 32)) return fail(RT_ERR_INVALID_ARGUMENT, "an extension takes shards of fewer than 2^32 pixels");
    return RT_OK;
}

static int check_geometry(const rt_camera *camera, int32_t max_w, int32_t max_h, int32_t row_first, int32_t row_stride, int32_t n_rows) {
    if (!camera) return fail(RT_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (max_w <= 0 || max_h <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "max_width_coord and max_height_coord must be positive");
    if (max_w > (1 << 20) || max_h > (1 << 20)) return fail(RT_ERR_INVALID_ARGUMENT, "image too large");
    RT_TRY(check_spp(camera->samples_per_pixel));
    RT_TRY(check_depth(camera->bounce_depth));
    const int rows = 2 * max_h + 1;
    if (row_stride <= 0 || row_first < 0 || n_rows < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad row shard");
    if (n_rows > 0 && (int64_t) row_first + (int64_t) (n_rows - 1) * row_stride >= rows) return fail(RT_ERR_INVALID_ARGUMENT, "row shard exceeds the image");
    return RT_OK;
}
// A frame shard's checks: rt_render_device(_ex) and the frame extensions (`no_accum`: their texts for a missing buffer differ).
static int check_frame(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, int32_t row_first, int32_t row_stride, int32_t n_rows,
                       const void *accum, const char *no_accum, const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    RT_TRY(check_geometry(camera, max_w, max_h, row_first, row_stride, n_rows));
    if (n_rows > 0 && !accum) return fail(RT_ERR_INVALID_ARGUMENT, no_accum);
    return check_options(options);
}

} // extern "C"

struct RayLog { double *rays; unsigned int *count; uint32_t cap, mask; }; // rt_scene_tune's probe (RenderParams::ray_log)

// What a launch leaves behind when its statistics are wanted: events around the kernels and the launch's scratch, which
// then stays allocated until the counters have been read.
struct Pending {
    hipEvent_t a = nullptr, b = nullptr;
    unsigned char *scr = nullptr;
    hipStream_t st = nullptr;
    int device = -1;
    uint64_t pixels = 0, waves = 0;
    bool launched = false, keep = false;
    bool extend = false; // an extension: collect_stats reads LaunchScratch::ext_malformed
    bool map = false;    // ... by map (the message of a malformed buffer)
    bool list = false;   // a pixel list (of a render, or of camera hits): collect_stats reads ext_malformed for a fresh render too (an entry outside the frame)
    std::chrono::steady_clock::time_point t0;
    void release() { // events destroyed, scratch handed back to the stream's pool in stream order
        if (a) (void) hipEventDestroy(a);
        if (b) (void) hipEventDestroy(b);
        if (scr) (void) hipFreeAsync(scr, st);
        a = b = nullptr; scr = nullptr;
    }
    ~Pending() { release(); }
};

static CameraParams camera_params(const rt_camera *camera, int32_t max_w, int32_t max_h) {
    CameraParams c{};
    for (int a = 0; a < 3; ++a) {
        c.eye[a] = camera->view_origin[a];
        c.xo[a] = camera->xaxis_origin[a];
        c.xd[a] = camera->xaxis_dir[a];
        c.yd[a] = camera->yaxis_dir[a];
    }
    c.vw = camera->viewport_width;
    c.vh = camera->viewport_height;
    c.max_w = max_w; c.max_h = max_h;
    c.spp = camera->samples_per_pixel;
    c.depth = camera->bounce_depth;
    return c;
}
static void set_plan_fields(RenderParams &p, const rtp::Pass &q) {
    p.chunk = q.chunk;
    p.park = q.park; p.park_l = q.park_l; p.park_l_lds = q.park_l_lds;
    p.lds_node_bytes = q.lds_node_bytes; p.lds_node_thr = q.lds_node_thr;
    p.yield_lanes = q.yield_lanes; p.leaf_wait = q.leaf_wait; p.refill_lanes = q.refill_lanes;
    p.k = q.k;
    p.total_waves = q.total_waves;
}

// rt_dev_last_launch_plan: the plan enqueue() is about to execute, inputs and outputs, as plain integers in the order
// include/rtfs_amd.h gives (tests/c/launch_plan_table.cpp's names).  Host bookkeeping only: nothing that is launched reads it.
static void remember_plan(const rtp::LaunchPlan &pl, int per_cu) {
    int64_t *o = g_last_launch_plan;
    int n = 0;
    auto put = [&](int64_t v) { o[n++] = v; };
    const rtp::SceneSize &sc = pl.scene;
    const Settings &s = pl.set;
    const rtp::Job &j = pl.job;
    put(1);
    put(j.kind == rtp::Job::FRAME ? 0 : (j.kind == rtp::Job::TRACE ? 1 : (j.kind == rtp::Job::HIT ? 2 : (j.kind == rtp::Job::FOOTPRINTS ? 3 : (j.kind == rtp::Job::PIXELS ? 4 :
        (j.kind == rtp::Job::CAMERA_HITS ? (j.n_views ? 7 : 5) : 6))))));
    put((int64_t) sc.lds_total); put((int64_t) sc.lds32_total); put(sc.n_nodes); put((int64_t) sc.n_objects); put((int) sc.tex + (int) sc.prog);
    put(s.block); put(s.chunk); put(s.blocks_per_cu); put(s.yield); put(s.refill); put(s.passes); put(s.park);
    put(pl.one.count); put(j.ray_log); put((int64_t) j.n_rows); put(j.max_w); put(j.spp); put(j.views() ? (int64_t) j.n_views : (int64_t) j.n); put(pl.cu_count); put(per_cu);
    const rtp::Pass &q = pl.one;
    put(q.lds); put(q.count); put(q.block); put(q.mode); put((int) q.tex + (int) q.prog); put((int64_t) q.lds_bytes); put(pl.two_pass);
    put((int64_t) pl.pairs_bytes); put((int64_t) pl.list_bytes); put((int64_t) pl.sort_bytes); put((int64_t) pl.pool_bytes); put((int64_t) pl.waves);
    put(pl.error ? 1 : 0);
    for (const rtp::Pass *r : {&pl.one, &pl.a, &pl.b}) {
        put(r->mode); put((int64_t) r->grid); put((int64_t) r->lds_bytes); put(r->chunk); put(r->park); put(r->park_l); put(r->park_l_lds);
        put(r->lds_node_bytes); put(r->lds_node_thr); put(r->yield_lanes); put(r->leaf_wait); put(r->refill_lanes); put(r->k); put(r->total_waves);
    }
    put(j.first_sample); // [77]: 0 = a fresh render, else the samples_done of an extension (by map: RTD_EXTEND_MIN_DONE); camera hits: sample_first
    put(j.map ? 1 : 0);  // [78]: 1 = an extension by map
    put(j.camera_hits_views() ? (int64_t) j.n_views : 0); // [79]: the views of camera hits over a batch (kind 7: [19] is the list's n, as kind 5's)
    static_assert(1 + 21 + 13 + 3 * 14 + 3 <= RT_LAUNCH_PLAN_WORDS, "rt_dev_last_launch_plan's words");
    while (n < RT_LAUNCH_PLAN_WORDS) put(0);
}

// The one enqueue path of frames and ray lists (arguments checked, settings valid): plans the launch, takes its scratch and workspace
// from the stream's pool, launches what the plan lists -- one kernel, or pass A, the three sort kernels and pass B -- and never waits
// for the device.  `p` arrives with the caller's own fields filled (camera and rows and buffers, or the ray list's pointers); the
// scene's and the plan's are set here.  With want_stats the launch is bracketed by events and its scratch is kept in `pd` for
// collect_stats.
// A batch of views (job.kind == VIEWS, or CAMERA_HITS with n_views >= 1): the per-view cameras and seed keys, which get a section of their own behind the workspace.
struct ViewsArgs { std::vector<CameraParams> cams; std::vector<uint64_t> keys; };
static int enqueue(const rt_scene *scene, int32_t device, const rtp::Job &job, const Settings &set, uint32_t flags, void *stream, RenderParams p,
                   const CameraParams &cam, bool want_stats, Pending &pd, const ViewsArgs *views = nullptr) {
    DeviceGuard guard;
    int rc = guard.enter(device);
    if (rc != RT_OK) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    DeviceScene *ds = nullptr;
    rc = device_scene(const_cast<rt_scene *>(scene), device, &ds);
    if (rc != RT_OK) return rc;
    const rth::HostScene &h = scene->host;
    hipStream_t st = (hipStream_t) stream;
    p.off = h.off;
    p.scene_image = ds->image;
    p.tex = ds->tex;
    p.texels = ds->texels;
    p.obj_to_orig = ds->obj_to_orig; // (read by the hit queries only)

    rtp::LaunchPlan plan = rtp::plan_begin(scene_size(h), set, (flags & RT_RENDER_COUNTERS) != 0, job, ds->cu_count);
    const int block = plan.one.block;
    const size_t ldsBytes = plan.one.lds_bytes;
    render_fn fn = pick_kernel(plan.one);
    if (!fn) return fail(RT_ERR_HIP, "no kernel is built for this launch");
    rc = allow_full_lds((const void *) fn);
    if (rc != RT_OK) return rc;
    // the one device answer the plan needs: asked once, for the fused (or ray-list) kernel at its own LDS size; both passes of a
    // two-pass launch use the grid that follows from it
    int perCu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, (const void *) fn, block, ldsBytes));
    if (perCu < 1) return fail(RT_ERR_HIP, job.pixels() ? "render kernel does not fit on a CU (occupancy 0)" : "ray-list kernel does not fit on a CU (occupancy 0)");
    rtp::plan_finish(plan, perCu);
    remember_plan(plan, perCu);
    const uint64_t grid = plan.one.grid;
    const size_t pairsBytes = plan.pairs_bytes, listBytes = plan.list_bytes, sortBytes = plan.sort_bytes, poolBytes = plan.pool_bytes;
    const size_t viewsBytes = views ? views->cams.size() * (sizeof(CameraParams) + sizeof(uint64_t)) : 0u;

    // Everything below is stream-ordered: scratch and workspace come from the stream's pool and go back to it after the last
    // launch that uses them, so no launch shares state with another and the call returns without waiting for the device.
    unsigned char *scr = nullptr;
    if (grid > 0 || want_stats) HIP_TRY(hipMallocAsync((void **) &scr, RT_SCRATCH_BYTES + pairsBytes + listBytes + sortBytes + poolBytes + viewsBytes, st));
    Pending &cl = pd; // on every exit path its destructor (or collect_stats) gives the scratch back
    cl.scr = scr; cl.st = st; cl.device = device; cl.t0 = t0;
    cl.pixels = plan.pixels;
    cl.waves = plan.waves;
    cl.extend = job.extend();
    cl.map = job.map;
    const bool checked_list = job.kind == rtp::Job::PIXELS || (job.kind == rtp::Job::CAMERA_HITS && p.pixel_list != nullptr);
    cl.list = checked_list;
    if (want_stats) {
        HIP_TRY(hipEventCreate(&cl.a));
        HIP_TRY(hipEventCreate(&cl.b));
    }
    if (scr) {
        LaunchScratch *ls = (LaunchScratch *) scr;
        p.counters = ls->counters;
        p.queue = &ls->queue;
        p.queue_b = &ls->queue_b;
        p.live_count = &ls->live_count;
        p.cam_ptr = &ls->cam;
        p.park_pool = scr + RT_SCRATCH_BYTES + pairsBytes + listBytes + sortBytes;
        hipLaunchKernelGGL(launch_init_kernel, dim3(1), dim3(64), 0, st, scr, cam);
        HIP_TRY(hipGetLastError());
    }
    if (views && grid > 0) { // the views' cameras and seed keys: behind the park pools (poolBytes is a multiple of 16)
        const size_t nv = views->cams.size();
        CameraParams *cams = (CameraParams *) (scr + RT_SCRATCH_BYTES + pairsBytes + listBytes + sortBytes + poolBytes);
        uint64_t *keys = (uint64_t *) (cams + nv);
        for (size_t at = 0; at < nv; at += VIEWS_INIT_CAMERAS) {
            ViewsInit vi{};
            vi.first = (uint32_t) at; vi.n = (uint32_t) (nv - at < (size_t) VIEWS_INIT_CAMERAS ? nv - at : (size_t) VIEWS_INIT_CAMERAS);
            for (uint32_t i = 0; i < vi.n; ++i) { vi.cam[i] = views->cams[at + i]; vi.key[i] = views->keys[at + i]; }
            hipLaunchKernelGGL(views_init_kernel, dim3(1), dim3(64), 0, st, cams, keys, vi);
        }
        HIP_TRY(hipGetLastError());
        p.view_cams = cams; p.view_keys = keys;
        p.n_views = (uint32_t) nv;
        p.view_pixels = job.camera_hits_views() ? (uint32_t) job.n : (uint32_t) job.view_pixels(); // (camera hits: the list's entries)
    }
    if (grid > 0) {
        if (want_stats) HIP_TRY(hipEventRecord(cl.a, st));
        if (checked_list) {
            // in front of everything else: is every entry a pixel of the frame?  An extension's own seal acts on the count; a fresh render
            // (and camera hits) gets a seal that poisons the unit counter, so that nothing is rendered and nothing written (rt_render_kernel.h)
            LaunchScratch *ls = (LaunchScratch *) scr;
            const unsigned long long want = (job.n + 255ull) / 256ull, most = (unsigned long long) ds->cu_count * 8ull;
            hipLaunchKernelGGL(pixel_list_check_kernel, dim3((unsigned) (want < most ? want : most)), dim3(256), 0, st, p.pixel_list, (unsigned long long) job.n,
                               (uint32_t) p.cols * (uint32_t) (2 * p.max_h + 1), &ls->ext_foreign);
            if (!job.extend()) hipLaunchKernelGGL(pixel_list_seal_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) &ls->ext_foreign, p.queue, &ls->ext_malformed);
            HIP_TRY(hipGetLastError());
        }
        if (job.extend()) {
            // pass B alone, from sample first_sample on: its list comes from the stored Counts (extend_list_kernel) instead of pass A
            // and the sort; the seal between them makes "malformed buffer => nothing written" hold (rt_render_kernel.h)
            if (plan.error || !plan.two_pass) return fail(RT_ERR_HIP, plan.error ? plan.error : "an extension needs a pass B");
            LaunchScratch *ls = (LaunchScratch *) scr;
            unsigned int *list = (unsigned int *) (scr + RT_SCRATCH_BYTES + pairsBytes);
            p.live_list = list;
            render_fn fb = pick_kernel(plan.b);
            if (!fb) return fail(RT_ERR_HIP, "no kernel is built for this launch");
            if ((rc = allow_full_lds((const void *) fb)) != RT_OK) return rc;
            set_plan_fields(p, plan.b);
            p.first_b = job.first_sample;
            const unsigned long long nLocal = plan.pixels; // (< 2^32: the plan's condition for a list)
            const unsigned long long want = (nLocal + 255ull) / 256ull, most = (unsigned long long) ds->cu_count * 8ull;
            const unsigned listGrid = (unsigned) (want < most ? want : most);
            if (views) {
                // a batch of views: the list builders of the batch write PAIRS (samples to add, batch pixel); the seal; then the batch's
                // ordering -- by view, inside a view longest job first -- which also fills view_end, what clips pass B's ranges.  A
                // sealed buffer has no pair: every key counts nothing, every view_end is 0, and pass B opens no range
                unsigned long long *pairs = (unsigned long long *) (scr + RT_SCRATCH_BYTES);
                unsigned int *sortBuf = (unsigned int *) (scr + RT_SCRATCH_BYTES + pairsBytes + listBytes);
                HIP_TRY(hipMemsetAsync(sortBuf, 0, sortBytes, st));
                p.pairs = pairs;
                if (job.map)
                    hipLaunchKernelGGL(views_extend_map_list_kernel, dim3(listGrid), dim3(256), 0, st, (const int32_t *) p.accum, p.ext_targets, nLocal, p.spp, pairs,
                                       p.live_count, p.counters, &ls->ext_foreign);
                else
                    hipLaunchKernelGGL(views_extend_list_kernel, dim3(listGrid), dim3(256), 0, st, (const int32_t *) p.accum, nLocal, job.first_sample, p.spp, pairs,
                                       p.live_count, p.counters, &ls->ext_foreign);
                hipLaunchKernelGGL(extend_seal_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) &ls->ext_foreign, p.live_count, &ls->ext_malformed);
                const uint32_t buckets = rtviews::sort_buckets(p.n_views, RTD_COST_BUCKETS);
                unsigned int *viewEnd = sortBuf + (size_t) p.n_views * buckets;
                p.view_end = viewEnd;
                const uint64_t nKeys = (uint64_t) p.n_views * buckets;
                const uint32_t ldsKeys = nKeys <= (uint64_t) VIEWS_SORT_LDS_KEYS ? (uint32_t) nKeys : 0u;
                // cost_bucket's divisor: a cost is at most spp samples, and 4 * spp / (spp / 16 + 1) < 64 = RTD_COST_BUCKETS
                const uint32_t costDiv = (uint32_t) p.spp / 16u + 1u;
                hipLaunchKernelGGL(views_sort_hist_kernel, dim3(256), dim3(256), (size_t) ldsKeys * 4u, st, (const unsigned long long *) pairs,
                                   (const unsigned int *) p.live_count, costDiv, p.view_pixels, buckets, ldsKeys, sortBuf);
                hipLaunchKernelGGL(views_sort_scan_kernel, dim3(1), dim3(256), 0, st, sortBuf, p.n_views, buckets, viewEnd);
                hipLaunchKernelGGL(views_sort_scatter_kernel, dim3(256), dim3(256), (size_t) ldsKeys * 8u, st, (const unsigned long long *) pairs,
                                   (const unsigned int *) p.live_count, costDiv, p.view_pixels, buckets, ldsKeys, sortBuf, list);
            } else
            if (job.map) // every pixel against its own target (p.spp is the cap); the seal is the same
                hipLaunchKernelGGL(extend_map_list_kernel, dim3(listGrid), dim3(256), 0, st, (const int32_t *) p.accum, p.ext_targets, nLocal, p.spp, list,
                                   p.live_count, p.counters, &ls->ext_foreign);
            else
                hipLaunchKernelGGL(extend_list_kernel, dim3(listGrid), dim3(256), 0, st, (const int32_t *) p.accum, nLocal, job.first_sample, list, p.live_count,
                                   p.counters, &ls->ext_foreign);
            if (!views) hipLaunchKernelGGL(extend_seal_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) &ls->ext_foreign, p.live_count, &ls->ext_malformed);
            if (p.rgb && job.map) // the final pixels AND the ones left as they are; pass B writes the continued ones'
                hipLaunchKernelGGL(extend_map_rest_rgb_kernel, dim3(listGrid), dim3(256), 0, st, (const int32_t *) p.accum, p.ext_targets, nLocal,
                                   (const unsigned int *) &ls->ext_malformed, p.rgb);
            else if (p.rgb)
                hipLaunchKernelGGL(extend_final_rgb_kernel, dim3(listGrid), dim3(256), 0, st, (const int32_t *) p.accum, nLocal,
                                   (const unsigned int *) &ls->ext_malformed, p.rgb);
            hipLaunchKernelGGL(fb, dim3((unsigned) plan.b.grid), dim3((unsigned) block), plan.b.lds_bytes, st, p);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("extension launch: ") + hipGetErrorString(e));
        } else if (!plan.two_pass) {
            set_plan_fields(p, plan.one);
            if (views) p.view_units = rtviews::units_per_view(rtviews::Plan{p.view_pixels, (uint32_t) p.chunk, p.n_views});
            hipLaunchKernelGGL(fn, dim3((unsigned) grid), dim3((unsigned) block), ldsBytes, st, p);
            HIP_TRY(hipGetLastError());
        } else {
            // workspace: pairs[nLocal] u64, list[nLocal] u32, hist/offsets/cursor[64] u32
            unsigned char *ws = scr + RT_SCRATCH_BYTES;
            unsigned int *sortBuf = (unsigned int *) (ws + pairsBytes + listBytes);
            HIP_TRY(hipMemsetAsync(sortBuf, 0, sortBytes, st));
            p.pairs = (unsigned long long *) ws;
            p.live_list = (const unsigned int *) (ws + pairsBytes);
            // both passes fit the LDS beside the scene image or nothing is launched (a misfit found after pass A would leave a
            // half-rendered buffer)
            if (plan.error) return fail(RT_ERR_HIP, plan.error);
            render_fn fa = pick_kernel(plan.a), fb = pick_kernel(plan.b);
            if (!fa || !fb) return fail(RT_ERR_HIP, "no kernel is built for this launch");
            if ((rc = allow_full_lds((const void *) fa)) != RT_OK || (rc = allow_full_lds((const void *) fb)) != RT_OK) return rc;
            RenderParams pa = p;
            set_plan_fields(pa, plan.a);
            set_plan_fields(p, plan.b);
            const uint32_t n1 = (uint32_t) (2 * p.k + 1);
            if (views) pa.view_units = rtviews::units_per_view(rtviews::Plan{p.view_pixels, (uint32_t) pa.chunk, p.n_views});
            hipLaunchKernelGGL(fa, dim3((unsigned) plan.a.grid), dim3((unsigned) block), plan.a.lds_bytes, st, pa);
            if (views) { // ordered by view, inside a view by decreasing cost; view_end clips pass B's ranges (rt_views_plan.h)
                const uint32_t buckets = rtviews::sort_buckets(p.n_views, RTD_COST_BUCKETS);
                unsigned int *viewEnd = sortBuf + (size_t) p.n_views * buckets;
                p.view_end = viewEnd;
                const uint64_t nKeys = (uint64_t) p.n_views * buckets;
                const uint32_t ldsKeys = nKeys <= (uint64_t) VIEWS_SORT_LDS_KEYS ? (uint32_t) nKeys : 0u; // (counted in LDS where the keys fit it)
                hipLaunchKernelGGL(views_sort_hist_kernel, dim3(256), dim3(256), (size_t) ldsKeys * 4u, st, (const unsigned long long *) p.pairs,
                                   (const unsigned int *) p.live_count, n1, p.view_pixels, buckets, ldsKeys, sortBuf);
                hipLaunchKernelGGL(views_sort_scan_kernel, dim3(1), dim3(256), 0, st, sortBuf, p.n_views, buckets, viewEnd);
                hipLaunchKernelGGL(views_sort_scatter_kernel, dim3(256), dim3(256), (size_t) ldsKeys * 8u, st, (const unsigned long long *) p.pairs,
                                   (const unsigned int *) p.live_count, n1, p.view_pixels, buckets, ldsKeys, sortBuf, (unsigned int *) (ws + pairsBytes));
            } else {
            hipLaunchKernelGGL(sort_hist_kernel, dim3(256), dim3(256), 0, st, (const unsigned long long *) p.pairs, (const unsigned int *) p.live_count, n1, sortBuf);
            hipLaunchKernelGGL(sort_offsets_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) sortBuf, sortBuf + RTD_COST_BUCKETS);
            hipLaunchKernelGGL(sort_scatter_kernel, dim3(256), dim3(256), 0, st, (const unsigned long long *) p.pairs, (const unsigned int *) p.live_count, n1,
                               (const unsigned int *) (sortBuf + RTD_COST_BUCKETS), sortBuf + 2 * RTD_COST_BUCKETS, (unsigned int *) (ws + pairsBytes));
            }
            hipLaunchKernelGGL(fb, dim3((unsigned) plan.b.grid), dim3((unsigned) block), plan.b.lds_bytes, st, p);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("two-pass launch: ") + hipGetErrorString(e));
        }
        if (want_stats) HIP_TRY(hipEventRecord(cl.b, st));
    }
    cl.launched = grid > 0;
    if (!want_stats) cl.release();
    return RT_OK;
}

// Enqueues one shard's render on `stream` (arguments checked by the caller, check_frame; n_rows may be 0: an empty shard of a fresh
// render still goes to the device, which the later entry points' no-op does not): the frame's own RenderParams fields, then enqueue().
static int launch_render(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                         int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                         const rt_render_options *options, bool want_stats, Pending &pd, const RayLog *log = nullptr, int32_t first_sample = 0,
                         const void *d_targets = nullptr) { // d_targets: an extension by map (first_sample is then RTD_EXTEND_MIN_DONE)
    RenderParams p{};
    p.max_w = max_w; p.max_h = max_h;
    p.spp = camera->samples_per_pixel;
    p.depth = camera->bounce_depth;
    p.seed_key = mix64(seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side
    p.cols = 2 * max_w + 1;
    p.row_first = row_first; p.row_stride = row_stride; p.n_rows = n_rows;
    p.accum = (int32_t *) d_accum;
    p.rgb = (uint8_t *) d_rgb;
    if (log) { p.ray_log = log->rays; p.ray_log_count = log->count; p.ray_log_cap = log->cap; p.ray_log_mask = log->mask; }
    rtp::Job job;
    job.kind = rtp::Job::FRAME;
    job.n_rows = (uint64_t) n_rows; job.max_w = max_w; job.spp = camera->samples_per_pixel;
    job.ray_log = log != nullptr;
    job.first_sample = first_sample;
    job.map = d_targets != nullptr;
    p.ext_targets = (const int32_t *) d_targets;
    return enqueue(scene, device, job, resolve_settings(options), flags, stream, p, camera_params(camera, max_w, max_h), want_stats, pd);
}

// Waits for the launch's stream and reads its counters (the device of the launch must be current).
static int collect_stats(Pending &pd, rt_stats *stats) {
    HIP_TRY(hipStreamSynchronize(pd.st));
    unsigned long long c[32] = {0}; // LaunchScratch: counters[16], then stage[12]
    if (pd.scr) {
        HIP_TRY(hipMemcpy(c, pd.scr + offsetof(LaunchScratch, counters), sizeof(LaunchScratch::counters), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(c + 16, pd.scr + offsetof(LaunchScratch, stage), sizeof(LaunchScratch::stage), hipMemcpyDeviceToHost));
    }
#ifdef RTD_STAGE_CLOCKS
    if (getenv("RTFS_STAGE_CLOCKS")) // diagnostic build: the finer clocks of rt_render_kernel.h's StageStats
        fprintf(stderr, "stage clocks: loop %llu leaf %llu unbounded %llu new_items %llu lambert %llu; node loop trips %llu, lanes stepping %llu (%.1f of 64 per trip)\n",
                c[23], c[24], c[25], c[26], c[27], c[14], c[15], c[14] ? (double) c[15] / (double) c[14] : 0.0);
#endif
    for (int i = 0; i < 6; ++i) g_last_stage_stats[i] = c[8 + i];
    g_last_stage_stats[6] = c[14];                                  // sum of wave lifetimes, 100 MHz ticks
    g_last_stage_stats[7] = c[15] - (0x4000000000000000ull - c[7]); // first wave start -> last wave end, ticks
    g_last_stage_stats[8] = pd.waves;
    for (int i = 0; i < 7; ++i) g_last_stage_stats[9 + i] = c[16 + i]; // slow stages, lanes in them, lanes parked, cycles in refill / slow / walk / shade
    if ((pd.extend || pd.list) && pd.scr) { // the seal found a Count the arguments do not explain (a pixel list: or an entry outside the frame): nothing was continued, nothing written
        unsigned int malformed = 0u;
        HIP_TRY(hipMemcpy(&malformed, pd.scr + offsetof(LaunchScratch, ext_malformed), sizeof(malformed), hipMemcpyDeviceToHost));
        if (malformed) {
            pd.release();
            return fail(RT_ERR_INVALID_ARGUMENT, pd.list ? (pd.extend ? "the pixel list has an entry outside the frame, or accum is not a buffer of samples_done samples per entry; left unchanged"
                                                                      : "the pixel list has an entry outside the frame; nothing was rendered")
                                                 : pd.map ? "accum or targets are not what the arguments say (a Count below 11, or a target above the cap); left unchanged"
                                                        : "accum is not a buffer of samples_done samples per pixel (a Count that is neither samples_done nor 11); left unchanged");
        }
    }
    float ms = 0.f;
    if (pd.launched) HIP_TRY(hipEventElapsedTime(&ms, pd.a, pd.b));
    memset(stats, 0, sizeof(*stats));
    stats->rays = c[0]; stats->aabb_tests = c[1]; stats->prim_tests = c[2]; stats->reflections = c[3];
    stats->samples = c[4]; stats->pixels_early = c[5];
    stats->pixels = pd.pixels;
    stats->kernel_ms = ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pd.t0).count();
    pd.release();
    return RT_OK;
}

// ------------------------------------------------------------------------------------------------------------
// the two shapes of a launching entry point: the device variant (the caller's device buffers, on its stream) and the host variant (host
// buffers staged through one device allocation, on the null stream).  Each is its argument checks, its no-op condition and ONE call of
// run_device or run_host around the same launch_* function.
// ------------------------------------------------------------------------------------------------------------
static int nothing_to_do(rt_stats *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    return RT_OK;
}

// The device variants' tail.  `launch(want_stats, pd)` is the entry point's launch_* call over its (checked) arguments.
template <class Launch> static int run_device(int32_t device, rt_stats *stats, bool nothing, Launch &&launch) {
    if (nothing) return nothing_to_do(stats);
    DeviceGuard guard; // (enqueue enters it again: a no-op then) so that collect_stats runs on the device too
    RT_TRY(guard.enter(device));
    Pending pd;
    const int rc = launch(stats != nullptr, pd);
    if (rc != RT_OK || !stats) return rc;
    return collect_stats(pd, stats);
}

namespace { // (host-side helpers with member functions: kept out of the library's dynamic symbols)

// One buffer of a host variant: where it is on the host (null: an optional buffer the caller left out, which takes no space), its
// size and which way it is copied.
enum { SEG_IN = 1, SEG_OUT = 2, SEG_INOUT = SEG_IN | SEG_OUT };
struct Segment { const void *host; size_t bytes; int use; };
// A host variant's device memory: its segments, in list order, at 16-byte-aligned offsets of ONE allocation that every exit path frees.
struct Staging {
    enum { MAX_SEGMENTS = 12 }; // (the most a call lists: the path records' two inputs and nine outputs)
    Segment seg[MAX_SEGMENTS];
    void *dev[MAX_SEGMENTS] = {}; // segment i on the device; null for an absent one
    int n = 0;
    unsigned char *buf = nullptr;
    ~Staging() { if (buf) (void) hipFree(buf); }
    int in(std::initializer_list<Segment> segments) { // the allocation (none for zero bytes), then the inputs, in list order
        size_t off[MAX_SEGMENTS], total = 0;
        for (const Segment &s : segments) {
            seg[n] = s; off[n++] = total;
            if (s.host) total += (s.bytes + 15u) & ~(size_t) 15u;
        }
        if (total) HIP_TRY(hipMalloc((void **) &buf, total));
        for (int i = 0; i < n; ++i) {
            if (!buf || !seg[i].host) continue;
            dev[i] = buf + off[i];
            if ((seg[i].use & SEG_IN) && seg[i].bytes) HIP_TRY(hipMemcpy(dev[i], seg[i].host, seg[i].bytes, hipMemcpyHostToDevice));
        }
        return RT_OK;
    }
    int out() { // the outputs, in list order
        for (int i = 0; i < n; ++i)
            if (dev[i] && (seg[i].use & SEG_OUT) && seg[i].bytes) HIP_TRY(hipMemcpy(const_cast<void *>(seg[i].host), dev[i], seg[i].bytes, hipMemcpyDeviceToHost));
        return RT_OK;
    }
};

} // namespace

// The host variants' body.  `launch(dev, want_stats, pd)` is the device variant's launch_* call over dev[i], segment i on the device,
// with a null stream and null options.  The statistics are ALWAYS asked for, whether or not the caller wants them: what only the
// device can refuse -- a buffer that is not what the arguments say, a list entry outside the frame -- is reported through
// collect_stats, and after such a refusal nothing is copied back.
template <class Launch>
static int run_host(int32_t device, rt_stats *stats, bool nothing, std::initializer_list<Segment> segments, Launch &&launch) {
    if (nothing) return nothing_to_do(stats);
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const auto t0 = std::chrono::steady_clock::now();
    Staging st;
    RT_TRY(st.in(segments));
    rt_stats local;
    RT_TRY(run_device(device, &local, false, [&](bool want_stats, Pending &pd) { return launch(st.dev, want_stats, pd); }));
    RT_TRY(st.out());
    if (stats) {
        *stats = local;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

#ifdef RTD_STAGE_CLOCKS
// Diagnostic builds only (not in include/rtfs_amd.h, not part of the ABI): the instruction census' execution counts of the current
// device, g_census (rt_device.h), summed over pass B's timed launches since the last reset.
extern "C" int rt_diag_census(uint64_t *out, int32_t n, int32_t reset) {
    unsigned long long c[RTD_CENSUS_WORDS] = {0};
    if (!out || n < 0 || n > RTD_CENSUS_WORDS) return fail(RT_ERR_INVALID_ARGUMENT, "rt_diag_census: bad arguments");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(c, HIP_SYMBOL(rtd::g_census), sizeof(c)));
    for (int i = 0; i < n; ++i) out[i] = c[i];
    if (reset) { memset(c, 0, sizeof(c)); HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_census), c, sizeof(c))); }
    return RT_OK;
}
#endif

extern "C" {

int rt_render_device_ex(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                        int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                        const rt_render_options *options, rt_stats *stats) {
    // The oldest entry points -- this one, rt_render_device and rt_render -- differ from all later ones in two ways that are kept as
    // they are and not fixed here: they test their arguments (rt_render: the scene and the settings) only after entering the device,
    // so a missing device or a bad device index is what they report first; and an empty shard (n_rows == 0) still goes to the device.
    return run_device(device, stats, false, [&](bool want_stats, Pending &pd) {
        RT_TRY(check_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, d_accum, "d_accum is NULL", options));
        return launch_render(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d_accum, d_rgb, stream, options, want_stats, pd);
    });
}

int rt_render_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                     int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                     rt_stats *stats) {
    return rt_render_device_ex(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d_accum, d_rgb, stream, nullptr, stats);
}

} // extern "C"

// The host half of tuning: at most 8192 of `raw` (evenly spaced) become the probe (the tree's quality levels off between 4096 and
// 8192 rays -- 15.64 / 15.50 box tests per held-out ray of the final scene, 15.55 with 32768 -- and the build time is linear in them); the walk tree is rebuilt and every device that
// holds a copy of the image gets the new one, once it has finished what it was doing.
struct RawRay { double v[6]; };
static int apply_tune(rt_scene *scene, const std::vector<RawRay> &raw, rt_tune_info &out) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t want = 8192;
    std::vector<rth::ProbeRay> rays;
    const size_t n = raw.size() < want ? raw.size() : want;
    rays.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const RawRay &r = raw[i * raw.size() / n];
        rth::ProbeRay pr;
        for (int a = 0; a < 3; ++a) { pr.o[a] = r.v[a]; pr.inv[a] = 1.0 / r.v[3 + a]; }
        rays.push_back(pr);
    }
    rth::TuneResult tr;
    std::lock_guard<std::mutex> lock(scene->mu);
    rth::HostScene &h = scene->host;
    if (rth::tune_applies(h, rays.size())) RT_TRY(ensure_host_mirror_locked(scene)); // (tune_walk_tree reads the scene's arrays exactly then)
    // Failure-atomic: the host tree and every device copy change together or not at all.  The new image is uploaded to fresh
    // allocations first; only when every device has its copy are the old ones released and the pointers swapped.  On any failure
    // the host scene is put back as it was and the new allocations are freed, so no launch can pair an old image with new offsets.
    struct Saved { rth::FlatTree walkTree; int walkKind; std::vector<unsigned char> image; rtd::SceneOffsets off; } saved{h.walkTree, h.walkKind, h.image, h.off};
    bool tuned = false;
    try {
        tuned = rth::tune_walk_tree(h, rays, tr);
    } catch (...) { // (out of host memory part-way: the scene stays as it was, guarded() reports it)
        h.walkTree = std::move(saved.walkTree); h.walkKind = saved.walkKind; h.image = std::move(saved.image); h.off = saved.off;
        throw;
    }
    if (!tuned) return RT_OK; // a reference-tree scene, or no rays: left as it is
    if (!scene->dev.empty()) {
        int prev = -1;
        if (hipGetDevice(&prev) != hipSuccess) { (void) hipGetLastError(); prev = -1; }
        struct Restore { int prev; ~Restore() { if (prev >= 0) (void) hipSetDevice(prev); } } restore{prev};
        std::vector<std::pair<int, unsigned char *>> fresh;
        hipError_t err = hipSuccess;
        for (auto &kv : scene->dev) {
            unsigned char *img = nullptr;
            err = hipSetDevice(kv.first);
            if (err == hipSuccess) err = hipMalloc((void **) &img, h.image.size());
            if (err == hipSuccess) { fresh.emplace_back(kv.first, img); err = hipMemcpy(img, h.image.data(), h.image.size(), hipMemcpyHostToDevice); }
            if (err != hipSuccess) break;
        }
        if (err != hipSuccess) {
            for (auto &f : fresh) if (hipSetDevice(f.first) == hipSuccess) (void) hipFree(f.second);
            h.walkTree = std::move(saved.walkTree); h.walkKind = saved.walkKind; h.image = std::move(saved.image); h.off = saved.off;
            return fail(RT_ERR_HIP, std::string("rt_scene_tune: uploading the rebuilt image: ") + hipGetErrorString(err));
        }
        for (auto &f : fresh) { // every device has the new image: let each finish what it was doing with the old one, then swap
            DeviceScene &d = scene->dev[f.first];
            if (hipSetDevice(f.first) == hipSuccess) { (void) hipDeviceSynchronize(); (void) hipFree(d.image); }
            d.image = f.second;
        }
    }
    out.tuned = 1;
    out.probe_rays = (int32_t) rays.size();
    out.nodes_before = tr.nodesBefore; out.nodes_after = tr.nodesAfter;
    out.box_tests_before = tr.visitsBefore; out.box_tests_after = tr.visitsAfter;
    out.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}

extern "C" {

static int scene_tune(rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, rt_tune_info *info) {
    rt_tune_info out{};
    auto report = [&]() {
        if (!info) return;
        const uint32_t sz = info->struct_size;
        memcpy(info, &out, sz < sizeof(out) ? sz : sizeof(out));
        info->struct_size = sz;
    };
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (info && info->struct_size < sizeof(uint32_t)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_tune_info.struct_size is not set");
    int rc = check_geometry(camera, max_w, max_h, 0, 1, 0);
    if (rc != RT_OK) return rc;
    rth::HostScene &h = scene->host;
    out.nodes_before = out.nodes_after = h.off.n_nodes;
    if (h.walkKind == RT_WALK_TREE_REFERENCE || h.nBounded < 3) { report(); return RT_OK; }
    DeviceGuard guard;
    rc = guard.enter(device);
    if (rc != RT_OK) return rc;

    // ---- the probe: 16 rows spread over the frame at a reduced sample count (a few million rays), traced by the TIMED kernel
    // variant, rays logged 1 in 2^k ----
    const int rows = 2 * max_h + 1, cols = 2 * max_w + 1;
    const int nProbe = rows < 16 ? rows : 16, stride = rows / nProbe, first = stride / 2;
    const uint32_t cap = 1u << 15, want = 8192u;
    rt_camera probeCam = *camera;
    {
        const double perSample = (double) nProbe * (double) cols * 3.3; // rays one sample of every probe pixel brings
        int spp = (int) std::ceil(4.0e6 / perSample);
        if (spp < 48) spp = 48; // well past the 2k+1 = 11 samples every pixel gets: the pixels that go on (Scene.fs:185-192) must weigh in the
                                // probe as they do in the frame, or the tree is tuned for the sky's rays
        if (spp < camera->samples_per_pixel) probeCam.samples_per_pixel = spp;
    }
    const double upper = (double) nProbe * (double) cols * (double) probeCam.samples_per_pixel * 4.0; // ~4 rays per sample
    int k = 0;
    while (k < 20 && upper / (double) (1u << k) > (double) (cap / 2u)) ++k;
    struct Bufs {
        unsigned char *all = nullptr;
        ~Bufs() { (void) hipFree(all); }
    } b;
    const size_t accumBytes = ((size_t) nProbe * (size_t) cols * 16u + 255u) & ~(size_t) 255u, rayBytes = (size_t) cap * 48u;
    HIP_TRY(hipMalloc((void **) &b.all, accumBytes + rayBytes + 256u));
    int32_t *pAccum = (int32_t *) b.all;
    double *pRays = (double *) (b.all + accumBytes);
    unsigned int *pCount = (unsigned int *) (b.all + accumBytes + rayBytes);
    unsigned int logged = 0;
    for (int attempt = 0; attempt < 12; ++attempt) {
        HIP_TRY(hipMemsetAsync(pCount, 0, sizeof(unsigned int), nullptr));
        const RayLog log{pRays, pCount, cap, (1u << k) - 1u};
        Pending pd;
        rt_render_options po{};
        po.struct_size = (uint32_t) sizeof(po);
        po.chunk_pixels = 4; // 16 rows are a few thousand pixels for 4096 waves: small units, or most waves get none and a few get the long ones
        po.passes = 1;       // the fused kernel: the only mode whose instantiations carry the ray log (rt_render_kernel.h, Sched<.., LOG>)
        rc = launch_render(scene, &probeCam, max_w, max_h, seed, device, first, stride, nProbe, 0u, pAccum, nullptr, nullptr, &po, true, pd, &log);
        if (rc != RT_OK) return rc;
        rt_stats st;
        rc = collect_stats(pd, &st);
        if (rc != RT_OK) return rc;
        out.probe_ms += st.kernel_ms;
        HIP_TRY(hipMemcpy(&logged, pCount, sizeof(logged), hipMemcpyDeviceToHost));
        if (logged > cap && k < 20) { k += 2; continue; }           // too many: log more thinly
        if (logged < want / 8u && k > 0) { k = k > 3 ? k - 3 : 0; continue; } // too few: log more densely
        break;
    }
    out.probe_rows = nProbe;
    // A log that still overflows holds whichever rays happened to be appended first: a scheduling-dependent subset, from which the
    // tree (and the box-test counters) would differ from run to run and from rank to rank.  Pixels would not, but "the same call
    // yields the same tree" is part of the contract: such a scene is left untuned.
    if (logged > cap || logged == 0) { report(); return RT_OK; }
    // ---- host: sort the log (its order depends on scheduling, its content does not) and rebuild ----
    std::vector<RawRay> raw(logged);
    HIP_TRY(hipMemcpy(raw.data(), pRays, (size_t) logged * sizeof(RawRay), hipMemcpyDeviceToHost));
    std::sort(raw.begin(), raw.end(), [](const RawRay &x, const RawRay &y) { return memcmp(&x, &y, sizeof(RawRay)) < 0; });
    rc = apply_tune(scene, raw, out);
    if (rc == RT_OK) report();
    return rc;
}
int rt_scene_tune(rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, rt_tune_info *info) {
    return guarded("rt_scene_tune", [&]() { return scene_tune(scene, camera, max_w, max_h, seed, device, info); });
}

int rt_scene_tune_rays(rt_scene *scene, const double *rays, size_t n_rays, rt_tune_info *info) {
    rt_tune_info out{};
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n_rays > 0 && !rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (info && info->struct_size < sizeof(uint32_t)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_tune_info.struct_size is not set");
    out.nodes_before = out.nodes_after = scene->host.off.n_nodes;
    return guarded("rt_scene_tune_rays", [&]() {
        std::vector<RawRay> raw(n_rays);
        if (n_rays) memcpy(raw.data(), rays, n_rays * sizeof(RawRay));
        const int rc = apply_tune(scene, raw, out);
        if (rc == RT_OK && info) {
            const uint32_t sz = info->struct_size;
            memcpy(info, &out, sz < sizeof(out) ? sz : sizeof(out));
            info->struct_size = sz;
        }
        return rc;
    });
}

int rt_render(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
              int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, int32_t *accum_host, uint8_t *rgb_host, rt_stats *stats) {
    RT_TRY(check_geometry(camera, max_w, max_h, row_first, row_stride, n_rows));
    if (n_rows > 0 && !accum_host) return fail(RT_ERR_INVALID_ARGUMENT, "accum_host is NULL");
    const size_t npx = (size_t) n_rows * (size_t) (2 * max_w + 1);
    return run_host(device, stats, false, {{accum_host, npx * 16u, SEG_OUT}, {rgb_host, npx * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL"); // (tested here, on the device: see rt_render_device_ex)
        RT_TRY(check_options(nullptr));
        return launch_render(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d[0], d[1], nullptr, nullptr, want_stats, pd);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// ray lists: the caller's rays through Scene.traceRay / Scene.hitObject (rtmode::RAYS_TRACE [4] / RAYS_HIT [5], run_rays)
// ------------------------------------------------------------------------------------------------------------
struct RayJob {
    bool hit;            // RAYS_HIT (hit queries) or RAYS_TRACE (paths)
    size_t n;
    const void *rays;    // [n][6] doubles
    void *rng;           // [n][4] uint32 or null (RAYS_TRACE)
    void *colour;        // [n][3] uint8 (RAYS_TRACE)
    void *hit_index;     // [n] int32 (RAYS_HIT)
    void *strike;        // [n][3] doubles or null (RAYS_HIT)
    uint64_t seed = 0, stream_base = 0;
    uint32_t sample = 0;
    int32_t depth = 0;
};

// Every argument check of the four ray-list entry points, made before anything touches a device.
static int check_rays(const rt_scene *scene, size_t n, const void *rays, const void *out, int32_t bounce_depth, const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n > 0 && !rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (n > 0 && !out) return fail(RT_ERR_INVALID_ARGUMENT, "output is NULL");
    RT_TRY(check_count(n, "rays"));
    RT_TRY(check_depth(bounce_depth));
    return check_options(options);
}

// Enqueues one ray-list launch on `stream` (n > 0, arguments checked by check_rays): the list's own RenderParams fields, then
// enqueue().  Placement (LDS, hybrid or global) is the render's decision.
static int launch_rays(const rt_scene *scene, int32_t device, const RayJob &job, uint32_t flags, void *stream, const rt_render_options *options,
                       bool want_stats, Pending &pd) {
    RenderParams p{};
    p.seed_key = mix64(job.seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side: the render's keying of (pixel, sample)
    p.depth = job.depth;
    p.rays = (const double *) job.rays;
    p.ray_rng = (uint32_t *) job.rng;
    p.ray_colour = (uint8_t *) job.colour;
    p.ray_hit = (int32_t *) job.hit_index;
    p.ray_strike = (double *) job.strike;
    p.ray_n = job.n;
    p.ray_base = job.stream_base;
    p.ray_sample = job.sample;
    rtp::Job list;
    list.kind = job.hit ? rtp::Job::HIT : rtp::Job::TRACE;
    list.n = job.n;
    return enqueue(scene, device, list, resolve_settings(options), flags, stream, p, CameraParams{}, want_stats, pd); // (no camera: never read in these modes)
}

static int run_rays_device(const rt_scene *scene, int32_t device, const RayJob &job, uint32_t flags, void *stream,
                           const rt_render_options *options, rt_stats *stats) {
    return run_device(device, stats, job.n == 0, [&](bool want_stats, Pending &pd) { return launch_rays(scene, device, job, flags, stream, options, want_stats, pd); });
}

// The host variants.  A job has the buffers of its own mode only (hit_job, trace_job); the colours come before the generator states
// because that is the order the two have always been copied back in.
static int run_rays_host(const rt_scene *scene, int32_t device, const RayJob &job, uint32_t flags, rt_stats *stats) {
    const size_t n = job.n;
    return run_host(device, stats, n == 0,
                    {{job.rays, n * 48u, SEG_IN}, {job.colour, n * 3u, SEG_OUT}, {job.rng, n * 16u, SEG_INOUT}, {job.hit_index, n * 4u, SEG_OUT}, {job.strike, n * 24u, SEG_OUT}},
                    [&](void *const *d, bool want_stats, Pending &pd) {
                        RayJob dev = job;
                        dev.rays = d[0]; dev.colour = d[1]; dev.rng = d[2]; dev.hit_index = d[3]; dev.strike = d[4];
                        return launch_rays(scene, device, dev, flags, nullptr, nullptr, want_stats, pd);
                    });
}

static RayJob hit_job(size_t n, const void *rays, void *hit_index, void *strike) {
    RayJob j{};
    j.hit = true; j.n = n; j.rays = rays; j.hit_index = hit_index; j.strike = strike;
    return j;
}
static RayJob trace_job(size_t n, const void *rays, void *rng, uint64_t seed, uint64_t stream_base, uint32_t sample, int32_t depth, void *colour) {
    RayJob j{};
    j.hit = false; j.n = n; j.rays = rays; j.rng = rng; j.colour = colour;
    j.seed = seed; j.stream_base = stream_base; j.sample = sample; j.depth = depth;
    return j;
}

extern "C" {

int rt_hit_objects(const rt_scene *scene, int32_t device, size_t n, const double *rays, uint32_t flags, int32_t *hit_index, double *strike,
                   rt_stats *stats) {
    RT_TRY(check_rays(scene, n, rays, hit_index, 0, nullptr));
    return run_rays_host(scene, device, hit_job(n, rays, hit_index, strike), flags, stats);
}

int rt_hit_objects_device(const rt_scene *scene, int32_t device, size_t n, const void *d_rays, uint32_t flags, void *d_hit_index, void *d_strike,
                          void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_rays(scene, n, d_rays, d_hit_index, 0, options));
    return run_rays_device(scene, device, hit_job(n, d_rays, d_hit_index, d_strike), flags, stream, options, stats);
}

int rt_trace_rays(const rt_scene *scene, int32_t device, size_t n, const double *rays, uint32_t *rng, uint64_t seed, uint64_t stream_base,
                  uint32_t sample, int32_t bounce_depth, uint32_t flags, uint8_t *colour, rt_stats *stats) {
    RT_TRY(check_rays(scene, n, rays, colour, bounce_depth, nullptr));
    return run_rays_host(scene, device, trace_job(n, rays, rng, seed, stream_base, sample, bounce_depth, colour), flags, stats);
}

int rt_trace_rays_device(const rt_scene *scene, int32_t device, size_t n, const void *d_rays, void *d_rng, uint64_t seed, uint64_t stream_base,
                         uint32_t sample, int32_t bounce_depth, uint32_t flags, void *d_colour, void *stream, const rt_render_options *options,
                         rt_stats *stats) {
    RT_TRY(check_rays(scene, n, d_rays, d_colour, bounce_depth, options));
    return run_rays_device(scene, device, trace_job(n, d_rays, d_rng, seed, stream_base, sample, bounce_depth, d_colour), flags, stream, options, stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// footprints: Scene.renderPixel over the caller's pixels, each with a camera of its own (rtmode::FOOTPRINTS_* [6, 7, 8])
// ------------------------------------------------------------------------------------------------------------
// Every argument check of the two footprint entry points, made before anything touches a device.
static int check_footprints(const rt_scene *scene, size_t n, const void *footprints, const void *accum, int32_t spp, int32_t bounce_depth,
                            const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n > 0 && !footprints) return fail(RT_ERR_INVALID_ARGUMENT, "footprints is NULL");
    if (n > 0 && !accum) return fail(RT_ERR_INVALID_ARGUMENT, "accum is NULL");
    RT_TRY(check_count(n, "footprints"));
    RT_TRY(check_spp(spp));
    RT_TRY(check_depth(bounce_depth));
    return check_options(options);
}

// Enqueues one footprint launch on `stream` (n > 0, arguments checked): to the kernel the list is a frame of one row and n columns
// whose pixel i reads footprint i and owns the stream of (seed, stream_base + i); then enqueue(), as for a frame shard.
static int launch_footprints(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints, int32_t spp, int32_t bounce_depth,
                             uint64_t seed, uint64_t stream_base, uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                             const rt_render_options *options, bool want_stats, Pending &pd, int32_t first_sample = 0, const void *d_targets = nullptr) {
    RenderParams p{};
    p.spp = spp;
    p.depth = bounce_depth;
    p.seed_key = mix64(seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side
    p.cols = (int32_t) n;
    p.row_first = 0; p.row_stride = 1; p.n_rows = 1;
    p.accum = (int32_t *) d_accum;
    p.rgb = (uint8_t *) d_rgb;
    p.rays = (const double *) d_footprints;
    p.ray_n = n;
    p.ray_base = stream_base;
    rtp::Job job;
    job.kind = rtp::Job::FOOTPRINTS;
    job.n = n; job.spp = spp;
    job.first_sample = first_sample;
    job.map = d_targets != nullptr; // an extension by map (first_sample is then RTD_EXTEND_MIN_DONE)
    p.ext_targets = (const int32_t *) d_targets;
    return enqueue(scene, device, job, resolve_settings(options), flags, stream, p, CameraParams{}, want_stats, pd); // (no camera: never read in these modes)
}

extern "C" {

int rt_render_footprints_device(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints, int32_t samples_per_pixel,
                                int32_t bounce_depth, uint64_t seed, uint64_t stream_base, uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                                const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_footprints(scene, n, d_footprints, d_accum, samples_per_pixel, bounce_depth, options));
    return run_device(device, stats, n == 0, [&](bool want_stats, Pending &pd) {
        return launch_footprints(scene, device, n, d_footprints, samples_per_pixel, bounce_depth, seed, stream_base, flags, d_accum, d_rgb, stream, options, want_stats, pd);
    });
}

int rt_render_footprints(const rt_scene *scene, int32_t device, size_t n, const double *footprints, int32_t samples_per_pixel, int32_t bounce_depth,
                         uint64_t seed, uint64_t stream_base, uint32_t flags, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_footprints(scene, n, footprints, accum, samples_per_pixel, bounce_depth, nullptr));
    return run_host(device, stats, n == 0, {{footprints, n * 96u, SEG_IN}, {accum, n * 16u, SEG_OUT}, {rgb, n * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_footprints(scene, device, n, d[0], samples_per_pixel, bounce_depth, seed, stream_base, flags, d[1], d[2], nullptr, nullptr, want_stats, pd);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// extending a rendered buffer to a higher sample count (DESIGN.md "Extending a frame"): pass B alone, from the stored PixelStats
// ------------------------------------------------------------------------------------------------------------
static int check_extend(int32_t target, int32_t samples_done) {
    if (samples_done < RTD_EXTEND_MIN_DONE)
        return fail(RT_ERR_INVALID_ARGUMENT, "samples_done must be >= 12 (below, firstTrial differs and Count cannot tell a stopped pixel from a finished one)");
    if (target < samples_done) return fail(RT_ERR_INVALID_ARGUMENT, "the target samples_per_pixel is below samples_done");
    return RT_OK;
}
// Every argument check of the two frame entry points, made before anything touches a device.
static int check_extend_frame(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, int32_t row_first, int32_t row_stride,
                              int32_t n_rows, const void *accum, const rt_render_options *options, int32_t samples_done) {
    RT_TRY(check_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, accum, "accum is NULL", options)); // (the options BEFORE the counts)
    RT_TRY(check_extend(camera->samples_per_pixel, samples_done));
    return check_extend_shard(max_w, n_rows);
}

extern "C" {

int rt_render_extend_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                            int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, int32_t samples_done, void *d_accum, void *d_rgb,
                            void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_extend_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, d_accum, options, samples_done));
    const bool nothing = n_rows == 0 || camera->samples_per_pixel == samples_done; // nothing to add
    return run_device(device, stats, nothing, [&](bool want_stats, Pending &pd) {
        return launch_render(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d_accum, d_rgb, stream, options, want_stats, pd, nullptr, samples_done);
    });
}

int rt_render_extend(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                     int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, int32_t samples_done, int32_t *accum, uint8_t *rgb,
                     rt_stats *stats) {
    RT_TRY(check_extend_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, accum, nullptr, samples_done));
    const bool nothing = n_rows == 0 || camera->samples_per_pixel == samples_done;
    const size_t npx = (size_t) n_rows * (size_t) (2 * max_w + 1);
    return run_host(device, stats, nothing, {{accum, npx * 16u, SEG_INOUT}, {rgb, npx * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_render(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d[0], d[1], nullptr, nullptr, want_stats, pd, nullptr, samples_done);
    });
}

int rt_render_footprints_extend_device(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints, int32_t samples_per_pixel,
                                       int32_t bounce_depth, uint64_t seed, uint64_t stream_base, uint32_t flags, int32_t samples_done, void *d_accum,
                                       void *d_rgb, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_footprints(scene, n, d_footprints, d_accum, samples_per_pixel, bounce_depth, options));
    RT_TRY(check_extend(samples_per_pixel, samples_done));
    return run_device(device, stats, n == 0 || samples_per_pixel == samples_done, [&](bool want_stats, Pending &pd) {
        return launch_footprints(scene, device, n, d_footprints, samples_per_pixel, bounce_depth, seed, stream_base, flags, d_accum, d_rgb, stream, options, want_stats, pd, samples_done);
    });
}

int rt_render_footprints_extend(const rt_scene *scene, int32_t device, size_t n, const double *footprints, int32_t samples_per_pixel, int32_t bounce_depth,
                                uint64_t seed, uint64_t stream_base, uint32_t flags, int32_t samples_done, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_footprints(scene, n, footprints, accum, samples_per_pixel, bounce_depth, nullptr));
    RT_TRY(check_extend(samples_per_pixel, samples_done));
    return run_host(device, stats, n == 0 || samples_per_pixel == samples_done,
                    {{footprints, n * 96u, SEG_IN}, {accum, n * 16u, SEG_INOUT}, {rgb, n * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_footprints(scene, device, n, d[0], samples_per_pixel, bounce_depth, seed, stream_base, flags, d[1], d[2], nullptr, nullptr, want_stats, pd, samples_done);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// extending by map (DESIGN.md "Extending by map"): every pixel from its stored Count to a target of its own.  The cap -- the camera's
// (footprints: the argument's) samples_per_pixel -- bounds every target.  Planned and launched as the extension 12 -> cap, with the
// map's list builder and pass B's per-pixel variant (rtmode::FRAME_PASS_B_MAP [9] / FOOTPRINTS_PASS_B_MAP [10]).
// ------------------------------------------------------------------------------------------------------------
static int check_extend_map(int32_t cap, size_t pixels, const void *targets) {
    if (cap < RTD_EXTEND_MIN_DONE)
        return fail(RT_ERR_INVALID_ARGUMENT, "a map's samples_per_pixel (the bound on every target) must be >= 12 (a buffer rendered below cannot be continued)");
    if (pixels > 0 && !targets) return fail(RT_ERR_INVALID_ARGUMENT, "targets is NULL");
    return RT_OK;
}
// Every argument check of the two frame entry points, made before anything touches a device.
static int check_extend_map_frame(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, int32_t row_first, int32_t row_stride,
                                  int32_t n_rows, const void *targets, const void *accum, const rt_render_options *options) {
    RT_TRY(check_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, accum, "accum is NULL", options)); // (the options BEFORE the map)
    RT_TRY(check_extend_map(camera->samples_per_pixel, (size_t) n_rows, targets));
    return check_extend_shard(max_w, n_rows);
}

extern "C" {

int rt_render_extend_map_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                                int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, const void *d_targets, void *d_accum, void *d_rgb,
                                void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_extend_map_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, d_targets, d_accum, options));
    return run_device(device, stats, n_rows == 0, [&](bool want_stats, Pending &pd) { // (an empty shard; a map whose every target is reached still goes to the device)
        return launch_render(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d_accum, d_rgb, stream, options, want_stats, pd, nullptr, RTD_EXTEND_MIN_DONE, d_targets);
    });
}

int rt_render_extend_map(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                         int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, const int32_t *targets, int32_t *accum, uint8_t *rgb,
                         rt_stats *stats) {
    RT_TRY(check_extend_map_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, targets, accum, nullptr));
    const size_t npx = (size_t) n_rows * (size_t) (2 * max_w + 1);
    return run_host(device, stats, n_rows == 0, {{accum, npx * 16u, SEG_INOUT}, {targets, npx * 4u, SEG_IN}, {rgb, npx * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_render(scene, camera, max_w, max_h, seed, device, row_first, row_stride, n_rows, flags, d[0], d[2], nullptr, nullptr, want_stats, pd, nullptr, RTD_EXTEND_MIN_DONE, d[1]);
    });
}

int rt_render_footprints_extend_map_device(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints, int32_t samples_per_pixel,
                                           int32_t bounce_depth, uint64_t seed, uint64_t stream_base, uint32_t flags, const void *d_targets, void *d_accum,
                                           void *d_rgb, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_footprints(scene, n, d_footprints, d_accum, samples_per_pixel, bounce_depth, options));
    RT_TRY(check_extend_map(samples_per_pixel, n, d_targets));
    return run_device(device, stats, n == 0, [&](bool want_stats, Pending &pd) {
        return launch_footprints(scene, device, n, d_footprints, samples_per_pixel, bounce_depth, seed, stream_base, flags, d_accum, d_rgb, stream, options, want_stats, pd, RTD_EXTEND_MIN_DONE, d_targets);
    });
}

int rt_render_footprints_extend_map(const rt_scene *scene, int32_t device, size_t n, const double *footprints, int32_t samples_per_pixel, int32_t bounce_depth,
                                    uint64_t seed, uint64_t stream_base, uint32_t flags, const int32_t *targets, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_footprints(scene, n, footprints, accum, samples_per_pixel, bounce_depth, nullptr));
    RT_TRY(check_extend_map(samples_per_pixel, n, targets));
    return run_host(device, stats, n == 0, {{footprints, n * 96u, SEG_IN}, {accum, n * 16u, SEG_INOUT}, {targets, n * 4u, SEG_IN}, {rgb, n * 3u, SEG_OUT}},
                    [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_footprints(scene, device, n, d[0], samples_per_pixel, bounce_depth, seed, stream_base, flags, d[1], d[3], nullptr, nullptr, want_stats, pd, RTD_EXTEND_MIN_DONE, d[2]);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// pixel lists (DESIGN.md "Pixel lists"): Scene.renderPixel (Scene.fs:157-194) over a caller's list of the FRAME's pixels, outputs in list
// order (rtmode::PIXELS_* [11, 12, 13])
// ------------------------------------------------------------------------------------------------------------
// Every argument check the four entry points share, made before anything touches a device.
static int check_pixels(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, size_t n, const void *pixels, const void *accum,
                        const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    RT_TRY(check_geometry(camera, max_w, max_h, 0, 1, 0));
    if (n > 0 && !pixels) return fail(RT_ERR_INVALID_ARGUMENT, "pixels is NULL");
    if (n > 0 && !accum) return fail(RT_ERR_INVALID_ARGUMENT, "accum is NULL");
    RT_TRY(check_count(n, "list entries"));
    RT_TRY(check_list_frame(max_w, max_h));
    return check_options(options);
}
// The host variants' list check (the device variants' is pixel_list_check_kernel): every entry a global pixel index of the frame.
static int check_pixel_entries(const int32_t *pixels, size_t n, int32_t max_w, int32_t max_h) {
    const int32_t frame = (2 * max_w + 1) * (2 * max_h + 1);
    for (size_t i = 0; i < n; ++i)
        if (pixels[i] < 0 || pixels[i] >= frame) return fail(RT_ERR_INVALID_ARGUMENT, "the pixel list has an entry outside the frame");
    return RT_OK;
}

// Enqueues one list launch on `stream` (n > 0, arguments checked): the frame's own RenderParams fields -- camera, geometry, seed -- and, for
// the kernel's unit loop, a frame of one row whose pixel i is the frame's pixel d_pixels[i]; then enqueue(), as for a frame shard.
static int launch_pixels(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                         const void *d_pixels, uint32_t flags, void *d_accum, void *d_rgb, void *stream, const rt_render_options *options,
                         bool want_stats, Pending &pd, int32_t first_sample = 0) {
    RenderParams p{};
    p.max_w = max_w; p.max_h = max_h;
    p.spp = camera->samples_per_pixel;
    p.depth = camera->bounce_depth;
    p.seed_key = mix64(seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side
    p.cols = 2 * max_w + 1;
    p.row_first = 0; p.row_stride = 1; p.n_rows = 1;
    p.accum = (int32_t *) d_accum;
    p.rgb = (uint8_t *) d_rgb;
    p.pixel_list = (const int32_t *) d_pixels;
    p.ray_n = n;
    rtp::Job job;
    job.kind = rtp::Job::PIXELS;
    job.n = n; job.spp = camera->samples_per_pixel;
    job.first_sample = first_sample;
    return enqueue(scene, device, job, resolve_settings(options), flags, stream, p, camera_params(camera, max_w, max_h), want_stats, pd);
}

extern "C" {

int rt_render_pixels_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                            const void *d_pixels, uint32_t flags, void *d_accum, void *d_rgb, void *stream, const rt_render_options *options,
                            rt_stats *stats) {
    RT_TRY(check_pixels(scene, camera, max_w, max_h, n, d_pixels, d_accum, options));
    return run_device(device, stats, n == 0, [&](bool want_stats, Pending &pd) {
        return launch_pixels(scene, camera, max_w, max_h, seed, device, n, d_pixels, flags, d_accum, d_rgb, stream, options, want_stats, pd);
    });
}

// The host variants check the list here, before anything touches a device (the device variants: pixel_list_check_kernel).
int rt_render_pixels(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                     const int32_t *pixels, uint32_t flags, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_pixels(scene, camera, max_w, max_h, n, pixels, accum, nullptr));
    RT_TRY(check_pixel_entries(pixels, n, max_w, max_h));
    return run_host(device, stats, n == 0, {{pixels, n * 4u, SEG_IN}, {accum, n * 16u, SEG_OUT}, {rgb, n * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_pixels(scene, camera, max_w, max_h, seed, device, n, d[0], flags, d[1], d[2], nullptr, nullptr, want_stats, pd);
    });
}

int rt_render_pixels_extend_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                                   const void *d_pixels, uint32_t flags, int32_t samples_done, void *d_accum, void *d_rgb, void *stream,
                                   const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_pixels(scene, camera, max_w, max_h, n, d_pixels, d_accum, options));
    RT_TRY(check_extend(camera->samples_per_pixel, samples_done));
    return run_device(device, stats, n == 0 || camera->samples_per_pixel == samples_done, [&](bool want_stats, Pending &pd) { // nothing to add
        return launch_pixels(scene, camera, max_w, max_h, seed, device, n, d_pixels, flags, d_accum, d_rgb, stream, options, want_stats, pd, samples_done);
    });
}

int rt_render_pixels_extend(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                            const int32_t *pixels, uint32_t flags, int32_t samples_done, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_pixels(scene, camera, max_w, max_h, n, pixels, accum, nullptr));
    RT_TRY(check_extend(camera->samples_per_pixel, samples_done));
    RT_TRY(check_pixel_entries(pixels, n, max_w, max_h));
    return run_host(device, stats, n == 0 || camera->samples_per_pixel == samples_done,
                    {{pixels, n * 4u, SEG_IN}, {accum, n * 16u, SEG_INOUT}, {rgb, n * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_pixels(scene, camera, max_w, max_h, seed, device, n, d[0], flags, d[1], d[2], nullptr, nullptr, want_stats, pd, samples_done);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// batches of views (DESIGN.md "Batches of views"): Scene.render (Scene.fs:157-236) for n_views cameras over one scene in ONE launch; view v is
// rt_render's frame for cameras[v] and seed v, in every PixelStats word and every rgb byte (render_views_kernel, rt_views_plan.h)
// ------------------------------------------------------------------------------------------------------------
// Every argument check both entry points make, before anything touches a device.
static int check_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const void *accum,
                       const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n_views < 0) return fail(RT_ERR_INVALID_ARGUMENT, "n_views must be >= 0");
    if (n_views > 0 && !cameras) return fail(RT_ERR_INVALID_ARGUMENT, "cameras is NULL");
    if (n_views > 0 && !accum) return fail(RT_ERR_INVALID_ARGUMENT, "accum is NULL");
    for (int32_t v = 0; v < n_views; ++v) {
        RT_TRY(check_geometry(&cameras[v], max_w, max_h, 0, 1, 2 * max_h + 1));
        // (the sample counts of a pass are wave-uniform launch parameters)
        if (cameras[v].samples_per_pixel != cameras[0].samples_per_pixel || cameras[v].bounce_depth != cameras[0].bounce_depth)
            return fail(RT_ERR_INVALID_ARGUMENT, "the cameras of a batch must share samples_per_pixel and bounce_depth");
    }
    if (n_views > 0 && (uint64_t) n_views * (uint64_t) (2 * max_w + 1) * (uint64_t) (2 * max_h + 1) > (uint64_t) INT32_MAX)
        return fail(RT_ERR_INVALID_ARGUMENT, "a batch of views holds at most INT32_MAX pixels");
    RT_TRY(check_options(options));
    if (scene->host.hasPrograms) return fail(RT_ERR_UNSUPPORTED, "a batch of views does not take a scene that holds a texture program");
    return RT_OK;
}

// Enqueues the batch on `stream` (n_views > 0, arguments checked): one view's geometry in the frame's RenderParams fields, the batch's
// buffers, the per-view cameras and seed keys for enqueue() to stage; cameras and seeds are read HERE, before the call returns.
static int launch_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                        int32_t device, uint32_t flags, void *d_accum, void *d_rgb, void *stream, const rt_render_options *options, bool want_stats, Pending &pd,
                        int32_t first_sample = 0, const void *d_targets = nullptr) { // as launch_render's: an extension of the batch; by map (first_sample is then RTD_EXTEND_MIN_DONE)
    RenderParams p{};
    p.max_w = max_w; p.max_h = max_h;
    p.spp = cameras[0].samples_per_pixel;
    p.depth = cameras[0].bounce_depth;
    p.cols = 2 * max_w + 1;
    p.row_first = 0; p.row_stride = 1; p.n_rows = 2 * max_h + 1;
    p.accum = (int32_t *) d_accum;
    p.rgb = (uint8_t *) d_rgb;
    ViewsArgs va;
    va.cams.reserve((size_t) n_views); va.keys.reserve((size_t) n_views);
    for (int32_t v = 0; v < n_views; ++v) {
        va.cams.push_back(camera_params(&cameras[v], max_w, max_h));
        va.keys.push_back(mix64((seeds ? seeds[v] : seed) + 0x9E3779B97F4A7C15ull)); // seed_key(), host side
    }
    rtp::Job job;
    job.kind = rtp::Job::VIEWS;
    job.n_views = (uint32_t) n_views;
    job.n_rows = (uint64_t) (2 * max_h + 1); job.max_w = max_w; job.spp = cameras[0].samples_per_pixel;
    job.first_sample = first_sample;
    job.map = d_targets != nullptr;
    p.ext_targets = (const int32_t *) d_targets;
    return enqueue(scene, device, job, resolve_settings(options), flags, stream, p, va.cams[0], want_stats, pd, &va);
}

extern "C" {

int rt_render_views_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                           int32_t device, uint32_t flags, void *d_accum, void *d_rgb, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_views(scene, cameras, n_views, max_w, max_h, d_accum, options));
    return run_device(device, stats, n_views == 0, [&](bool want_stats, Pending &pd) {
        return launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, d_accum, d_rgb, stream, options, want_stats, pd);
    });
}

int rt_render_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                    int32_t device, uint32_t flags, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_views(scene, cameras, n_views, max_w, max_h, accum, nullptr));
    const size_t px = n_views > 0 ? (size_t) n_views * (size_t) (2 * max_w + 1) * (size_t) (2 * max_h + 1) : 0u;
    return run_host(device, stats, n_views == 0, {{accum, px * 16u, SEG_OUT}, {rgb, px * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, d[0], d[1], nullptr, nullptr, want_stats, pd);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// continuing a batch of views (DESIGN.md "Continuing a batch of views"): rt_render_extend and rt_render_extend_map (Scene.fs:157-236 at a higher
// sample count) for the n_views frames of a batch in ONE launch -- the batch's list builders, the batch's ordering, then pass B of the
// views kernels from first_b on (uniform) or over per-pixel ranges (by map: render_views_kernel<.., FRAME_PASS_B_MAP, ..>)
// ------------------------------------------------------------------------------------------------------------
// Every argument check of the uniform pair, before anything touches a device: the batch's, then the extension's.  (No view: there is no
// camera to take the target from, and only samples_done itself is looked at.)
static int check_views_extend(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const void *accum,
                              const rt_render_options *options, int32_t samples_done) {
    RT_TRY(check_views(scene, cameras, n_views, max_w, max_h, accum, options));
    return check_extend(n_views > 0 ? cameras[0].samples_per_pixel : samples_done, samples_done);
}
// ... and of the pair by map: the cap is the cameras' shared samples_per_pixel
static int check_views_extend_map(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const void *targets,
                                  const void *accum, const rt_render_options *options) {
    RT_TRY(check_views(scene, cameras, n_views, max_w, max_h, accum, options));
    if (n_views == 0) return RT_OK;
    return check_extend_map(cameras[0].samples_per_pixel, (size_t) n_views, targets);
}
static size_t views_pixels(int32_t n_views, int32_t max_w, int32_t max_h) { // (checked: at most INT32_MAX)
    return n_views > 0 ? (size_t) n_views * (size_t) (2 * max_w + 1) * (size_t) (2 * max_h + 1) : 0u;
}

extern "C" {

int rt_render_views_extend_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds,
                                  uint64_t seed, int32_t device, uint32_t flags, int32_t samples_done, void *d_accum, void *d_rgb, void *stream,
                                  const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_views_extend(scene, cameras, n_views, max_w, max_h, d_accum, options, samples_done));
    const bool nothing = n_views == 0 || cameras[0].samples_per_pixel == samples_done; // nothing to add
    return run_device(device, stats, nothing, [&](bool want_stats, Pending &pd) {
        return launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, d_accum, d_rgb, stream, options, want_stats, pd, samples_done);
    });
}

int rt_render_views_extend(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                           int32_t device, uint32_t flags, int32_t samples_done, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_views_extend(scene, cameras, n_views, max_w, max_h, accum, nullptr, samples_done));
    const bool nothing = n_views == 0 || cameras[0].samples_per_pixel == samples_done;
    const size_t px = views_pixels(n_views, max_w, max_h);
    return run_host(device, stats, nothing, {{accum, px * 16u, SEG_INOUT}, {rgb, px * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, d[0], d[1], nullptr, nullptr, want_stats, pd, samples_done);
    });
}

int rt_render_views_extend_map_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds,
                                      uint64_t seed, int32_t device, uint32_t flags, const void *d_targets, void *d_accum, void *d_rgb, void *stream,
                                      const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_views_extend_map(scene, cameras, n_views, max_w, max_h, d_targets, d_accum, options));
    return run_device(device, stats, n_views == 0, [&](bool want_stats, Pending &pd) { // (a map whose every target is reached still goes to the device)
        return launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, d_accum, d_rgb, stream, options, want_stats, pd, RTD_EXTEND_MIN_DONE, d_targets);
    });
}

int rt_render_views_extend_map(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                               int32_t device, uint32_t flags, const int32_t *targets, int32_t *accum, uint8_t *rgb, rt_stats *stats) {
    RT_TRY(check_views_extend_map(scene, cameras, n_views, max_w, max_h, targets, accum, nullptr));
    const size_t px = views_pixels(n_views, max_w, max_h);
    return run_host(device, stats, n_views == 0, {{accum, px * 16u, SEG_INOUT}, {targets, px * 4u, SEG_IN}, {rgb, px * 3u, SEG_OUT}}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, d[0], d[2], nullptr, nullptr, want_stats, pd, RTD_EXTEND_MIN_DONE, d[1]);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// camera hits (DESIGN.md "Camera hits"): Scene.hitObject (Scene.fs:62-91) of the ray sample s of a frame's pixel starts with
// (Scene.traceOnce, Scene.fs:129-143), for a caller's list of pixels and a range of samples (rtmode::CAMERA_HITS [14])
// ------------------------------------------------------------------------------------------------------------
#define RT_CAMERA_HITS_MAX_SAMPLE 8000000 /* sample_first + n_samples at most: the cap of the map calls (check_geometry's samples_per_pixel) */
// Every argument check the two entry points share, made before anything touches a device.
static int check_camera_hits(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, size_t n, const void *pixels, int32_t sample_first,
                             int32_t n_samples, const void *hit_index, const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    RT_TRY(check_geometry(camera, max_w, max_h, 0, 1, 0));
    RT_TRY(check_list_frame(max_w, max_h));
    const uint64_t frame = (uint64_t) (2 * max_w + 1) * (uint64_t) (2 * max_h + 1);
    if (sample_first < 0) return fail(RT_ERR_INVALID_ARGUMENT, "sample_first must be >= 0");
    if (n_samples < 1) return fail(RT_ERR_INVALID_ARGUMENT, "n_samples must be >= 1");
    if ((int64_t) sample_first + (int64_t) n_samples > (int64_t) RT_CAMERA_HITS_MAX_SAMPLE) return fail(RT_ERR_INVALID_ARGUMENT, "sample_first + n_samples exceeds 8000000");
    if (n > (size_t) INT32_MAX || (uint64_t) n * (uint64_t) n_samples > (uint64_t) INT32_MAX)
        return fail(RT_ERR_INVALID_ARGUMENT, "more than INT32_MAX output slots (n * n_samples)");
    if (n > 0 && !hit_index) return fail(RT_ERR_INVALID_ARGUMENT, "hit_index is NULL");
    if (!pixels && (uint64_t) n > frame) return fail(RT_ERR_INVALID_ARGUMENT, "pixels is NULL and n exceeds the frame's pixels");
    return check_options(options);
}

// Enqueues the one launch on `stream` (n > 0, arguments checked): the frame's camera, geometry and seed, the list (or none), the sample
// range and the outputs, as RAYS_HIT's where they are RAYS_HIT's; then enqueue(), which checks a device list in front of the launch.
static int launch_camera_hits(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                              const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, void *d_hit_index, void *d_strike,
                              void *d_rays_out, void *stream, const rt_render_options *options, bool want_stats, Pending &pd) {
    RenderParams p{};
    p.max_w = max_w; p.max_h = max_h;
    p.spp = camera->samples_per_pixel;
    p.depth = camera->bounce_depth;
    p.seed_key = mix64(seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side
    p.cols = 2 * max_w + 1;
    p.row_first = 0; p.row_stride = 1; p.n_rows = 1;
    p.pixel_list = (const int32_t *) d_pixels;
    p.ray_n = n;
    p.ray_hit = (int32_t *) d_hit_index;
    p.ray_strike = (double *) d_strike;
    p.cam_rays_out = (double *) d_rays_out;
    p.cam_sample_first = sample_first; p.cam_n_samples = n_samples;
    rtp::Job job;
    job.kind = rtp::Job::CAMERA_HITS;
    job.n = n; job.spp = n_samples; job.first_sample = sample_first;
    return enqueue(scene, device, job, resolve_settings(options), flags, stream, p, camera_params(camera, max_w, max_h), want_stats, pd);
}

// What the statistics of camera hits count (collect_stats has filled in the rest).
static void camera_hits_counts(rt_stats *stats, size_t n, int32_t n_samples) {
    if (!stats) return;
    stats->pixels = (uint64_t) n;                          // list entries; nothing is shaded, so `reflections` stays 0
    stats->samples = (uint64_t) n * (uint64_t) n_samples;  // output slots (`rays`, under RT_RENDER_COUNTERS: those whose ray was made)
}

extern "C" {

int rt_camera_hits_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                          const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, void *d_hit_index, void *d_strike,
                          void *d_rays_out, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_camera_hits(scene, camera, max_w, max_h, n, d_pixels, sample_first, n_samples, d_hit_index, options));
    RT_TRY(run_device(device, stats, n == 0, [&](bool want_stats, Pending &pd) {
        return launch_camera_hits(scene, camera, max_w, max_h, seed, device, n, d_pixels, sample_first, n_samples, flags, d_hit_index, d_strike, d_rays_out, stream, options, want_stats, pd);
    }));
    camera_hits_counts(stats, n, n_samples);
    return RT_OK;
}

// The host variant checks a list here, before anything touches a device.
int rt_camera_hits(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                   const int32_t *pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, int32_t *hit_index, double *strike, double *rays_out,
                   rt_stats *stats) {
    RT_TRY(check_camera_hits(scene, camera, max_w, max_h, n, pixels, sample_first, n_samples, hit_index, nullptr));
    if (pixels) RT_TRY(check_pixel_entries(pixels, n, max_w, max_h));
    const size_t slots = n * (size_t) n_samples;
    RT_TRY(run_host(device, stats, n == 0, {{pixels, n * 4u, SEG_IN}, {hit_index, slots * 4u, SEG_OUT}, {strike, slots * 24u, SEG_OUT}, {rays_out, slots * 48u, SEG_OUT}},
                    [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_camera_hits(scene, camera, max_w, max_h, seed, device, n, d[0], sample_first, n_samples, flags, d[1], d[2], d[3], nullptr, nullptr, want_stats, pd);
    }));
    camera_hits_counts(stats, n, n_samples);
    return RT_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// surface records (DESIGN.md "Surface records"): normal, side, colour, tint and uv at a list of hits (surface_kernel, rt_surface_plan.h),
// and the same for what each pixel sample's camera ray strikes first (the camera-hits launch above, then surface_kernel on its stream)
// ------------------------------------------------------------------------------------------------------------
static int check_surface_outputs(const rt_surface_outputs *out) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out->struct_size != sizeof(rt_surface_outputs)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_surface_outputs.struct_size is not sizeof(rt_surface_outputs)");
    if (!out->normal && !out->inside && !out->colour && !out->tint && !out->uv) return fail(RT_ERR_INVALID_ARGUMENT, "every output is NULL");
    return RT_OK;
}
// Every argument check of rt_surfaces / rt_surfaces_device, made before anything touches a device.
static int check_surfaces(const rt_scene *scene, size_t n, const void *hit_index, const void *strike, const void *rays, const rt_surface_outputs *out,
                          const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n > 0 && !hit_index) return fail(RT_ERR_INVALID_ARGUMENT, "hit_index is NULL");
    if (n > 0 && !strike) return fail(RT_ERR_INVALID_ARGUMENT, "strike is NULL");
    if (n > 0 && !rays) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL");
    RT_TRY(check_surface_outputs(out));
    RT_TRY(check_count(n, "slots"));
    return check_options(options);
}
static int32_t scene_hittables(const rt_scene *scene) { return scene->host.off.n_bounded + scene->host.off.n_unbounded; }

// (`device` current.)  The inverse of obj_to_orig, made once per (scene, device) under the scene's mutex and finished before the mutex is
// given up, so every later launch on any stream finds it complete.  rt_scene_tune swaps the image and keeps the object table, so it holds.
static int surface_inverse_map(rt_scene *s, DeviceScene *ds, int32_t n) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (ds->orig_to_obj || n <= 0) return RT_OK;
    if (!ds->obj_to_orig) return fail(RT_ERR_HIP, "the scene has no object table on this device");
    int32_t *inv = nullptr;
    HIP_TRY(hipMalloc((void **) &inv, (size_t) n * sizeof(int32_t)));
    hipError_t e = hipMemset(inv, 0, (size_t) n * sizeof(int32_t));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(surface_inverse_map_kernel, dim3(((unsigned) n + 255u) / 256u), dim3(256), 0, nullptr, (const int32_t *) ds->obj_to_orig, n, inv);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { (void) hipFree(inv); return fail(RT_ERR_HIP, std::string("surface_inverse_map: ") + hipGetErrorString(e)); }
    ds->orig_to_obj = inv;
    return RT_OK;
}

struct SurfaceJob {
    size_t slots = 0;
    const void *hit_index = nullptr, *strike = nullptr, *origins = nullptr;
    uint32_t slots_per_origin = 1, origin_stride = 6;
    rt_surface_outputs out{};
    const unsigned int *bad = nullptr; // the camera route: the camera launch's LaunchScratch::ext_malformed.  null: the list is checked here
};
// What a surface launch leaves behind: events around the kernel and its two words (bad entries; textured slots evaluated).
struct SurfacePending {
    hipEvent_t a = nullptr, b = nullptr;
    unsigned char *words = nullptr;
    hipStream_t st = nullptr;
    bool checked = false;
    std::chrono::steady_clock::time_point t0;
    void release() {
        if (a) (void) hipEventDestroy(a);
        if (b) (void) hipEventDestroy(b);
        if (words) (void) hipFreeAsync(words, st);
        a = b = nullptr; words = nullptr;
    }
    ~SurfacePending() { release(); }
};
#define RT_SURFACE_WORDS_BYTES 16 /* [0] bad entries (uint32) [8] textured slots evaluated (uint64) */

// Enqueues the list check (unless the job brings its own verdict) and the surface kernel on `stream` (slots > 0, arguments checked).
static int launch_surfaces(const rt_scene *scene, int32_t device, const SurfaceJob &job, void *stream, bool want_stats, SurfacePending &sp) {
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    sp.t0 = std::chrono::steady_clock::now();
    DeviceScene *ds = nullptr;
    RT_TRY(device_scene(const_cast<rt_scene *>(scene), device, &ds));
    const rth::HostScene &h = scene->host;
    const int32_t nh = scene_hittables(scene);
    RT_TRY(surface_inverse_map(const_cast<rt_scene *>(scene), ds, nh));
    hipStream_t st = (hipStream_t) stream;
    const rtp::SceneSize sz = scene_size(h);
    const rtsf::SurfacePlan plan = rtsf::plan((uint64_t) job.slots, ds->cu_count, sz.tex, sz.prog, job.out.colour || job.out.tint || job.out.uv);
    {
        int64_t *o = g_last_surface_plan;
        o[0] = (int64_t) plan.slots; o[1] = plan.tile; o[2] = (int64_t) plan.grid; o[3] = plan.block; o[4] = plan.prog; o[5] = plan.tex_phase; o[6] = -1; o[7] = 0;
    }
    sp.st = st;
    sp.checked = job.bad == nullptr;
    if (sp.checked || want_stats) {
        HIP_TRY(hipMallocAsync((void **) &sp.words, RT_SURFACE_WORDS_BYTES, st));
        HIP_TRY(hipMemsetAsync(sp.words, 0, RT_SURFACE_WORDS_BYTES, st));
    }
    if (want_stats) {
        HIP_TRY(hipEventCreate(&sp.a));
        HIP_TRY(hipEventCreate(&sp.b));
        HIP_TRY(hipEventRecord(sp.a, st));
    }
    SurfaceParams p{};
    p.scene_image = ds->image; p.off = h.off; p.tex = ds->tex; p.texels = ds->texels;
    p.orig_to_obj = ds->orig_to_obj; p.n_hittables = nh;
    p.tex_phase = plan.tex_phase ? 1u : 0u;
    p.hit_index = (const int32_t *) job.hit_index; p.strike = (const double *) job.strike;
    p.origin_base = (const double *) job.origins; p.slots_per_origin = job.slots_per_origin; p.origin_stride = job.origin_stride;
    p.slots = (uint64_t) job.slots;
    p.normal = (double *) job.out.normal; p.inside = (uint8_t *) job.out.inside; p.colour = (uint8_t *) job.out.colour;
    p.tint = (uint8_t *) job.out.tint; p.uv = (double *) job.out.uv;
    p.bad = job.bad ? job.bad : (const unsigned int *) sp.words;
    p.textured = want_stats ? (unsigned long long *) (sp.words + 8) : nullptr;
    if (sp.checked) { // in front of the launch, on the same stream: is every entry an index of the scene, -1 or -2?
        const unsigned long long want = ((unsigned long long) job.slots + 255ull) / 256ull, most = (unsigned long long) ds->cu_count * 8ull;
        hipLaunchKernelGGL(surface_list_check_kernel, dim3((unsigned) (want < most ? want : most)), dim3(256), 0, st, p.hit_index, (unsigned long long) job.slots, nh,
                           (unsigned int *) sp.words);
    }
    if (plan.prog) hipLaunchKernelGGL(surface_kernel<true>, dim3((unsigned) plan.grid), dim3(RTSF_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(surface_kernel<false>, dim3((unsigned) plan.grid), dim3(RTSF_BLOCK), 0, st, p);
    HIP_TRY(hipGetLastError());
    if (want_stats) HIP_TRY(hipEventRecord(sp.b, st));
    else sp.release();
    return RT_OK;
}
// Waits for the launch's stream; a malformed list is reported here.  kernel_ms: the surface kernel's (with its list check).
static int collect_surfaces(SurfacePending &sp, float *kernel_ms) {
    HIP_TRY(hipStreamSynchronize(sp.st));
    unsigned int bad = 0u;
    unsigned long long textured = 0ull;
    HIP_TRY(hipMemcpy(&bad, sp.words, sizeof(bad), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&textured, sp.words + 8, sizeof(textured), hipMemcpyDeviceToHost));
    if (sp.checked && bad != 0u) {
        sp.release();
        return fail(RT_ERR_INVALID_ARGUMENT, "hit_index has an entry outside [-2, n_hittables); nothing was written");
    }
    HIP_TRY(hipEventElapsedTime(kernel_ms, sp.a, sp.b));
    g_last_surface_plan[6] = (int64_t) textured;
    sp.release();
    return RT_OK;
}
static void surface_stats(rt_stats *stats, size_t slots, float kernel_ms, std::chrono::steady_clock::time_point t0) {
    if (!stats) return;
    memset(stats, 0, sizeof(*stats));
    stats->samples = (uint64_t) slots;
    stats->kernel_ms = kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
static SurfaceJob ray_surface_job(size_t n, const void *hit_index, const void *strike, const void *rays, const rt_surface_outputs &out) {
    SurfaceJob j;
    j.slots = n; j.hit_index = hit_index; j.strike = strike; j.origins = rays; j.out = out;
    return j;
}
static int run_surfaces_device(const rt_scene *scene, int32_t device, const SurfaceJob &job, void *stream, rt_stats *stats) {
    DeviceGuard guard; // (launch_surfaces enters it again: a no-op then) so that collect_surfaces runs on the device too
    RT_TRY(guard.enter(device));
    SurfacePending sp;
    RT_TRY(launch_surfaces(scene, device, job, stream, stats != nullptr, sp));
    if (!stats) return RT_OK;
    float ms = 0.f;
    RT_TRY(collect_surfaces(sp, &ms));
    surface_stats(stats, job.slots, ms, sp.t0);
    return RT_OK;
}
// the five outputs as staging segments, in rt_surface_outputs' order
#define RT_SURFACE_OUT_SEGMENTS(o, slots) {(o).normal, (slots) * 24u, SEG_OUT}, {(o).inside, (slots), SEG_OUT}, {(o).colour, (slots) * 3u, SEG_OUT}, \
                                          {(o).tint, (slots) * 3u, SEG_OUT}, {(o).uv, (slots) * 16u, SEG_OUT}
static rt_surface_outputs staged_surface_outputs(const rt_surface_outputs &host, void *const *d) { // d: the five segments above, on the device
    rt_surface_outputs o = host;
    o.normal = d[0]; o.inside = d[1]; o.colour = d[2]; o.tint = d[3]; o.uv = d[4];
    return o;
}

extern "C" {

int rt_surfaces_device(const rt_scene *scene, int32_t device, size_t n, const void *d_hit_index, const void *d_strike, const void *d_rays, uint32_t flags,
                       const rt_surface_outputs *out, void *stream, const rt_render_options *options, rt_stats *stats) {
    (void) flags; // RT_RENDER_COUNTERS is accepted and changes nothing: there is one variant
    RT_TRY(check_surfaces(scene, n, d_hit_index, d_strike, d_rays, out, options));
    if (n == 0) return nothing_to_do(stats);
    return run_surfaces_device(scene, device, ray_surface_job(n, d_hit_index, d_strike, d_rays, *out), stream, stats);
}

// The host variant checks the list here, before anything touches a device.
int rt_surfaces(const rt_scene *scene, int32_t device, size_t n, const int32_t *hit_index, const double *strike, const double *rays, uint32_t flags,
                const rt_surface_outputs *out, rt_stats *stats) {
    (void) flags;
    RT_TRY(check_surfaces(scene, n, hit_index, strike, rays, out, nullptr));
    if (n == 0) return nothing_to_do(stats);
    const int32_t nh = scene_hittables(scene);
    for (size_t i = 0; i < n; ++i)
        if (!rtsf::list_entry_ok(hit_index[i], nh)) return fail(RT_ERR_INVALID_ARGUMENT, "hit_index has an entry outside [-2, n_hittables)");
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const auto t0 = std::chrono::steady_clock::now();
    Staging st;
    RT_TRY(st.in({{hit_index, n * 4u, SEG_IN}, {strike, n * 24u, SEG_IN}, {rays, n * 48u, SEG_IN}, RT_SURFACE_OUT_SEGMENTS(*out, n)}));
    rt_stats local;
    RT_TRY(run_surfaces_device(scene, device, ray_surface_job(n, st.dev[0], st.dev[1], st.dev[2], staged_surface_outputs(*out, st.dev + 3)), nullptr, &local));
    RT_TRY(st.out());
    if (stats) {
        *stats = local;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

int rt_dev_last_surface_plan(int64_t out[8]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = g_last_surface_plan[i];
    return RT_OK;
}

int rt_camera_surfaces_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                              const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, void *d_hit_index, void *d_strike,
                              const rt_surface_outputs *out, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_camera_hits(scene, camera, max_w, max_h, n, d_pixels, sample_first, n_samples, /* hit_index may be NULL here */ scene, options));
    RT_TRY(check_surface_outputs(out));
    if (n == 0) return nothing_to_do(stats);
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const size_t slots = n * (size_t) n_samples;
    hipStream_t st = (hipStream_t) stream;
    // what the caller does not want of the camera hits lives in stream-ordered scratch, given back behind the surface kernel
    struct Temp {
        unsigned char *p = nullptr;
        hipStream_t st = nullptr;
        ~Temp() { if (p) (void) hipFreeAsync(p, st); }
    } tmp;
    tmp.st = st;
    const size_t hitBytes = d_hit_index ? 0u : (slots * 4u + 15u) & ~(size_t) 15u, strikeBytes = d_strike ? 0u : slots * 24u;
    if (hitBytes + strikeBytes) HIP_TRY(hipMallocAsync((void **) &tmp.p, hitBytes + strikeBytes, st));
    void *hit = d_hit_index ? d_hit_index : (void *) tmp.p;
    void *strike = d_strike ? d_strike : (void *) (tmp.p + hitBytes);
    // the camera launch keeps its scratch (its statistics are asked for) until the surface kernel is enqueued: the kernel reads the
    // list's verdict and the one origin of every slot, camera->view_origin, from it
    Pending pd;
    RT_TRY(launch_camera_hits(scene, camera, max_w, max_h, seed, device, n, d_pixels, sample_first, n_samples, flags, hit, strike, nullptr, stream, options, true, pd));
    SurfaceJob job;
    job.slots = slots; job.hit_index = hit; job.strike = strike; job.out = *out;
    job.origins = pd.scr + offsetof(LaunchScratch, cam) + offsetof(CameraParams, eye);
    job.slots_per_origin = (uint32_t) slots; job.origin_stride = 3;
    job.bad = (const unsigned int *) (pd.scr + offsetof(LaunchScratch, ext_malformed));
    SurfacePending sp;
    RT_TRY(launch_surfaces(scene, device, job, stream, stats != nullptr, sp));
    if (!stats) { pd.release(); return RT_OK; }
    RT_TRY(collect_stats(pd, stats)); // (a list with an entry outside the frame is reported here)
    float ms = 0.f;
    RT_TRY(collect_surfaces(sp, &ms));
    stats->kernel_ms += ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pd.t0).count();
    camera_hits_counts(stats, n, n_samples);
    return RT_OK;
}

// The host variant checks a list here, before anything touches a device.
int rt_camera_surfaces(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                       const int32_t *pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, int32_t *hit_index, double *strike,
                       const rt_surface_outputs *out, rt_stats *stats) {
    RT_TRY(check_camera_hits(scene, camera, max_w, max_h, n, pixels, sample_first, n_samples, scene, nullptr));
    RT_TRY(check_surface_outputs(out));
    if (pixels) RT_TRY(check_pixel_entries(pixels, n, max_w, max_h));
    if (n == 0) return nothing_to_do(stats);
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const auto t0 = std::chrono::steady_clock::now();
    const size_t slots = n * (size_t) n_samples;
    Staging st;
    RT_TRY(st.in({{pixels, n * 4u, SEG_IN}, {hit_index, slots * 4u, SEG_OUT}, {strike, slots * 24u, SEG_OUT}, RT_SURFACE_OUT_SEGMENTS(*out, slots)}));
    const rt_surface_outputs dev = staged_surface_outputs(*out, st.dev + 3);
    rt_stats local;
    RT_TRY(rt_camera_surfaces_device(scene, camera, max_w, max_h, seed, device, n, st.dev[0], sample_first, n_samples, flags, st.dev[1], st.dev[2], &dev, nullptr, nullptr, &local));
    RT_TRY(st.out());
    if (stats) {
        *stats = local;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// camera hits over a batch of views (DESIGN.md "Camera hits over a batch of views"): the above for n_views cameras and ONE list in ONE
// launch; view v's slice of every output is rt_camera_hits' answer for cameras[v] and seed v (camera_hits_views_kernel, rt_views_plan.h)
// ------------------------------------------------------------------------------------------------------------
// Every argument check both entry points make, before anything touches a device: rt_camera_hits' own for every view (the first offending
// view reports), then the batch's bound.  The cameras need not share samples_per_pixel or bounce_depth -- nothing here traces beyond the
// camera ray -- and a scene with a texture program is taken: nothing is shaded.
static int check_camera_hits_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, size_t n, const void *pixels,
                                   int32_t sample_first, int32_t n_samples, const void *hit_index, const rt_render_options *options) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (n_views < 0) return fail(RT_ERR_INVALID_ARGUMENT, "n_views must be >= 0");
    if (n_views > 0 && !cameras) return fail(RT_ERR_INVALID_ARGUMENT, "cameras is NULL");
    for (int32_t v = 0; v < n_views; ++v) RT_TRY(check_camera_hits(scene, &cameras[v], max_w, max_h, n, pixels, sample_first, n_samples, hit_index, options));
    if (n_views > 0 && (uint64_t) n_views * (uint64_t) n * (uint64_t) n_samples > (uint64_t) INT32_MAX) // (n * n_samples <= INT32_MAX: no overflow)
        return fail(RT_ERR_INVALID_ARGUMENT, "more than INT32_MAX output slots (n_views * n * n_samples)");
    return check_options(options);
}

// Enqueues the one launch on `stream` (n_views > 0, n > 0, arguments checked): launch_camera_hits' fields with the batch's outputs, the
// per-view cameras and seed keys for enqueue() to stage; cameras and seeds are read HERE, before the call returns.
static int launch_camera_hits_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds,
                                    uint64_t seed, int32_t device, size_t n, const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags,
                                    void *d_hit_index, void *d_strike, void *d_rays_out, void *stream, const rt_render_options *options, bool want_stats,
                                    Pending &pd) {
    RenderParams p{};
    p.max_w = max_w; p.max_h = max_h;
    p.spp = cameras[0].samples_per_pixel;
    p.depth = cameras[0].bounce_depth;
    p.cols = 2 * max_w + 1;
    p.row_first = 0; p.row_stride = 1; p.n_rows = 1;
    p.pixel_list = (const int32_t *) d_pixels;
    p.ray_n = n; // (one view's: the kernel reads view_pixels, which enqueue() sets to the same)
    p.ray_hit = (int32_t *) d_hit_index;
    p.ray_strike = (double *) d_strike;
    p.cam_rays_out = (double *) d_rays_out;
    p.cam_sample_first = sample_first; p.cam_n_samples = n_samples;
    ViewsArgs va;
    va.cams.reserve((size_t) n_views); va.keys.reserve((size_t) n_views);
    for (int32_t v = 0; v < n_views; ++v) {
        va.cams.push_back(camera_params(&cameras[v], max_w, max_h));
        va.keys.push_back(mix64((seeds ? seeds[v] : seed) + 0x9E3779B97F4A7C15ull)); // seed_key(), host side
    }
    rtp::Job job;
    job.kind = rtp::Job::CAMERA_HITS;
    job.n_views = (uint32_t) n_views; // (>= 1: the batch)
    job.n = n; job.spp = n_samples; job.first_sample = sample_first;
    return enqueue(scene, device, job, resolve_settings(options), flags, stream, p, va.cams[0], want_stats, pd, &va);
}

extern "C" {

int rt_camera_hits_views_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds,
                                uint64_t seed, int32_t device, size_t n, const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags,
                                void *d_hit_index, void *d_strike, void *d_rays_out, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_camera_hits_views(scene, cameras, n_views, max_w, max_h, n, d_pixels, sample_first, n_samples, d_hit_index, options));
    const bool nothing = n_views == 0 || n == 0;
    RT_TRY(run_device(device, stats, nothing, [&](bool want_stats, Pending &pd) {
        return launch_camera_hits_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, n, d_pixels, sample_first, n_samples, flags, d_hit_index,
                                        d_strike, d_rays_out, stream, options, want_stats, pd);
    }));
    if (!nothing) camera_hits_counts(stats, (size_t) n_views * n, n_samples);
    return RT_OK;
}

// The host variant checks the shared list here, once, before anything touches a device.
int rt_camera_hits_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                         int32_t device, size_t n, const int32_t *pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, int32_t *hit_index,
                         double *strike, double *rays_out, rt_stats *stats) {
    RT_TRY(check_camera_hits_views(scene, cameras, n_views, max_w, max_h, n, pixels, sample_first, n_samples, hit_index, nullptr));
    const bool nothing = n_views == 0 || n == 0;
    if (pixels && !nothing) RT_TRY(check_pixel_entries(pixels, n, max_w, max_h));
    const size_t slots = nothing ? 0u : (size_t) n_views * n * (size_t) n_samples;
    RT_TRY(run_host(device, stats, nothing, {{pixels, n * 4u, SEG_IN}, {hit_index, slots * 4u, SEG_OUT}, {strike, slots * 24u, SEG_OUT}, {rays_out, slots * 48u, SEG_OUT}},
                    [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_camera_hits_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, n, d[0], sample_first, n_samples, flags, d[1], d[2], d[3], nullptr,
                                        nullptr, want_stats, pd);
    }));
    if (!nothing) camera_hits_counts(stats, (size_t) n_views * n, n_samples);
    return RT_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// path records (DESIGN.md "Path records"): Scene.traceRay (Scene.fs:93-114) with every vertex written down, for the samples of a
// frame's pixels (rt_camera_paths: rt_camera_hits' list, frame and slots) or a caller's rays (rt_trace_paths: rt_trace_rays' rays,
// states and keys).  A kernel of its own (rt_paths_kernels.h) with a plan of its own (rt_paths_plan.h), on the launch wrapper, the
// staging helper and the check list of every other entry point.
// ------------------------------------------------------------------------------------------------------------
typedef void (*paths_fn)(const RenderParams, const PathParams);
template <bool TEX, int BLOCK> static paths_fn pick_paths_variant(bool lds, bool count) {
    if (count) return paths_kernel<false, true, TEX, BLOCK>;
    return lds ? paths_kernel<true, false, TEX, BLOCK> : paths_kernel<false, false, TEX, BLOCK>;
}
static paths_fn pick_paths_kernel(const rtpp::PathsPlan &pl) { // blocks of 256 and 1024 only; TEX only where the scene has parameterised textures
    if (pl.prog) {
        if (pl.count) return pl.block == 256 ? paths_prog_kernel<false, true, 256> : paths_prog_kernel<false, true, 1024>;
        if (pl.lds) return pl.block == 256 ? paths_prog_kernel<true, false, 256> : paths_prog_kernel<true, false, 1024>;
        return pl.block == 256 ? paths_prog_kernel<false, false, 256> : paths_prog_kernel<false, false, 1024>;
    }
    if (pl.block == 256) return pl.tex ? pick_paths_variant<true, 256>(pl.lds, pl.count) : pick_paths_variant<false, 256>(pl.lds, pl.count);
    return pl.tex ? pick_paths_variant<true, 1024>(pl.lds, pl.count) : pick_paths_variant<false, 1024>(pl.lds, pl.count);
}

// What both families refuse about `out`, made before anything touches a device.  `camera`: first_ray and summary belong to camera paths.
static int check_path_outputs(const rt_path_outputs *out, bool camera) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    if (out->struct_size != sizeof(rt_path_outputs)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_path_outputs.struct_size is not sizeof(rt_path_outputs)");
    if (out->max_vertices < 0) return fail(RT_ERR_INVALID_ARGUMENT, "max_vertices must be >= 0");
    if (!camera && (out->first_ray || out->summary)) return fail(RT_ERR_INVALID_ARGUMENT, "first_ray and summary belong to camera paths");
    const bool records = out->max_vertices > 0 && (out->hit_index || out->strike || out->colour_after || out->ray_after);
    if (!out->n_vertices && !out->end && !out->colour && !out->first_ray && !out->summary && !records)
        return fail(RT_ERR_INVALID_ARGUMENT, "every output is NULL");
    return RT_OK;
}
static int check_path_sizes(uint64_t slots, const rt_path_outputs *out, int32_t n_samples, int32_t bounce_depth) {
    const uint64_t k = out->max_vertices > 0 ? (uint64_t) out->max_vertices : 1u;
    if (slots > (uint64_t) INT32_MAX || slots * k > (uint64_t) INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "more than INT32_MAX records (slots * max(max_vertices, 1))");
    if (out->summary && (uint64_t) n_samples * ((uint64_t) bounce_depth + 1u) > (uint64_t) INT32_MAX)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_samples * (bounce_depth + 1) exceeds INT32_MAX: the summary's sum of n_vertices is an int32");
    return RT_OK;
}
static int check_camera_paths(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, size_t n, const void *pixels, int32_t sample_first,
                              int32_t n_samples, const rt_path_outputs *out, const rt_render_options *options) {
    RT_TRY(check_path_outputs(out, true));
    RT_TRY(check_camera_hits(scene, camera, max_w, max_h, n, pixels, sample_first, n_samples, out, options)); // (`out` stands for its one required output)
    return check_path_sizes((uint64_t) n * (uint64_t) n_samples, out, n_samples, camera->bounce_depth);
}
static int check_trace_paths(const rt_scene *scene, size_t n, const void *rays, int32_t bounce_depth, const rt_path_outputs *out, const rt_render_options *options) {
    RT_TRY(check_path_outputs(out, false));
    RT_TRY(check_rays(scene, n, rays, out, bounce_depth, options));
    return check_path_sizes((uint64_t) n, out, 1, bounce_depth);
}

// The outputs as the kernel reads them: K == 0 ignores the per-record pointers.
static void path_outputs_to_params(const rt_path_outputs &o, PathParams &q) {
    const bool rec = o.max_vertices > 0;
    q.max_vertices = o.max_vertices;
    q.n_vertices = o.n_vertices; q.end = o.end; q.colour = o.colour; q.first_ray = o.first_ray;
    q.hit_index = rec ? o.hit_index : nullptr; q.strike = rec ? o.strike : nullptr;
    q.colour_after = rec ? o.colour_after : nullptr; q.ray_after = rec ? o.ray_after : nullptr;
    q.summary = o.summary;
}

// Enqueues one path launch on `stream` (slots > 0, arguments checked): the scene's RenderParams fields, the plan, the launch's scratch
// from the stream's pool, then -- all on `stream`, nothing waits for the device -- the scratch's set-up, a device list's check and seal
// (pixel_list_check_kernel; the seal poisons the run counter, so nothing is traced and nothing written), the summary's zeroing behind
// that seal, and the kernel.  `entries`: list entries (camera paths) or rays.
static int enqueue_paths(const rt_scene *scene, int32_t device, PathParams q, uint64_t entries, const CameraParams &cam, const Settings &set, uint32_t flags,
                         void *stream, bool want_stats, Pending &pd) {
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const auto t0 = std::chrono::steady_clock::now();
    DeviceScene *ds = nullptr;
    RT_TRY(device_scene(const_cast<rt_scene *>(scene), device, &ds));
    const rth::HostScene &h = scene->host;
    hipStream_t st = (hipStream_t) stream;
    RenderParams p{}; // the scene's part only: what stage_scene and make_view read
    p.off = h.off;
    p.scene_image = ds->image;
    p.tex = ds->tex;
    p.texels = ds->texels;
    q.obj_to_orig = ds->obj_to_orig;

    // RTFS_PATHS_ROUTE=global: a measurement's switch (scripts/paths_measure.py times the two routes of one scene); results cannot depend on it
    const char *route = getenv("RTFS_PATHS_ROUTE");
    rtpp::PathsPlan plan = rtpp::plan_begin(scene_size(h), set, (flags & RT_RENDER_COUNTERS) != 0, q.slots, !(route && strcmp(route, "global") == 0));
    paths_fn fn = pick_paths_kernel(plan);
    RT_TRY(allow_full_lds((const void *) fn));
    int perCu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, (const void *) fn, plan.block, plan.lds_bytes));
    if (perCu < 1) return fail(RT_ERR_HIP, "path kernel does not fit on a CU (occupancy 0)");
    rtpp::plan_finish(plan, ds->cu_count, perCu);
    {
        int64_t *o = g_last_paths_plan;
        o[0] = plan.block; o[1] = (int64_t) plan.grid; o[2] = plan.chunk; o[3] = (int64_t) plan.lds_bytes; o[4] = plan.lds ? 1 : 0;
        o[5] = plan.count ? 1 : 0; o[6] = plan.tex ? (plan.prog ? 2 : 1) : 0; o[7] = (int64_t) plan.slots;
    }
    q.chunk = plan.chunk;

    unsigned char *scr = nullptr;
    HIP_TRY(hipMallocAsync((void **) &scr, RT_SCRATCH_BYTES, st));
    pd.scr = scr; pd.st = st; pd.device = device; pd.t0 = t0; // on every exit path pd's destructor (or collect_stats) gives the scratch back
    pd.pixels = entries;
    pd.waves = plan.grid * (uint64_t) (plan.block / 64);
    pd.list = q.pixel_list != nullptr;
    if (want_stats) {
        HIP_TRY(hipEventCreate(&pd.a));
        HIP_TRY(hipEventCreate(&pd.b));
    }
    LaunchScratch *ls = (LaunchScratch *) scr;
    q.counters = ls->counters;
    q.queue = &ls->queue;
    q.cam = &ls->cam;
    hipLaunchKernelGGL(launch_init_kernel, dim3(1), dim3(64), 0, st, scr, cam);
    HIP_TRY(hipGetLastError());
    if (want_stats) HIP_TRY(hipEventRecord(pd.a, st));
    const unsigned long long most = (unsigned long long) ds->cu_count * 8ull;
    if (pd.list) {
        const unsigned long long want = ((unsigned long long) entries + 255ull) / 256ull;
        hipLaunchKernelGGL(pixel_list_check_kernel, dim3((unsigned) (want < most ? want : most)), dim3(256), 0, st, q.pixel_list, (unsigned long long) entries,
                           (uint32_t) q.cols * (uint32_t) (2 * q.max_h + 1), &ls->ext_foreign);
        hipLaunchKernelGGL(pixel_list_seal_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) &ls->ext_foreign, q.queue, &ls->ext_malformed);
        HIP_TRY(hipGetLastError());
    }
    if (q.summary) {
        const unsigned long long words = (unsigned long long) entries * RT_PATH_SUMMARY_WORDS, want = (words + 255ull) / 256ull;
        hipLaunchKernelGGL(paths_summary_zero_kernel, dim3((unsigned) (want < most ? want : most)), dim3(256), 0, st, q.summary, words,
                           pd.list ? (const unsigned int *) &ls->ext_malformed : (const unsigned int *) nullptr);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(fn, dim3((unsigned) plan.grid), dim3((unsigned) plan.block), plan.lds_bytes, st, p, q);
    HIP_TRY(hipGetLastError());
    if (want_stats) HIP_TRY(hipEventRecord(pd.b, st));
    pd.launched = true;
    if (!want_stats) pd.release();
    return RT_OK;
}

static int launch_camera_paths(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                               const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, const rt_path_outputs &out, void *stream,
                               const rt_render_options *options, bool want_stats, Pending &pd) {
    PathParams q{};
    q.pixel_list = (const int32_t *) d_pixels;
    q.seed_key = mix64(seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side
    q.sample_first = sample_first; q.n_samples = n_samples;
    q.cols = 2 * max_w + 1; q.max_w = max_w; q.max_h = max_h;
    q.depth = camera->bounce_depth;
    q.slots = (uint64_t) n * (uint64_t) n_samples;
    path_outputs_to_params(out, q);
    return enqueue_paths(scene, device, q, (uint64_t) n, camera_params(camera, max_w, max_h), resolve_settings(options), flags, stream, want_stats, pd);
}
static int launch_trace_paths(const rt_scene *scene, int32_t device, size_t n, const void *d_rays, void *d_rng, uint64_t seed, uint64_t stream_base, uint32_t sample,
                              int32_t bounce_depth, uint32_t flags, const rt_path_outputs &out, void *stream, const rt_render_options *options, bool want_stats,
                              Pending &pd) {
    PathParams q{};
    q.rays = (const double *) d_rays;
    q.rng = (uint32_t *) d_rng;
    q.seed_key = mix64(seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side: rt_trace_rays' keying
    q.ray_base = stream_base; q.ray_sample = sample;
    q.n_samples = 1;
    q.depth = bounce_depth;
    q.slots = (uint64_t) n;
    path_outputs_to_params(out, q);
    q.first_ray = nullptr; q.summary = nullptr;
    return enqueue_paths(scene, device, q, (uint64_t) n, CameraParams{}, resolve_settings(options), flags, stream, want_stats, pd); // (no camera: never read)
}

// What the statistics of a path call count (collect_stats has filled in the rest).
static void paths_counts(rt_stats *stats, size_t n, uint64_t slots) {
    if (!stats) return;
    stats->pixels = (uint64_t) n; // list entries or rays
    stats->samples = slots;
}

// The host variants' segments behind their inputs: the nine outputs, in rt_path_outputs' order (an absent one takes no space).
#define RT_PATH_SEGMENTS(o, slots, recs, entries)                                                                                                       \
    {(o).n_vertices, (slots) * 4u, SEG_OUT}, {(o).end, (slots) * 4u, SEG_OUT}, {(o).colour, (slots) * 3u, SEG_OUT}, {(o).first_ray, (slots) * 48u, SEG_OUT},  \
    {(o).hit_index, (recs) * 4u, SEG_OUT}, {(o).strike, (recs) * 24u, SEG_OUT}, {(o).colour_after, (recs) * 3u, SEG_OUT}, {(o).ray_after, (recs) * 48u, SEG_OUT}, \
    {(o).summary, (entries) * (size_t) RT_PATH_SUMMARY_WORDS * 4u, SEG_OUT}
static rt_path_outputs staged_path_outputs(const rt_path_outputs &host, void *const *d) { // d: the nine segments above, on the device
    rt_path_outputs o = host;
    o.n_vertices = (int32_t *) d[0]; o.end = (int32_t *) d[1]; o.colour = (uint8_t *) d[2]; o.first_ray = (double *) d[3];
    o.hit_index = (int32_t *) d[4]; o.strike = (double *) d[5]; o.colour_after = (uint8_t *) d[6]; o.ray_after = (double *) d[7];
    o.summary = (int32_t *) d[8];
    return o;
}
static rt_path_outputs host_path_outputs(const rt_path_outputs &out) { // K == 0: the per-record pointers are not the caller's to be written
    rt_path_outputs o = out;
    if (o.max_vertices == 0) { o.hit_index = nullptr; o.strike = nullptr; o.colour_after = nullptr; o.ray_after = nullptr; }
    return o;
}

extern "C" {

int rt_camera_paths_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                           const void *d_pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, const rt_path_outputs *out, void *stream,
                           const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_camera_paths(scene, camera, max_w, max_h, n, d_pixels, sample_first, n_samples, out, options));
    RT_TRY(run_device(device, stats, n == 0, [&](bool want_stats, Pending &pd) {
        return launch_camera_paths(scene, camera, max_w, max_h, seed, device, n, d_pixels, sample_first, n_samples, flags, *out, stream, options, want_stats, pd);
    }));
    if (n) paths_counts(stats, n, (uint64_t) n * (uint64_t) n_samples);
    return RT_OK;
}

// The host variant checks a list here, before anything touches a device.
int rt_camera_paths(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, size_t n,
                    const int32_t *pixels, int32_t sample_first, int32_t n_samples, uint32_t flags, const rt_path_outputs *out, rt_stats *stats) {
    RT_TRY(check_camera_paths(scene, camera, max_w, max_h, n, pixels, sample_first, n_samples, out, nullptr));
    if (pixels) RT_TRY(check_pixel_entries(pixels, n, max_w, max_h));
    const rt_path_outputs o = host_path_outputs(*out);
    const size_t slots = n * (size_t) n_samples, recs = slots * (size_t) o.max_vertices;
    RT_TRY(run_host(device, stats, n == 0, {{pixels, n * 4u, SEG_IN}, RT_PATH_SEGMENTS(o, slots, recs, n)}, [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_camera_paths(scene, camera, max_w, max_h, seed, device, n, d[0], sample_first, n_samples, flags, staged_path_outputs(o, d + 1), nullptr, nullptr,
                                   want_stats, pd);
    }));
    if (n) paths_counts(stats, n, (uint64_t) slots);
    return RT_OK;
}

int rt_trace_paths_device(const rt_scene *scene, int32_t device, size_t n, const void *d_rays, void *d_rng, uint64_t seed, uint64_t stream_base, uint32_t sample,
                          int32_t bounce_depth, uint32_t flags, const rt_path_outputs *out, void *stream, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_trace_paths(scene, n, d_rays, bounce_depth, out, options));
    RT_TRY(run_device(device, stats, n == 0, [&](bool want_stats, Pending &pd) {
        return launch_trace_paths(scene, device, n, d_rays, d_rng, seed, stream_base, sample, bounce_depth, flags, *out, stream, options, want_stats, pd);
    }));
    if (n) paths_counts(stats, n, (uint64_t) n);
    return RT_OK;
}

int rt_trace_paths(const rt_scene *scene, int32_t device, size_t n, const double *rays, uint32_t *rng, uint64_t seed, uint64_t stream_base, uint32_t sample,
                   int32_t bounce_depth, uint32_t flags, const rt_path_outputs *out, rt_stats *stats) {
    RT_TRY(check_trace_paths(scene, n, rays, bounce_depth, out, nullptr));
    const rt_path_outputs o = host_path_outputs(*out);
    const size_t recs = n * (size_t) o.max_vertices;
    RT_TRY(run_host(device, stats, n == 0, {{rays, n * 48u, SEG_IN}, {rng, n * 16u, SEG_INOUT}, RT_PATH_SEGMENTS(o, n, recs, (size_t) 0)},
                    [&](void *const *d, bool want_stats, Pending &pd) {
        return launch_trace_paths(scene, device, n, d[0], d[1], seed, stream_base, sample, bounce_depth, flags, staged_path_outputs(o, d + 2), nullptr, nullptr,
                                  want_stats, pd);
    }));
    if (n) paths_counts(stats, n, (uint64_t) n);
    return RT_OK;
}

int rt_dev_last_paths_plan(int64_t out[8]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = g_last_paths_plan[i];
    return RT_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// rt_render_frame: one process, several devices, one gather
// ------------------------------------------------------------------------------------------------------------
namespace {

// librccl.so is loaded on first use (dlopen), so the library itself depends on libamdhip64 only.
struct RcclApi {
    typedef int (*init_all_t)(void **, int, const int *);
    typedef int (*destroy_t)(void *);
    typedef int (*group_t)(void);
    typedef int (*send_t)(const void *, size_t, int, int, void *, hipStream_t);
    typedef int (*recv_t)(void *, size_t, int, int, void *, hipStream_t);
    typedef const char *(*errstr_t)(int);
    void *lib = nullptr;
    init_all_t CommInitAll = nullptr;
    destroy_t CommDestroy = nullptr;
    group_t GroupStart = nullptr, GroupEnd = nullptr;
    send_t Send = nullptr;
    recv_t Recv = nullptr;
    errstr_t GetErrorString = nullptr;
    std::string why;
    bool ok() const { return lib != nullptr; }
};
static RcclApi load_rccl() {
    RcclApi r;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) { r.why = std::string("librccl.so could not be loaded: ") + (dlerror() ? dlerror() : "?"); return r; }
    r.CommInitAll = (RcclApi::init_all_t) dlsym(h, "ncclCommInitAll");
    r.CommDestroy = (RcclApi::destroy_t) dlsym(h, "ncclCommDestroy");
    r.GroupStart = (RcclApi::group_t) dlsym(h, "ncclGroupStart");
    r.GroupEnd = (RcclApi::group_t) dlsym(h, "ncclGroupEnd");
    r.Send = (RcclApi::send_t) dlsym(h, "ncclSend");
    r.Recv = (RcclApi::recv_t) dlsym(h, "ncclRecv");
    r.GetErrorString = (RcclApi::errstr_t) dlsym(h, "ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.Send || !r.Recv || !r.GetErrorString) {
        r.why = "librccl.so lacks a needed symbol";
        return r;
    }
    r.lib = h;
    return r;
}
static RcclApi &rccl() { static RcclApi api = load_rccl(); return api; }
#define RT_NCCL_INT32 2 /* ncclInt32 (rccl.h) */

// communicators are expensive to set up (~0.1-1 s): kept per device list for the life of the process.  Calls from several threads
// over the same list share them, so each call's group (ncclGroupStart .. ncclGroupEnd) is issued under the list's mutex: two
// groups interleaved op by op could be matched in different orders on different ranks and hang them.
struct CommSet { std::vector<void *> comms; std::mutex group_mu; };
static std::mutex g_comm_mu;
static std::map<std::vector<int>, CommSet> g_comms;
static int comms_for(const std::vector<int> &devs, CommSet **out) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    auto it = g_comms.find(devs);
    if (it == g_comms.end()) {
        std::vector<void *> c(devs.size(), nullptr);
        const int rc = rccl().CommInitAll(c.data(), (int) devs.size(), devs.data());
        if (rc != 0) return fail(RT_ERR_HIP, std::string("ncclCommInitAll: ") + rccl().GetErrorString(rc));
        it = g_comms.emplace(std::piecewise_construct, std::forward_as_tuple(devs), std::forward_as_tuple()).first;
        it->second.comms = std::move(c);
    }
    *out = &it->second;
    return RT_OK;
}

struct FrameDevice { // one device's share of a frame; everything is released on every exit path
    int device = -1;
    hipStream_t stream = nullptr;
    int32_t *accum = nullptr; // this device's shard
    int32_t *stage = nullptr; // on devices[0]: where this device's shard arrives
    int32_t n_rows = 0;
    Pending pd;
    ~FrameDevice() {
        if (device < 0) return;
        if (hipSetDevice(device) != hipSuccess) return;
        pd.release();
        if (stream) { (void) hipStreamSynchronize(stream); (void) hipStreamDestroy(stream); }
        (void) hipFree(accum);
    }
};

} // namespace

extern "C" {

static int render_frame(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, const int32_t *devices,
                        int32_t n_devices, uint32_t flags, int32_t gather, const rt_render_options *options, int32_t *accum_host, uint8_t *rgb_host,
                        rt_stats *stats) {
    if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
    if (!devices || n_devices < 1 || n_devices > 64) return fail(RT_ERR_INVALID_ARGUMENT, "devices: 1 to 64 device ids");
    if (gather < RT_GATHER_AUTO || gather > RT_GATHER_HOST) return fail(RT_ERR_INVALID_ARGUMENT, "gather must be one of RT_GATHER_*");
    int rc = check_geometry(camera, max_w, max_h, 0, 1, 2 * max_h + 1);
    if (rc != RT_OK) return rc;
    if (!accum_host) return fail(RT_ERR_INVALID_ARGUMENT, "accum_host is NULL");
    const int visible = visible_devices();
    if (visible <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible: the render path has no CPU fallback");
    bool distinct = true;
    for (int i = 0; i < n_devices; ++i) {
        if (devices[i] < 0 || devices[i] >= visible) return fail(RT_ERR_INVALID_ARGUMENT, "device index out of range");
        for (int j = 0; j < i; ++j) distinct = distinct && devices[j] != devices[i];
    }
    if (gather == RT_GATHER_RCCL && !distinct) return fail(RT_ERR_INVALID_ARGUMENT, "RT_GATHER_RCCL needs distinct devices (one communicator rank per GPU)");
    if (gather == RT_GATHER_RCCL && !rccl().ok()) return fail(RT_ERR_UNSUPPORTED, rccl().why);
    const bool viaSelf = gather == RT_GATHER_RCCL; // asked for by name: devices[0]'s own shard goes through ncclSend/ncclRecv as well
    if (gather == RT_GATHER_AUTO) gather = (n_devices > 1 && distinct && rccl().ok()) ? RT_GATHER_RCCL : RT_GATHER_PEER;

    const auto t0 = std::chrono::steady_clock::now();
    const int rows = 2 * max_h + 1, cols = 2 * max_w + 1;
    const size_t rowBytes = (size_t) cols * 16u;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) { (void) hipGetLastError(); prev = -1; }
    struct Restore { int prev; ~Restore() { if (prev >= 0) (void) hipSetDevice(prev); } } restore{prev};

    std::vector<FrameDevice> fd((size_t) n_devices); // destroyed (streams drained, buffers freed) before `restore`
    struct StageOwner { std::vector<int32_t *> bufs; int device; ~StageOwner() { if (hipSetDevice(device) == hipSuccess) for (auto *b : bufs) (void) hipFree(b); } } stages{{}, devices[0]};

    // ---- every device renders its interleaved rows on a stream of its own; nothing waits here ----
    for (int i = 0; i < n_devices; ++i) {
        FrameDevice &f = fd[(size_t) i];
        HIP_TRY(hipSetDevice(devices[i]));
        f.device = devices[i];
        f.n_rows = (rows - i + n_devices - 1) / n_devices;
        if (f.n_rows < 0) f.n_rows = 0;
        HIP_TRY(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
        if (f.n_rows > 0) HIP_TRY(hipMalloc((void **) &f.accum, (size_t) f.n_rows * rowBytes));
        RT_TRY(check_options(options)); // (the one argument not tested above; here, where launch_render used to test it)
        rc = launch_render(scene, camera, max_w, max_h, seed, devices[i], i, n_devices, f.n_rows, flags, f.accum, nullptr, f.stream, options,
                           stats != nullptr, f.pd);
        if (rc != RT_OK) return rc;
    }

    // ---- one gather ----
    const size_t dpitch = (size_t) n_devices * rowBytes;
    auto to_host = [&](const int32_t *src, int i, hipStream_t st) -> hipError_t { // de-interleaving strided copy: shard row j -> image row i + j*n
        if (fd[(size_t) i].n_rows == 0) return hipSuccess;
        return hipMemcpy2DAsync((char *) accum_host + (size_t) i * rowBytes, dpitch, src, rowBytes, rowBytes, (size_t) fd[(size_t) i].n_rows, hipMemcpyDeviceToHost, st);
    };
    if (gather == RT_GATHER_HOST) {
        for (int i = 0; i < n_devices; ++i) {
            HIP_TRY(hipSetDevice(devices[i]));
            HIP_TRY(to_host(fd[(size_t) i].accum, i, fd[(size_t) i].stream));
        }
        for (int i = 0; i < n_devices; ++i) { HIP_TRY(hipSetDevice(devices[i])); HIP_TRY(hipStreamSynchronize(fd[(size_t) i].stream)); }
    } else {
        HIP_TRY(hipSetDevice(devices[0]));
        for (int i = 0; i < n_devices; ++i) {
            int32_t *b = nullptr;
            if ((i > 0 || viaSelf) && fd[(size_t) i].n_rows > 0) HIP_TRY(hipMalloc((void **) &b, (size_t) fd[(size_t) i].n_rows * rowBytes));
            stages.bufs.push_back(b);
            fd[(size_t) i].stage = b;
        }
        if (gather == RT_GATHER_PEER) {
            for (int i = 1; i < n_devices; ++i) {
                if (fd[(size_t) i].n_rows == 0) continue;
                HIP_TRY(hipSetDevice(devices[i]));
                HIP_TRY(hipMemcpyPeerAsync(fd[(size_t) i].stage, devices[0], fd[(size_t) i].accum, devices[i], (size_t) fd[(size_t) i].n_rows * rowBytes, fd[(size_t) i].stream));
            }
            for (int i = 1; i < n_devices; ++i) { HIP_TRY(hipSetDevice(devices[i])); HIP_TRY(hipStreamSynchronize(fd[(size_t) i].stream)); }
        } else { // RCCL over xGMI: every sender on its own render stream, every receive on devices[0]'s
            std::vector<int> devs(devices, devices + n_devices);
            CommSet *set = nullptr;
            rc = comms_for(devs, &set);
            if (rc != RT_OK) return rc;
            const std::vector<void *> *comms = &set->comms;
            RcclApi &nc = rccl();
            // nothing returns between GroupStart and GroupEnd: an early return would leave RCCL in group mode for the rest of the
            // process (the communicators are cached); errors are collected and reported after the group has been closed
            std::unique_lock<std::mutex> group(set->group_mu);
            int e = nc.GroupStart();
            hipError_t he = hipSuccess;
            for (int i = viaSelf ? 0 : 1; i < n_devices && e == 0 && he == hipSuccess; ++i) {
                const size_t count = (size_t) fd[(size_t) i].n_rows * (size_t) cols * 4u;
                if (count == 0) continue;
                he = hipSetDevice(devices[i]);
                if (he != hipSuccess) break;
                e = nc.Send(fd[(size_t) i].accum, count, RT_NCCL_INT32, 0, (*comms)[(size_t) i], fd[(size_t) i].stream);
                if (e != 0) break;
                he = hipSetDevice(devices[0]);
                if (he != hipSuccess) break;
                e = nc.Recv(fd[(size_t) i].stage, count, RT_NCCL_INT32, i, (*comms)[0], fd[0].stream);
            }
            const int e2 = nc.GroupEnd();
            group.unlock();
            if (e == 0) e = e2;
            if (he != hipSuccess) return fail(RT_ERR_HIP, std::string("RCCL gather: hipSetDevice: ") + hipGetErrorString(he));
            if (e != 0) return fail(RT_ERR_HIP, std::string("RCCL gather: ") + nc.GetErrorString(e));
            for (int i = 1; i < n_devices; ++i) { HIP_TRY(hipSetDevice(devices[i])); HIP_TRY(hipStreamSynchronize(fd[(size_t) i].stream)); }
        }
        HIP_TRY(hipSetDevice(devices[0]));
        for (int i = 0; i < n_devices; ++i) HIP_TRY(to_host(fd[(size_t) i].stage ? fd[(size_t) i].stage : fd[(size_t) i].accum, i, fd[0].stream));
        HIP_TRY(hipStreamSynchronize(fd[0].stream));
    }

    if (rgb_host) { // PixelStats.mean (Pixel.fs:103-108): integer division of the sums by Count
        const size_t npx = (size_t) rows * (size_t) cols;
        for (size_t i = 0; i < npx; ++i) {
            const int32_t *a = accum_host + i * 4;
            rgb_host[i * 3 + 0] = (uint8_t) (a[1] / a[0]);
            rgb_host[i * 3 + 1] = (uint8_t) (a[2] / a[0]);
            rgb_host[i * 3 + 2] = (uint8_t) (a[3] / a[0]);
        }
    }
    if (stats) {
        for (int i = 0; i < n_devices; ++i) {
            HIP_TRY(hipSetDevice(devices[i]));
            rc = collect_stats(fd[(size_t) i].pd, &stats[i]);
            if (rc != RT_OK) return rc;
        }
        const double total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        for (int i = 0; i < n_devices; ++i) stats[i].total_ms = total;
    }
    return RT_OK;
}
int rt_render_frame(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, const int32_t *devices,
                    int32_t n_devices, uint32_t flags, int32_t gather, const rt_render_options *options, int32_t *accum_host, uint8_t *rgb_host,
                    rt_stats *stats) {
    return guarded("rt_render_frame", [&]() {
        return render_frame(scene, camera, max_w, max_h, seed, devices, n_devices, flags, gather, options, accum_host, rgb_host, stats);
    });
}

// ---- output side ------------------------------------------------------------------------------------------
uint8_t rt_gamma_correct(uint8_t b) { return rth::gamma_correct(b); }

int64_t rt_format_ppm(const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct, char *out, size_t out_capacity) {
    if (!rgb || rows <= 0 || cols <= 0) { fail(RT_ERR_INVALID_ARGUMENT, "bad image"); return -RT_ERR_INVALID_ARGUMENT; }
    return guarded<int64_t>("rt_format_ppm", [&]() {
        std::string s = rth::format_ppm(rgb, rows, cols, gamma_correct != 0);
        if (out && out_capacity > s.size()) { memcpy(out, s.data(), s.size()); out[s.size()] = 0; }
        return (int64_t) s.size();
    }, -RT_ERR_HOST);
}

int64_t rt_format_pixel_map(const uint8_t *rgb, int32_t rows, int32_t cols, uint8_t *out, size_t out_capacity) {
    if (!rgb || rows <= 0 || cols <= 0) { fail(RT_ERR_INVALID_ARGUMENT, "bad image"); return -RT_ERR_INVALID_ARGUMENT; }
    return guarded<int64_t>("rt_format_pixel_map", [&]() {
        std::string s = rth::format_pixel_map(rgb, rows, cols);
        if (out && out_capacity >= s.size()) memcpy(out, s.data(), s.size());
        return (int64_t) s.size();
    }, -RT_ERR_HOST);
}

int64_t rt_parse_pixel_map(const uint8_t *data, size_t n, int32_t rows, int32_t cols, uint8_t *rgb_out, uint8_t *present_out) {
    if ((!data && n) || rows <= 0 || cols <= 0 || !rgb_out) { fail(RT_ERR_INVALID_ARGUMENT, "bad argument"); return -RT_ERR_INVALID_ARGUMENT; }
    if (present_out) memset(present_out, 0, (size_t) rows * (size_t) cols);
    const int64_t c = rth::parse_pixel_map(data, n, rows, cols, rgb_out, present_out);
    if (c < 0) { fail(RT_ERR_INVALID_ARGUMENT, "pixel map names a pixel outside the image"); return -RT_ERR_INVALID_ARGUMENT; }
    return c;
}

int rt_write_ppm(const char *path, const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct) {
    if (!path || !rgb || rows <= 0 || cols <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad image or path");
    return guarded("rt_write_ppm", [&]() {
        std::string s = rth::format_ppm(rgb, rows, cols, gamma_correct != 0);
        FILE *f = fopen(path, "wb");
        if (!f) return fail(RT_ERR_IO, std::string("cannot open ") + path);
        const size_t w = fwrite(s.data(), 1, s.size(), f);
        const int c = fclose(f);
        if (w != s.size() || c != 0) return fail(RT_ERR_IO, std::string("short write to ") + path);
        return (int) RT_OK;
    });
}

} // extern "C"

static int check_image_size(int32_t rows, int32_t cols);
static int check_png_size(int32_t rows, int32_t cols) { // after check_image_size
    if (!rtp::supported((uint64_t) rows, (uint64_t) cols)) return fail(RT_ERR_UNSUPPORTED, "an image whose PNG data may pass 2^31 - 1 bytes");
    return RT_OK;
}
static void fill_gamma(uint8_t *t, bool gamma) { // the ONE definition, rth::gamma_correct, tabulated; the identity when gamma is off
    for (int i = 0; i < 256; ++i) t[i] = gamma ? rth::gamma_correct((uint8_t) i) : (uint8_t) i;
}
// Png.write's file (rt_png.h) of a host image
static std::vector<uint8_t> host_png(const uint8_t *rgb, int32_t rows, int32_t cols, bool gamma) {
    uint8_t table[256];
    fill_gamma(table, gamma);
    std::vector<uint8_t> file((size_t) rtp::max_bytes((uint64_t) rows, (uint64_t) cols));
    file.resize((size_t) rtp::format_png(rgb, (uint32_t) rows, (uint32_t) cols, table, file.data()));
    return file;
}

extern "C" {

int64_t rt_format_png(const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct, uint8_t *out, size_t out_capacity) {
    if (!rgb) { fail(RT_ERR_INVALID_ARGUMENT, "bad image"); return -RT_ERR_INVALID_ARGUMENT; }
    if (check_image_size(rows, cols) != RT_OK) return -RT_ERR_INVALID_ARGUMENT;
    if (check_png_size(rows, cols) != RT_OK) return -RT_ERR_UNSUPPORTED;
    return guarded<int64_t>("rt_format_png", [&]() {
        const std::vector<uint8_t> file = host_png(rgb, rows, cols, gamma_correct != 0);
        if (out && out_capacity < file.size()) { // nothing is written
            fail(RT_ERR_INVALID_ARGUMENT, "out_capacity " + std::to_string(out_capacity) + " below the " + std::to_string(file.size()) + " bytes needed");
            return (int64_t) -RT_ERR_INVALID_ARGUMENT;
        }
        if (out) memcpy(out, file.data(), file.size());
        return (int64_t) file.size();
    }, -RT_ERR_HOST);
}

int rt_write_png(const char *path, const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct) {
    if (!path || !rgb) return fail(RT_ERR_INVALID_ARGUMENT, "bad image or path");
    RT_TRY(check_image_size(rows, cols));
    RT_TRY(check_png_size(rows, cols));
    return guarded("rt_write_png", [&]() {
        const std::vector<uint8_t> file = host_png(rgb, rows, cols, gamma_correct != 0);
        FILE *f = fopen(path, "wb");
        if (!f) return fail(RT_ERR_IO, std::string("cannot open ") + path);
        const size_t w = fwrite(file.data(), 1, file.size(), f);
        const int c = fclose(f);
        if (w != file.size() || c != 0) return fail(RT_ERR_IO, std::string("short write to ") + path);
        return (int) RT_OK;
    });
}

int32_t rt_png_tile_bytes(void) { return RTO_PNG_TILE_BYTES; }

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// output on the device (rt_output.h): the same bytes as rth::format_ppm / rth::format_pixel_map, from an image that is already there
// ------------------------------------------------------------------------------------------------------------
namespace {

struct FormatJob {
    int fmt; // rto::FMT_PPM, rto::FMT_MAP or rto::FMT_PNG
    const void *d_rgb;
    int32_t rows, cols;
    bool gamma;
    void *d_out;
    size_t capacity;
    void *d_length;
};
// A format call's stream-ordered scratch (rto::FormatScratch, then one uint64 per tile): given back to the stream's pool on every exit path.
struct FormatPending {
    unsigned char *scr = nullptr;
    hipStream_t st = nullptr;
    ~FormatPending() { if (scr) (void) hipFreeAsync(scr, st); }
};
// Stream-ordered device memory of the calls that own their buffers (rt_write_ppm_device, rt_render_ppm).
struct StreamBuf {
    unsigned char *p = nullptr;
    hipStream_t st = nullptr;
    ~StreamBuf() { if (p) (void) hipFreeAsync(p, st); }
};
struct FileCloser {
    FILE *f = nullptr;
    ~FileCloser() { if (f) (void) fclose(f); }
};

} // namespace

static int check_image_size(int32_t rows, int32_t cols) {
    if (rows <= 0 || cols <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rows and cols must be positive");
    if ((uint64_t) rows * (uint64_t) cols > (uint64_t) INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "an image of more than INT32_MAX pixels");
    return RT_OK;
}
static int check_format(const void *d_rgb, int32_t rows, int32_t cols, const void *d_out, size_t out_capacity) {
    if (!d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "d_rgb is NULL");
    RT_TRY(check_image_size(rows, cols));
    if (d_out && out_capacity == 0) return fail(RT_ERR_INVALID_ARGUMENT, "d_out is given but out_capacity is 0");
    return RT_OK;
}
static rto::PpmHeader ppm_header(int32_t rows, int32_t cols) { // "P3\n<cols> <rows>\n255\n" (ImageOutput.fs:166-176)
    rto::PpmHeader h{};
    h.len = (uint32_t) snprintf((char *) h.text, sizeof(h.text), "P3\n%d %d\n255\n", cols, rows);
    return h;
}
static rto::GammaTable gamma_table(bool gamma) {
    rto::GammaTable t;
    fill_gamma(t.v, gamma);
    return t;
}
static int64_t ascii_int_digits_below(int64_t n) { // sum of writeAsciiInt's digit counts over 0 .. n-1 (0 has none): sum over k of max(0, n - 10^k)
    int64_t sum = 0;
    for (int64_t p = 1; p < n; p *= 10) sum += n - p;
    return sum;
}

// The PNG of rt_png.h (rt_png_kernels.h): sums, the same scan over the tiles and the file's tail, and -- when there is a buffer -- scatter
// and finish.  Scratch: the head, one uint64 per tile and one for the tail, one PngPartial per tile.
static int enqueue_png(const FormatJob &j, hipStream_t st, FormatPending &fp) {
    const uint32_t N = (uint32_t) rtp::filtered_bytes((uint64_t) j.rows, (uint64_t) j.cols), n_tiles = (uint32_t) rtp::tile_count((uint64_t) j.rows, (uint64_t) j.cols);
    const size_t parts_at = RTO_SCRATCH_HEAD + ((size_t) n_tiles + 1u) * sizeof(unsigned long long);
    HIP_TRY(hipMallocAsync((void **) &fp.scr, parts_at + (size_t) n_tiles * sizeof(rto::PngPartial), st));
    fp.st = st;
    rto::FormatScratch *head = (rto::FormatScratch *) fp.scr;
    unsigned long long *tiles = (unsigned long long *) (fp.scr + RTO_SCRATCH_HEAD);
    rto::PngPartial *parts = (rto::PngPartial *) (fp.scr + parts_at);
    const unsigned char *rgb = (const unsigned char *) j.d_rgb;
    const rto::GammaTable g = gamma_table(j.gamma);
    hipLaunchKernelGGL(rto::png_sums_kernel, dim3(n_tiles), dim3(RTO_BLOCK), 0, st, rgb, N, (uint32_t) j.cols, g, tiles, n_tiles);
    hipLaunchKernelGGL(rto::format_scan_kernel, dim3(1), dim3(RTO_SCAN_THREADS), 0, st, tiles, n_tiles + 1u, (unsigned long long) rtp::HEAD_BYTES, head,
                       (long long *) j.d_length, (unsigned long long) j.capacity, j.d_out ? 1 : 0);
    if (j.d_out) {
        hipLaunchKernelGGL(rto::png_scatter_kernel, dim3(n_tiles), dim3(RTO_BLOCK), 0, st, rgb, N, (uint32_t) j.cols, g, (const unsigned long long *) tiles,
                           (const rto::FormatScratch *) head, parts, (unsigned char *) j.d_out);
        hipLaunchKernelGGL(rto::png_finish_kernel, dim3(1), dim3(RTO_BLOCK), 0, st, (uint32_t) j.rows, (uint32_t) j.cols, N, (const unsigned long long *) tiles, n_tiles,
                           (const rto::FormatScratch *) head, (const rto::PngPartial *) parts, (unsigned char *) j.d_out);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Enqueues one format on `stream` (arguments checked, the device current): sums, scan and -- when there is a buffer -- the scatter.
// Never waits for the device.
static int enqueue_format(const FormatJob &j, void *stream, FormatPending &fp) {
    hipStream_t st = (hipStream_t) stream;
    if (j.fmt == rto::FMT_PNG) return enqueue_png(j, st, fp);
    const uint32_t npx = (uint32_t) ((uint64_t) j.rows * (uint64_t) j.cols);
    const uint32_t n_tiles = (npx + (uint32_t) RTO_TILE_PIXELS - 1u) / (uint32_t) RTO_TILE_PIXELS;
    HIP_TRY(hipMallocAsync((void **) &fp.scr, RTO_SCRATCH_HEAD + (size_t) n_tiles * sizeof(unsigned long long), st));
    fp.st = st;
    rto::FormatScratch *head = (rto::FormatScratch *) fp.scr;
    unsigned long long *tiles = (unsigned long long *) (fp.scr + RTO_SCRATCH_HEAD);
    const unsigned char *rgb = (const unsigned char *) j.d_rgb;
    const rto::GammaTable g = gamma_table(j.gamma);
    const rto::PpmHeader hdr = j.fmt == rto::FMT_PPM ? ppm_header(j.rows, j.cols) : rto::PpmHeader{};
    if (j.fmt == rto::FMT_PPM) hipLaunchKernelGGL(rto::format_sums_kernel<rto::FMT_PPM>, dim3(n_tiles), dim3(RTO_BLOCK), 0, st, rgb, npx, (uint32_t) j.cols, g, tiles);
    else hipLaunchKernelGGL(rto::format_sums_kernel<rto::FMT_MAP>, dim3(n_tiles), dim3(RTO_BLOCK), 0, st, rgb, npx, (uint32_t) j.cols, g, tiles);
    hipLaunchKernelGGL(rto::format_scan_kernel, dim3(1), dim3(RTO_SCAN_THREADS), 0, st, tiles, n_tiles, (unsigned long long) hdr.len, head, (long long *) j.d_length,
                       (unsigned long long) j.capacity, j.d_out ? 1 : 0);
    if (j.d_out) {
#ifdef RTO_PLAIN_STORES
        constexpr bool staged = false;
#else
        constexpr bool staged = true;
#endif
        if (j.fmt == rto::FMT_PPM)
            hipLaunchKernelGGL((rto::format_scatter_kernel<rto::FMT_PPM, staged>), dim3(n_tiles), dim3(RTO_BLOCK), 0, st, rgb, npx, (uint32_t) j.cols, g, hdr,
                               (const unsigned long long *) tiles, (const rto::FormatScratch *) head, (unsigned char *) j.d_out);
        else
            hipLaunchKernelGGL((rto::format_scatter_kernel<rto::FMT_MAP, staged>), dim3(n_tiles), dim3(RTO_BLOCK), 0, st, rgb, npx, (uint32_t) j.cols, g, hdr,
                               (const unsigned long long *) tiles, (const rto::FormatScratch *) head, (unsigned char *) j.d_out);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
// Waits for the stream, reads the needed length and reports a buffer the device found too small (it wrote none of it).
static int finish_format(FormatPending &fp, const FormatJob &j, int64_t *length) {
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, fp.scr + offsetof(rto::FormatScratch, total), sizeof(total), hipMemcpyDeviceToHost, fp.st));
    HIP_TRY(hipStreamSynchronize(fp.st));
    *length = (int64_t) total;
    if (j.d_out && (unsigned long long) total > (unsigned long long) j.capacity)
        return fail(RT_ERR_INVALID_ARGUMENT, "out_capacity " + std::to_string(j.capacity) + " below the " + std::to_string(total) + " bytes needed");
    return RT_OK;
}
static int run_format(int32_t device, const FormatJob &j, void *stream, int64_t *length) {
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    FormatPending fp;
    RT_TRY(enqueue_format(j, stream, fp));
    return length ? finish_format(fp, j, length) : RT_OK;
}
// The P3 text or the PNG of a device image in host memory (the device current): a device buffer of rt_ppm_max_bytes / rt_png_max_bytes from
// the stream's pool, the format, and ONE device-to-host copy of exactly the file.  Waits for the stream.
static int file_to_host(int fmt, const void *d_rgb, int32_t rows, int32_t cols, bool gamma, hipStream_t st, unsigned char *d_text, size_t capacity,
                        std::unique_ptr<char[]> &text, int64_t &len) {
    const FormatJob j{fmt, d_rgb, rows, cols, gamma, d_text, capacity, nullptr};
    FormatPending fp;
    RT_TRY(enqueue_format(j, st, fp));
    RT_TRY(finish_format(fp, j, &len));
    text.reset(new char[(size_t) len]);
    HIP_TRY(hipMemcpyAsync(text.get(), d_text, (size_t) len, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}
static int write_all(FileCloser &file, const char *path, const char *text, int64_t len) {
    const size_t w = fwrite(text, 1, (size_t) len, file.f);
    const int c = fclose(file.f);
    file.f = nullptr;
    if (w != (size_t) len || c != 0) return fail(RT_ERR_IO, std::string("short write to ") + path);
    return RT_OK;
}

static int64_t file_max_bytes(int fmt, int32_t rows, int32_t cols); // rt_ppm_max_bytes / rt_png_max_bytes

// rt_write_ppm_device / rt_write_png_device: one body, so that the two keep one check list and one order of events.
static int write_file_device(const char *name, int fmt, const char *path, int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct,
                             void *stream) {
    if (!path) return fail(RT_ERR_INVALID_ARGUMENT, "path is NULL");
    RT_TRY(check_format(d_rgb, rows, cols, nullptr, 0));
    if (fmt == rto::FMT_PNG) RT_TRY(check_png_size(rows, cols));
    return guarded(name, [&]() {
        FileCloser file;
        if (!(file.f = fopen(path, "wb"))) return fail(RT_ERR_IO, std::string("cannot open ") + path);
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        const size_t capacity = (size_t) file_max_bytes(fmt, rows, cols);
        StreamBuf d_text;
        d_text.st = (hipStream_t) stream;
        HIP_TRY(hipMallocAsync((void **) &d_text.p, capacity, d_text.st));
        std::unique_ptr<char[]> text;
        int64_t len = 0;
        RT_TRY(file_to_host(fmt, d_rgb, rows, cols, gamma_correct != 0, d_text.st, d_text.p, capacity, text, len));
        return write_all(file, path, text.get(), len);
    });
}

// rt_render_ppm / rt_render_png
static int render_file(const char *name, int fmt, const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                       uint32_t flags, int32_t gamma_correct, const char *path, const rt_render_options *options, rt_stats *stats) {
    const int32_t rows = (max_h > 0 && max_h <= (1 << 20)) ? 2 * max_h + 1 : 0, cols = (max_w > 0 && max_w <= (1 << 20)) ? 2 * max_w + 1 : 0;
    RT_TRY(check_frame(scene, camera, max_w, max_h, 0, 1, rows, scene, "", options)); // rt_render's check list (the buffers are this call's own)
    if (!path) return fail(RT_ERR_INVALID_ARGUMENT, "path is NULL");
    RT_TRY(check_image_size(rows, cols));
    if (fmt == rto::FMT_PNG) RT_TRY(check_png_size(rows, cols));
    return guarded(name, [&]() {
        const auto t0 = std::chrono::steady_clock::now();
        FileCloser file;
        if (!(file.f = fopen(path, "wb"))) return fail(RT_ERR_IO, std::string("cannot open ") + path);
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        // accum, rgb and the file in ONE allocation from the null stream's pool; the pixels never visit the host as rgb
        const size_t npx = (size_t) rows * (size_t) cols, capacity = (size_t) file_max_bytes(fmt, rows, cols), rgb_at = npx * 16u,
                     text_at = rgb_at + ((npx * 3u + 15u) & ~(size_t) 15u);
        StreamBuf buf;
        HIP_TRY(hipMallocAsync((void **) &buf.p, text_at + capacity, buf.st));
        rt_stats local;
        {
            Pending pd;
            RT_TRY(launch_render(scene, camera, max_w, max_h, seed, device, 0, 1, rows, flags, buf.p, buf.p + rgb_at, nullptr, options, true, pd));
            RT_TRY(collect_stats(pd, &local));
        }
        std::unique_ptr<char[]> text;
        int64_t len = 0;
        RT_TRY(file_to_host(fmt, buf.p + rgb_at, rows, cols, gamma_correct != 0, buf.st, buf.p + text_at, capacity, text, len));
        RT_TRY(write_all(file, path, text.get(), len));
        if (stats) {
            *stats = local;
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return (int) RT_OK;
    });
}

extern "C" {

int64_t rt_ppm_max_bytes(int32_t rows, int32_t cols) {
    if (check_image_size(rows, cols) != RT_OK) return -RT_ERR_INVALID_ARGUMENT;
    return (int64_t) ppm_header(rows, cols).len + (int64_t) RTO_PPM_PIXEL_BYTES * (int64_t) rows * (int64_t) cols - 1;
}

int64_t rt_png_max_bytes(int32_t rows, int32_t cols) {
    if (check_image_size(rows, cols) != RT_OK) return -RT_ERR_INVALID_ARGUMENT;
    if (check_png_size(rows, cols) != RT_OK) return -RT_ERR_UNSUPPORTED;
    return (int64_t) rtp::max_bytes((uint64_t) rows, (uint64_t) cols);
}

int64_t rt_pixel_map_bytes(int32_t rows, int32_t cols) {
    if (check_image_size(rows, cols) != RT_OK) return -RT_ERR_INVALID_ARGUMENT;
    return (int64_t) cols * ascii_int_digits_below(rows) + (int64_t) rows * ascii_int_digits_below(cols) + 5 * (int64_t) rows * (int64_t) cols;
}

int rt_gamma_correct_device(int32_t device, size_t n, const void *d_in, void *d_out, void *stream) {
    if (n > 0 && !d_in) return fail(RT_ERR_INVALID_ARGUMENT, "d_in is NULL");
    if (n > 0 && !d_out) return fail(RT_ERR_INVALID_ARGUMENT, "d_out is NULL");
    if (n == 0) return RT_OK;
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const size_t want = (n / 4u + RTO_BLOCK - 1u) / RTO_BLOCK + 1u;
    hipLaunchKernelGGL(rto::gamma_kernel, dim3((unsigned) (want < 4096u ? want : 4096u)), dim3(RTO_BLOCK), 0, (hipStream_t) stream, (const unsigned char *) d_in,
                       (unsigned char *) d_out, (unsigned long long) n, gamma_table(true));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_format_ppm_device(int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct, void *d_out, size_t out_capacity,
                         void *d_length, void *stream, int64_t *length) {
    RT_TRY(check_format(d_rgb, rows, cols, d_out, out_capacity));
    return run_format(device, FormatJob{rto::FMT_PPM, d_rgb, rows, cols, gamma_correct != 0, d_out, out_capacity, d_length}, stream, length);
}

int rt_format_pixel_map_device(int32_t device, const void *d_rgb, int32_t rows, int32_t cols, void *d_out, size_t out_capacity, void *d_length,
                               void *stream, int64_t *length) {
    RT_TRY(check_format(d_rgb, rows, cols, d_out, out_capacity));
    return run_format(device, FormatJob{rto::FMT_MAP, d_rgb, rows, cols, false, d_out, out_capacity, d_length}, stream, length);
}

int rt_format_png_device(int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct, void *d_out, size_t out_capacity,
                         void *d_length, void *stream, int64_t *length) {
    RT_TRY(check_format(d_rgb, rows, cols, d_out, out_capacity));
    RT_TRY(check_png_size(rows, cols));
    return run_format(device, FormatJob{rto::FMT_PNG, d_rgb, rows, cols, gamma_correct != 0, d_out, out_capacity, d_length}, stream, length);
}

int rt_write_ppm_device(const char *path, int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct, void *stream) {
    return write_file_device("rt_write_ppm_device", rto::FMT_PPM, path, device, d_rgb, rows, cols, gamma_correct, stream);
}
int rt_write_png_device(const char *path, int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct, void *stream) {
    return write_file_device("rt_write_png_device", rto::FMT_PNG, path, device, d_rgb, rows, cols, gamma_correct, stream);
}

int rt_render_ppm(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, uint32_t flags,
                  int32_t gamma_correct, const char *path, const rt_render_options *options, rt_stats *stats) {
    return render_file("rt_render_ppm", rto::FMT_PPM, scene, camera, max_w, max_h, seed, device, flags, gamma_correct, path, options, stats);
}
int rt_render_png(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, uint32_t flags,
                  int32_t gamma_correct, const char *path, const rt_render_options *options, rt_stats *stats) {
    return render_file("rt_render_png", rto::FMT_PNG, scene, camera, max_w, max_h, seed, device, flags, gamma_correct, path, options, stats);
}

} // extern "C"

static int64_t file_max_bytes(int fmt, int32_t rows, int32_t cols) { return fmt == rto::FMT_PNG ? rt_png_max_bytes(rows, cols) : rt_ppm_max_bytes(rows, cols); }

// ------------------------------------------------------------------------------------------------------------
// PNG files of a batch of views (DESIGN.md "PNG files of a batch of views"): the K equal-sized images of rt_render_views' rgb encoded in the
// same four launches as one image (rt_png_kernels.h "a batch of equal-sized images"; the layout is rt_png.h's), file v byte for byte
// rt_format_png of image v
// ------------------------------------------------------------------------------------------------------------
namespace {
struct PngViewsJob {
    const void *d_rgb;
    int32_t n_views, rows, cols;
    bool gamma;
    void *d_out;
    size_t capacity;
    void *d_offsets;
};
} // namespace

// Every argument check of the batch encode, before anything touches a device.
static int check_png_views(const void *d_rgb, int32_t n_views, int32_t rows, int32_t cols, const void *d_out, size_t out_capacity) {
    if (n_views < 0) return fail(RT_ERR_INVALID_ARGUMENT, "n_views must be >= 0");
    if (n_views > 0 && !d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "d_rgb is NULL");
    RT_TRY(check_image_size(rows, cols));
    if ((uint64_t) n_views * (uint64_t) rows * (uint64_t) cols > (uint64_t) INT32_MAX) return fail(RT_ERR_INVALID_ARGUMENT, "a batch of views holds at most INT32_MAX pixels");
    if (d_out && out_capacity == 0) return fail(RT_ERR_INVALID_ARGUMENT, "d_out is given but out_capacity is 0");
    return check_png_size(rows, cols);
}
static int check_paths(const char *const *paths, int32_t n_views) {
    if (!paths) return fail(RT_ERR_INVALID_ARGUMENT, "paths is NULL");
    for (int32_t v = 0; v < n_views; ++v)
        if (!paths[v]) return fail(RT_ERR_INVALID_ARGUMENT, "paths[" + std::to_string(v) + "] is NULL");
    return RT_OK;
}

// Enqueues the batch encode on `st` (n_views > 0, arguments checked, the device current): sums, scan and -- when there is a buffer -- scatter
// and finish.  Scratch: the head, the K + 1 file starts, one uint64 per scan entry, one PngPartial per tile.  Never waits for the device.
static int enqueue_png_views(const PngViewsJob &j, hipStream_t st, FormatPending &fp, size_t &offsets_at) {
    rto::PngViews b;
    b.rgb = (const unsigned char *) j.d_rgb;
    b.image_bytes = (unsigned long long) j.rows * (unsigned long long) j.cols * 3ull;
    b.n_views = (uint32_t) j.n_views;
    b.tiles = (uint32_t) rtp::tile_count((uint64_t) j.rows, (uint64_t) j.cols);
    b.rows = (uint32_t) j.rows; b.cols = (uint32_t) j.cols;
    b.N = (uint32_t) rtp::filtered_bytes((uint64_t) j.rows, (uint64_t) j.cols);
    const size_t n_entries = (size_t) rtp::views_entry_count(b.n_views, b.tiles), n_tiles = (size_t) b.n_views * (size_t) b.tiles; // n_tiles <= the batch's pixels
    offsets_at = RTO_SCRATCH_HEAD;
    const size_t entries_at = offsets_at + ((size_t) j.n_views + 1u) * sizeof(long long), parts_at = entries_at + n_entries * sizeof(unsigned long long);
    HIP_TRY(hipMallocAsync((void **) &fp.scr, parts_at + n_tiles * sizeof(rto::PngPartial), st));
    fp.st = st;
    rto::FormatScratch *head = (rto::FormatScratch *) fp.scr;
    long long *offsets = (long long *) (fp.scr + offsets_at);
    unsigned long long *entries = (unsigned long long *) (fp.scr + entries_at);
    rto::PngPartial *parts = (rto::PngPartial *) (fp.scr + parts_at);
    const rto::GammaTable g = gamma_table(j.gamma);
    hipLaunchKernelGGL(rto::png_views_sums_kernel, dim3((unsigned) n_tiles), dim3(RTO_BLOCK), 0, st, b, g, entries);
    hipLaunchKernelGGL(rto::png_views_scan_kernel, dim3(1), dim3(RTO_SCAN_THREADS), 0, st, entries, b, head, offsets, (long long *) j.d_offsets,
                       (unsigned long long) j.capacity, j.d_out ? 1 : 0);
    if (j.d_out) {
        hipLaunchKernelGGL(rto::png_views_scatter_kernel, dim3((unsigned) n_tiles), dim3(RTO_BLOCK), 0, st, b, g, (const unsigned long long *) entries,
                           (const rto::FormatScratch *) head, parts, (unsigned char *) j.d_out);
        hipLaunchKernelGGL(rto::png_views_finish_kernel, dim3(b.n_views), dim3(RTO_BLOCK), 0, st, b, (const unsigned long long *) entries, (const rto::FormatScratch *) head,
                           (const rto::PngPartial *) parts, (unsigned char *) j.d_out);
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
// Waits for the stream, reads the K + 1 file starts and reports a buffer the device found too small (it wrote none of it).
static int finish_png_views(FormatPending &fp, const PngViewsJob &j, size_t offsets_at, int64_t *offsets) {
    HIP_TRY(hipMemcpyAsync(offsets, fp.scr + offsets_at, ((size_t) j.n_views + 1u) * sizeof(int64_t), hipMemcpyDeviceToHost, fp.st));
    HIP_TRY(hipStreamSynchronize(fp.st));
    const int64_t total = offsets[j.n_views];
    if (j.d_out && (unsigned long long) total > (unsigned long long) j.capacity)
        return fail(RT_ERR_INVALID_ARGUMENT, "out_capacity " + std::to_string(j.capacity) + " below the " + std::to_string(total) + " bytes needed");
    return RT_OK;
}
// The K files of a device batch in host memory (the device current, n_views > 0): the encode into d_files, the offsets, and ONE device-to-host
// copy of exactly the files.  Waits for the stream.
static int png_views_to_host(const void *d_rgb, int32_t n_views, int32_t rows, int32_t cols, bool gamma, hipStream_t st, unsigned char *d_files, size_t capacity,
                             std::vector<int64_t> &offsets, std::unique_ptr<char[]> &files) {
    const PngViewsJob j{d_rgb, n_views, rows, cols, gamma, d_files, capacity, nullptr};
    FormatPending fp;
    size_t offsets_at = 0;
    offsets.assign((size_t) n_views + 1u, 0);
    RT_TRY(enqueue_png_views(j, st, fp, offsets_at));
    RT_TRY(finish_png_views(fp, j, offsets_at, offsets.data()));
    files.reset(new char[(size_t) offsets[(size_t) n_views]]);
    HIP_TRY(hipMemcpyAsync(files.get(), d_files, (size_t) offsets[(size_t) n_views], hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}
// paths[v] written for v = 0 .. n_views - 1, one file open at a time (K may pass the descriptor limit); the first that fails ends the call,
// the files before it stay.
static int write_png_views(const char *const *paths, int32_t n_views, const char *files, const int64_t *offsets) {
    for (int32_t v = 0; v < n_views; ++v) {
        FileCloser file;
        if (!(file.f = fopen(paths[v], "wb"))) return fail(RT_ERR_IO, std::string("cannot open ") + paths[v]);
        RT_TRY(write_all(file, paths[v], files + offsets[v], offsets[v + 1] - offsets[v]));
    }
    return RT_OK;
}

extern "C" {

int64_t rt_png_views_max_bytes(int32_t n_views, int32_t rows, int32_t cols) {
    const unsigned char none = 0; // (no image is looked at: the size checks of the encode, in its order)
    const int rc = check_png_views(&none, n_views, rows, cols, nullptr, 0);
    return rc != RT_OK ? -(int64_t) rc : (int64_t) rtp::views_max_bytes((uint64_t) n_views, (uint64_t) rows, (uint64_t) cols);
}

int rt_format_png_views_device(int32_t device, const void *d_rgb, int32_t n_views, int32_t rows, int32_t cols, int32_t gamma_correct, void *d_out, size_t out_capacity,
                               void *d_offsets, void *stream, int64_t *offsets) {
    RT_TRY(check_png_views(d_rgb, n_views, rows, cols, d_out, out_capacity));
    if (n_views == 0 && !d_offsets) { // no image, no file: nothing for a device to do
        if (offsets) offsets[0] = 0;
        return RT_OK;
    }
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    if (n_views == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(int64_t), (hipStream_t) stream));
        if (offsets) { offsets[0] = 0; HIP_TRY(hipStreamSynchronize((hipStream_t) stream)); }
        return RT_OK;
    }
    const PngViewsJob j{d_rgb, n_views, rows, cols, gamma_correct != 0, d_out, out_capacity, d_offsets};
    FormatPending fp;
    size_t offsets_at = 0;
    RT_TRY(enqueue_png_views(j, (hipStream_t) stream, fp, offsets_at));
    return offsets ? finish_png_views(fp, j, offsets_at, offsets) : RT_OK;
}

int rt_write_png_views_device(const char *const *paths, int32_t device, const void *d_rgb, int32_t n_views, int32_t rows, int32_t cols, int32_t gamma_correct,
                              void *stream) {
    RT_TRY(check_png_views(d_rgb, n_views, rows, cols, nullptr, 0));
    RT_TRY(check_paths(paths, n_views));
    if (n_views == 0) return RT_OK;
    return guarded("rt_write_png_views_device", [&]() {
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        const size_t capacity = (size_t) rtp::views_max_bytes((uint64_t) n_views, (uint64_t) rows, (uint64_t) cols);
        StreamBuf d_files;
        d_files.st = (hipStream_t) stream;
        HIP_TRY(hipMallocAsync((void **) &d_files.p, capacity, d_files.st));
        std::vector<int64_t> offsets;
        std::unique_ptr<char[]> files;
        RT_TRY(png_views_to_host(d_rgb, n_views, rows, cols, gamma_correct != 0, d_files.st, d_files.p, capacity, offsets, files));
        return write_png_views(paths, n_views, files.get(), offsets.data());
    });
}

int rt_render_views_png(const rt_scene *scene, const rt_camera *cameras, int32_t n_views, int32_t max_w, int32_t max_h, const uint64_t *seeds, uint64_t seed,
                        int32_t device, uint32_t flags, int32_t gamma_correct, const char *const *paths, const rt_render_options *options, rt_stats *stats) {
    RT_TRY(check_views(scene, cameras, n_views, max_w, max_h, scene, options)); // rt_render_views' check list (the buffers are this call's own)
    RT_TRY(check_paths(paths, n_views));
    if (n_views == 0) return nothing_to_do(stats);
    const int32_t rows = 2 * max_h + 1, cols = 2 * max_w + 1;
    RT_TRY(check_png_size(rows, cols));
    return guarded("rt_render_views_png", [&]() {
        const auto t0 = std::chrono::steady_clock::now();
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        // accum, rgb and the files in ONE allocation from the null stream's pool; the pixels never visit the host as rgb
        const size_t npx = (size_t) n_views * (size_t) rows * (size_t) cols, capacity = (size_t) rtp::views_max_bytes((uint64_t) n_views, (uint64_t) rows, (uint64_t) cols),
                     rgb_at = npx * 16u, files_at = rgb_at + ((npx * 3u + 15u) & ~(size_t) 15u);
        StreamBuf buf;
        HIP_TRY(hipMallocAsync((void **) &buf.p, files_at + capacity, buf.st));
        rt_stats local;
        {
            Pending pd;
            RT_TRY(launch_views(scene, cameras, n_views, max_w, max_h, seeds, seed, device, flags, buf.p, buf.p + rgb_at, nullptr, options, true, pd));
            RT_TRY(collect_stats(pd, &local));
        }
        std::vector<int64_t> offsets;
        std::unique_ptr<char[]> files;
        RT_TRY(png_views_to_host(buf.p + rgb_at, n_views, rows, cols, gamma_correct != 0, buf.st, buf.p + files_at, capacity, offsets, files));
        RT_TRY(write_png_views(paths, n_views, files.get(), offsets.data()));
        if (stats) {
            *stats = local;
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return (int) RT_OK;
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// resuming from a pixel map (rt_pixel_map.h, rt_pixel_map_kernels.h; DESIGN.md "Resuming from a pixel map"): ImageOutput.readPixelMap
// (ImageOutput.fs:46-113) from bytes on the device, the list of the pixels a presence map lacks, the scatter of a rendered list into a
// frame, and Program.fs:45-50 with the missing pixels rendered where ImageOutput.assertComplete would throw
// ------------------------------------------------------------------------------------------------------------
static const char *const kMalformedMap = "pixel map names a pixel outside the image; nothing was written";

static int check_map_bytes(const void *data, size_t n_bytes) {
    if (n_bytes > 0 && !data) return fail(RT_ERR_INVALID_ARGUMENT, "the pixel map's bytes are NULL");
    return RT_OK;
}
static int check_map_size(size_t n_bytes) { // after every RT_ERR_INVALID_ARGUMENT
    if (n_bytes > (size_t) INT32_MAX) return fail(RT_ERR_UNSUPPORTED, "a pixel map of more than INT32_MAX bytes");
    return RT_OK;
}
static int check_parse(const void *d_data, size_t n_bytes, int32_t rows, int32_t cols, const void *d_rgb, const void *d_present) {
    RT_TRY(check_map_bytes(d_data, n_bytes));
    RT_TRY(check_image_size(rows, cols));
    if (!d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "d_rgb is NULL");
    if (!d_present) return fail(RT_ERR_INVALID_ARGUMENT, "d_present is NULL");
    return check_map_size(n_bytes);
}
static int check_missing(const void *d_present, int32_t rows, int32_t cols, const void *d_pixels, size_t capacity) {
    if (!d_present) return fail(RT_ERR_INVALID_ARGUMENT, "d_present is NULL");
    RT_TRY(check_image_size(rows, cols));
    if (d_pixels && capacity == 0) return fail(RT_ERR_INVALID_ARGUMENT, "d_pixels is given but capacity is 0");
    return RT_OK;
}
static int check_scatter(size_t n, const void *d_pixels, const void *d_rgb_list, int32_t rows, int32_t cols, const void *d_rgb_frame) {
    if (n > 0 && !d_pixels) return fail(RT_ERR_INVALID_ARGUMENT, "d_pixels is NULL");
    if (n > 0 && !d_rgb_list) return fail(RT_ERR_INVALID_ARGUMENT, "d_rgb_list is NULL");
    RT_TRY(check_count(n, "list entries"));
    RT_TRY(check_image_size(rows, cols));
    if (!d_rgb_frame) return fail(RT_ERR_INVALID_ARGUMENT, "d_rgb_frame is NULL");
    return RT_OK;
}
static unsigned grid_for(size_t items) { // grid-stride kernels of RPM_BLOCK threads
    const size_t want = (items + RPM_BLOCK - 1u) / RPM_BLOCK;
    return (unsigned) (want < 1u ? 1u : want < 4096u ? want : 4096u);
}

// Enqueues one parse on `st` (arguments checked, the device current).  Scratch: the head and one winner word per pixel (zeroed), then one
// rpm::Entry and one rpm::Map per tile.  An empty map: present cleared, the count 0, no scratch.  Never waits for the device.
static int enqueue_parse(const void *d_data, size_t n_bytes, int32_t rows, int32_t cols, void *d_rgb, void *d_present, void *d_count, hipStream_t st,
                         FormatPending &fp) {
    const uint32_t npx = (uint32_t) ((uint64_t) rows * (uint64_t) cols), n = (uint32_t) n_bytes;
    if (n == 0u) {
        HIP_TRY(hipMemsetAsync(d_present, 0, npx, st));
        if (d_count) HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(long long), st));
        return RT_OK;
    }
    const uint32_t n_tiles = (n + (uint32_t) RPM_TILE_BYTES - 1u) / (uint32_t) RPM_TILE_BYTES;
    const size_t zeroed = RPM_HEAD_BYTES + (size_t) npx * sizeof(unsigned int), entries_at = (zeroed + 7u) & ~(size_t) 7u,
                 maps_at = entries_at + (size_t) n_tiles * sizeof(rpm::Entry);
    HIP_TRY(hipMallocAsync((void **) &fp.scr, maps_at + (size_t) n_tiles * sizeof(rpm::Map), st));
    fp.st = st;
    HIP_TRY(hipMemsetAsync(fp.scr, 0, zeroed, st));
    rpm::ParseHead *head = (rpm::ParseHead *) fp.scr;
    unsigned int *winner = (unsigned int *) (fp.scr + RPM_HEAD_BYTES);
    rpm::Entry *entries = (rpm::Entry *) (fp.scr + entries_at);
    rpm::Map *maps = (rpm::Map *) (fp.scr + maps_at);
    const uint8_t *data = (const uint8_t *) d_data;
    hipLaunchKernelGGL(rpm::parse_maps_kernel, dim3(n_tiles), dim3(RPM_BLOCK), 0, st, data, n, maps);
    hipLaunchKernelGGL(rpm::parse_scan_kernel, dim3(1), dim3(RPM_SCAN_THREADS), 0, st, (const rpm::Map *) maps, n_tiles, entries, head);
    hipLaunchKernelGGL(rpm::parse_records_kernel<false>, dim3(n_tiles), dim3(RPM_BLOCK), 0, st, data, n, (uint32_t) rows, (uint32_t) cols, (const rpm::Entry *) entries, head,
                       winner, (uint8_t *) d_rgb);
    hipLaunchKernelGGL(rpm::parse_records_kernel<true>, dim3(n_tiles), dim3(RPM_BLOCK), 0, st, data, n, (uint32_t) rows, (uint32_t) cols, (const rpm::Entry *) entries, head,
                       winner, (uint8_t *) d_rgb);
    hipLaunchKernelGGL(rpm::parse_finish_kernel, dim3(grid_for(npx)), dim3(RPM_BLOCK), 0, st, (const rpm::ParseHead *) head, (const unsigned int *) winner, npx,
                       (uint8_t *) d_present, (long long *) d_count, (long long) -RT_ERR_INVALID_ARGUMENT);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
// Waits for the stream and reads what the device found: the count, or a malformed map (of which it wrote nothing).
static int finish_parse(FormatPending &fp, hipStream_t st, int64_t *count) {
    rpm::ParseHead head{};
    if (fp.scr) HIP_TRY(hipMemcpyAsync(&head, fp.scr, sizeof(head), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (head.bad) return fail(RT_ERR_INVALID_ARGUMENT, kMalformedMap);
    *count = (int64_t) head.count;
    return RT_OK;
}

// Enqueues one list of absent pixels on `st`: rt_output.h's three steps over presence bytes (scratch: rto::FormatScratch and one uint64 per tile).
static int enqueue_missing(const void *d_present, int32_t rows, int32_t cols, void *d_pixels, size_t capacity, void *d_n, hipStream_t st, FormatPending &fp) {
    const uint32_t npx = (uint32_t) ((uint64_t) rows * (uint64_t) cols), n_tiles = (npx + (uint32_t) RPM_TILE_BYTES - 1u) / (uint32_t) RPM_TILE_BYTES;
    HIP_TRY(hipMallocAsync((void **) &fp.scr, RTO_SCRATCH_HEAD + (size_t) n_tiles * sizeof(unsigned long long), st));
    fp.st = st;
    rto::FormatScratch *head = (rto::FormatScratch *) fp.scr;
    unsigned long long *tiles = (unsigned long long *) (fp.scr + RTO_SCRATCH_HEAD);
    hipLaunchKernelGGL(rpm::missing_sums_kernel, dim3(n_tiles), dim3(RPM_BLOCK), 0, st, (const uint8_t *) d_present, npx, tiles);
    hipLaunchKernelGGL(rto::format_scan_kernel, dim3(1), dim3(RTO_SCAN_THREADS), 0, st, tiles, n_tiles, 0ull, head, (long long *) d_n, (unsigned long long) capacity,
                       d_pixels ? 1 : 0);
    if (d_pixels)
        hipLaunchKernelGGL(rpm::missing_scatter_kernel, dim3(n_tiles), dim3(RPM_BLOCK), 0, st, (const uint8_t *) d_present, npx, (const unsigned long long *) tiles,
                           (const rto::FormatScratch *) head, (int32_t *) d_pixels);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
static int finish_missing(FormatPending &fp, const void *d_pixels, size_t capacity, int64_t *n) {
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, fp.scr + offsetof(rto::FormatScratch, total), sizeof(total), hipMemcpyDeviceToHost, fp.st));
    HIP_TRY(hipStreamSynchronize(fp.st));
    *n = (int64_t) total;
    if (d_pixels && (unsigned long long) total > (unsigned long long) capacity)
        return fail(RT_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " below the " + std::to_string(total) + " entries needed");
    return RT_OK;
}

// Enqueues one scatter on `st` (n > 0).  Scratch: the head and one winner word per pixel of the frame, zeroed.
static int enqueue_scatter(size_t n, const void *d_pixels, const void *d_rgb_list, int32_t rows, int32_t cols, void *d_rgb_frame, hipStream_t st, FormatPending &fp) {
    const uint32_t npx = (uint32_t) ((uint64_t) rows * (uint64_t) cols);
    const size_t bytes = RPM_HEAD_BYTES + (size_t) npx * sizeof(unsigned int);
    HIP_TRY(hipMallocAsync((void **) &fp.scr, bytes, st));
    fp.st = st;
    HIP_TRY(hipMemsetAsync(fp.scr, 0, bytes, st));
    rpm::ParseHead *head = (rpm::ParseHead *) fp.scr;
    unsigned int *winner = (unsigned int *) (fp.scr + RPM_HEAD_BYTES);
    hipLaunchKernelGGL(rpm::scatter_claim_kernel, dim3(grid_for(n)), dim3(RPM_BLOCK), 0, st, (uint32_t) n, (const int32_t *) d_pixels, npx, head, winner);
    hipLaunchKernelGGL(rpm::scatter_store_kernel, dim3(grid_for(n)), dim3(RPM_BLOCK), 0, st, (uint32_t) n, (const int32_t *) d_pixels, (const uint8_t *) d_rgb_list,
                       (const rpm::ParseHead *) head, (const unsigned int *) winner, (uint8_t *) d_rgb_frame);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// rt_resume_*'s checks: rt_render's list about scene, camera, geometry and options, then the map's bytes and the frame a pixel list can index
static int check_resume(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, const void *data, size_t n_bytes,
                        const rt_render_options *options, int32_t &rows, int32_t &cols) {
    rows = (max_h > 0 && max_h <= (1 << 20)) ? 2 * max_h + 1 : 0;
    cols = (max_w > 0 && max_w <= (1 << 20)) ? 2 * max_w + 1 : 0;
    RT_TRY(check_frame(scene, camera, max_w, max_h, 0, 1, rows, scene, "", options)); // (the buffers are this call's own)
    RT_TRY(check_map_bytes(data, n_bytes));
    RT_TRY(check_list_frame(max_w, max_h));
    return RT_OK;
}

// The resumed frame on the device (the device current, arguments checked; everything on the null stream; waits for it): the map's bytes
// uploaded and parsed into `frame` (rows*cols*3, from the null stream's pool), the absent pixels listed, rendered as a pixel list and
// scattered into it.  `local` as a pixel-list render fills it; all zero when the map is complete.
static int resume_on_device(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, uint32_t flags,
                            const uint8_t *data, size_t n_bytes, int32_t rows, int32_t cols, const rt_render_options *options, StreamBuf &frame, rt_stats &local) {
    const size_t npx = (size_t) rows * (size_t) cols, present_at = (npx * 3u + 15u) & ~(size_t) 15u, pixels_at = present_at + ((npx + 15u) & ~(size_t) 15u),
                 map_at = pixels_at + npx * 4u;
    HIP_TRY(hipMallocAsync((void **) &frame.p, map_at + n_bytes, frame.st));
    if (n_bytes) HIP_TRY(hipMemcpyAsync(frame.p + map_at, data, n_bytes, hipMemcpyHostToDevice, frame.st));
    int64_t count = 0, missing = 0;
    {
        FormatPending fp;
        RT_TRY(enqueue_parse(frame.p + map_at, n_bytes, rows, cols, frame.p, frame.p + present_at, nullptr, frame.st, fp));
        RT_TRY(finish_parse(fp, frame.st, &count)); // a malformed map: before anything is rendered
    }
    {
        FormatPending fp;
        RT_TRY(enqueue_missing(frame.p + present_at, rows, cols, frame.p + pixels_at, npx, nullptr, frame.st, fp));
        RT_TRY(finish_missing(fp, frame.p + pixels_at, npx, &missing));
    }
    memset(&local, 0, sizeof(local));
    if (missing == 0) return RT_OK;
    const size_t n = (size_t) missing, list_at = n * 16u;
    StreamBuf out; // accum [n][4] int32, then rgb [n][3]
    HIP_TRY(hipMallocAsync((void **) &out.p, list_at + n * 3u, out.st));
    {
        Pending pd;
        RT_TRY(launch_pixels(scene, camera, max_w, max_h, seed, device, n, frame.p + pixels_at, flags, out.p, out.p + list_at, nullptr, options, true, pd));
        RT_TRY(collect_stats(pd, &local));
    }
    FormatPending fp;
    RT_TRY(enqueue_scatter(n, frame.p + pixels_at, out.p + list_at, rows, cols, frame.p, frame.st, fp));
    HIP_TRY(hipStreamSynchronize(frame.st));
    return RT_OK;
}

// rt_resume_ppm / rt_resume_png
static int resume_file(const char *name, int fmt, const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device,
                       uint32_t flags, const char *map_path, int32_t gamma_correct, const char *out_path, const rt_render_options *options, rt_stats *stats) {
    int32_t rows = 0, cols = 0;
    RT_TRY(check_resume(scene, camera, max_w, max_h, nullptr, 0, options, rows, cols));
    if (!map_path) return fail(RT_ERR_INVALID_ARGUMENT, "map_path is NULL");
    if (!out_path) return fail(RT_ERR_INVALID_ARGUMENT, "out_path is NULL");
    if (fmt == rto::FMT_PNG) RT_TRY(check_png_size(rows, cols));
    return guarded(name, [&]() {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint8_t> map; // the spill is read whole before the output is opened: the two paths may name one file
        {
            FileCloser in;
            if (!(in.f = fopen(map_path, "rb"))) return fail(RT_ERR_IO, std::string("cannot open ") + map_path);
            unsigned char block[1 << 16];
            for (size_t got; (got = fread(block, 1, sizeof(block), in.f)) > 0;) {
                map.insert(map.end(), block, block + got);
                if (map.size() > (size_t) INT32_MAX) return check_map_size(map.size());
            }
            if (ferror(in.f)) return fail(RT_ERR_IO, std::string("cannot read ") + map_path);
        }
        FileCloser file;
        if (!(file.f = fopen(out_path, "wb"))) return fail(RT_ERR_IO, std::string("cannot open ") + out_path);
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        StreamBuf frame;
        rt_stats local;
        RT_TRY(resume_on_device(scene, camera, max_w, max_h, seed, device, flags, map.data(), map.size(), rows, cols, options, frame, local));
        const size_t capacity = (size_t) file_max_bytes(fmt, rows, cols);
        StreamBuf d_text;
        HIP_TRY(hipMallocAsync((void **) &d_text.p, capacity, d_text.st));
        std::unique_ptr<char[]> text;
        int64_t len = 0;
        RT_TRY(file_to_host(fmt, frame.p, rows, cols, gamma_correct != 0, d_text.st, d_text.p, capacity, text, len));
        RT_TRY(write_all(file, out_path, text.get(), len));
        if (stats) {
            *stats = local;
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return (int) RT_OK;
    });
}

extern "C" {

int32_t rt_pixel_map_chunk_bytes(void) { return RPM_CHUNK_BYTES; }
int32_t rt_pixel_map_tile_bytes(void) { return RPM_TILE_BYTES; }
int32_t rt_pixel_map_scan_tiles(void) { return RPM_SCAN_THREADS; }

int rt_parse_pixel_map_device(int32_t device, const void *d_data, size_t n_bytes, int32_t rows, int32_t cols, void *d_rgb, void *d_present, void *d_count,
                              void *stream, int64_t *count) {
    RT_TRY(check_parse(d_data, n_bytes, rows, cols, d_rgb, d_present));
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    FormatPending fp;
    RT_TRY(enqueue_parse(d_data, n_bytes, rows, cols, d_rgb, d_present, d_count, (hipStream_t) stream, fp));
    return count ? finish_parse(fp, (hipStream_t) stream, count) : RT_OK;
}

int rt_missing_pixels_device(int32_t device, const void *d_present, int32_t rows, int32_t cols, void *d_pixels, size_t capacity, void *d_n, void *stream,
                             int64_t *n) {
    RT_TRY(check_missing(d_present, rows, cols, d_pixels, capacity));
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    FormatPending fp;
    RT_TRY(enqueue_missing(d_present, rows, cols, d_pixels, capacity, d_n, (hipStream_t) stream, fp));
    return n ? finish_missing(fp, d_pixels, capacity, n) : RT_OK;
}

int rt_scatter_pixels_device(int32_t device, size_t n, const void *d_pixels, const void *d_rgb_list, int32_t rows, int32_t cols, void *d_rgb_frame, void *stream) {
    RT_TRY(check_scatter(n, d_pixels, d_rgb_list, rows, cols, d_rgb_frame));
    if (n == 0) return RT_OK;
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    FormatPending fp;
    return enqueue_scatter(n, d_pixels, d_rgb_list, rows, cols, d_rgb_frame, (hipStream_t) stream, fp);
}

int rt_resume_pixel_map(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, uint32_t flags,
                        const uint8_t *data, size_t n_bytes, uint8_t *rgb_out, const rt_render_options *options, rt_stats *stats) {
    int32_t rows = 0, cols = 0;
    RT_TRY(check_resume(scene, camera, max_w, max_h, data, n_bytes, options, rows, cols));
    if (!rgb_out) return fail(RT_ERR_INVALID_ARGUMENT, "rgb_out is NULL");
    RT_TRY(check_map_size(n_bytes));
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    StreamBuf frame;
    rt_stats local;
    RT_TRY(resume_on_device(scene, camera, max_w, max_h, seed, device, flags, data, n_bytes, rows, cols, options, frame, local));
    HIP_TRY(hipMemcpy(rgb_out, frame.p, (size_t) rows * (size_t) cols * 3u, hipMemcpyDeviceToHost));
    if (stats) {
        *stats = local;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

int rt_resume_ppm(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, uint32_t flags,
                  const char *map_path, int32_t gamma_correct, const char *out_path, const rt_render_options *options, rt_stats *stats) {
    return resume_file("rt_resume_ppm", rto::FMT_PPM, scene, camera, max_w, max_h, seed, device, flags, map_path, gamma_correct, out_path, options, stats);
}
int rt_resume_png(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, uint32_t flags,
                  const char *map_path, int32_t gamma_correct, const char *out_path, const rt_render_options *options, rt_stats *stats) {
    return resume_file("rt_resume_png", rto::FMT_PNG, scene, camera, max_w, max_h, seed, device, flags, map_path, gamma_correct, out_path, options, stats);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// render jobs (DESIGN.md "Render jobs"; rt_job_plan.h, rt_render_kernel.h's JobCtl and finishing kernels, rt_job_kernels.h): a frame
// shard's render launched and left running, with progress the host reads, a stop word the kernels poll, and a partial frame whose
// present set rt_job_plan.h defines
// ------------------------------------------------------------------------------------------------------------
namespace {

// The job's control block: pinned, mapped, coherent host memory (hipHostMalloc).  The device polls `stop`, mirrors its count of final
// pixels to `progress`, and the finishing kernels leave the result and, last of all, `finished`.
struct JobControl {
    uint32_t stop, finished;
    unsigned long long progress;
    JobResult res;
};
// The job's device words, between the launch's scratch and its workspace
struct JobWords {
    unsigned long long done;     // JobCtl::done
    unsigned long long seal[3];  // done_a, done_b, n_present (job_seal_kernel .. job_result_kernel)
};
enum { JOB_WORDS_BYTES = 64 };
static_assert(sizeof(JobWords) <= JOB_WORDS_BYTES, "the job's words fit their slot");

typedef void (*job_fn)(const RenderParams, const JobCtl);
template <int BLOCK, int PASS, bool TEX> job_fn pick_job_lds(bool lds) { return lds ? render_job_kernel<true, BLOCK, PASS, TEX> : render_job_kernel<false, BLOCK, PASS, TEX>; }
template <int PASS> job_fn pick_job_pass(const rtp::Pass &q) {
    if (q.prog) {
        if (q.block == 256) return q.lds ? render_prog_job_kernel<true, 256, PASS> : render_prog_job_kernel<false, 256, PASS>;
        return q.lds ? render_prog_job_kernel<true, 1024, PASS> : render_prog_job_kernel<false, 1024, PASS>;
    }
    if (q.block == 256) return q.tex ? pick_job_lds<256, PASS, true>(q.lds) : pick_job_lds<256, PASS, false>(q.lds);
    return q.tex ? pick_job_lds<1024, PASS, true>(q.lds) : pick_job_lds<1024, PASS, false>(q.lds);
}
job_fn pick_job_kernel(const rtp::Pass &q) { // the frame passes at blocks of 256 and 1024; anything else is not built
    if (q.count || (q.block != 256 && q.block != 1024)) return nullptr;
    return q.mode == rtmode::FRAME_FUSED ? pick_job_pass<rtmode::FRAME_FUSED>(q) : q.mode == rtmode::FRAME_PASS_A ? pick_job_pass<rtmode::FRAME_PASS_A>(q) :
           q.mode == rtmode::FRAME_PASS_B ? pick_job_pass<rtmode::FRAME_PASS_B>(q) : nullptr;
}

thread_local int64_t g_job_limits[2] = {-1, -1};
thread_local int64_t g_last_job_plan[8] = {0};

} // namespace

struct rt_render_job {
    JobControl *ctl = nullptr;
    int device = -1;
    hipStream_t st = nullptr;
    Pending pd;
    // what rt_render_job_finish renders with
    const rt_scene *scene = nullptr;
    rt_camera camera{};
    int32_t max_w = 0, max_h = 0, row_first = 0, row_stride = 1, n_rows = 0;
    uint64_t seed = 0;
    uint32_t flags = 0;
    bool has_options = false;
    rt_render_options options{};
    void *d_accum = nullptr, *d_rgb = nullptr, *d_present = nullptr;
    int64_t pixels_total = 0;
    int64_t plan[8] = {0}; // rt_dev_last_job_plan's words (done_a, done_b and n_list after the wait)
    mutable std::atomic<long long> seen{0}; // the most the progress mirror has shown (racing device stores may regress it)
    std::mutex mu;          // wait / finish / destroy
    bool launched = false, waited = false;
    rt_job_result result{};
    rt_stats stats{};
};

// Plans and enqueues the job on job->st (arguments checked, the device current): enqueue()'s sequence for a fresh frame shard with the
// stoppable kernels, then the finishing kernels, all up front.  The plan is plan_launch's for the same arguments, but for the block:
// the job kernels are built for 256 and 1024 threads, and a request for 512 or 768 runs at 1024 (as the list modes do).
static int enqueue_job(rt_render_job *j, const int64_t limits[2]) {
    const auto t0 = std::chrono::steady_clock::now();
    DeviceScene *ds = nullptr;
    RT_TRY(device_scene(const_cast<rt_scene *>(j->scene), j->device, &ds));
    const rth::HostScene &h = j->scene->host;
    hipStream_t st = j->st;
    RenderParams p{};
    p.max_w = j->max_w; p.max_h = j->max_h;
    p.spp = j->camera.samples_per_pixel;
    p.depth = j->camera.bounce_depth;
    p.seed_key = mix64(j->seed + 0x9E3779B97F4A7C15ull); // seed_key(), host side
    p.cols = 2 * j->max_w + 1;
    p.row_first = j->row_first; p.row_stride = j->row_stride; p.n_rows = j->n_rows;
    p.accum = (int32_t *) j->d_accum;
    p.rgb = (uint8_t *) j->d_rgb;
    p.off = h.off;
    p.scene_image = ds->image;
    p.tex = ds->tex;
    p.texels = ds->texels;
    p.obj_to_orig = ds->obj_to_orig;
    rtp::Job job;
    job.kind = rtp::Job::FRAME;
    job.n_rows = (uint64_t) j->n_rows; job.max_w = j->max_w; job.spp = j->camera.samples_per_pixel;
    Settings set = resolve_settings(j->has_options ? &j->options : nullptr);
    if (set.block != 0 && set.block != 256) set.block = 1024;

    rtp::LaunchPlan plan = rtp::plan_begin(scene_size(h), set, false, job, ds->cu_count);
    const int block = plan.one.block;
    job_fn fn = pick_job_kernel(plan.one);
    if (!fn) return fail(RT_ERR_HIP, "no job kernel is built for this launch");
    RT_TRY(allow_full_lds((const void *) fn));
    int perCu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, (const void *) fn, block, plan.one.lds_bytes));
    if (perCu < 1) return fail(RT_ERR_HIP, "render job kernel does not fit on a CU (occupancy 0)");
    rtp::plan_finish(plan, perCu);
    if (plan.error) return fail(RT_ERR_HIP, plan.error);
    const size_t pairsBytes = plan.pairs_bytes, listBytes = plan.list_bytes, sortBytes = plan.sort_bytes, poolBytes = plan.pool_bytes;
    job_fn fa = nullptr, fb = nullptr;
    if (plan.two_pass) {
        fa = pick_job_kernel(plan.a); fb = pick_job_kernel(plan.b);
        if (!fa || !fb) return fail(RT_ERR_HIP, "no job kernel is built for this launch");
        RT_TRY(allow_full_lds((const void *) fa));
        RT_TRY(allow_full_lds((const void *) fb));
    }
    const rtjob::Plan jp{plan.two_pass ? 2 : 1, (uint32_t) (plan.two_pass ? plan.a.chunk : plan.one.chunk), (uint64_t) plan.pixels};
    int64_t *w = j->plan;
    w[0] = jp.passes; w[1] = jp.chunk; w[2] = (int64_t) rtjob::units_of(jp); w[3] = 0; w[4] = 0; w[5] = 0; w[6] = block; w[7] = plan.one.tex ? 1 : 0;

    Pending &cl = j->pd;
    unsigned char *scr = nullptr;
    HIP_TRY(hipMallocAsync((void **) &scr, RT_SCRATCH_BYTES + JOB_WORDS_BYTES + pairsBytes + listBytes + sortBytes + poolBytes, st));
    cl.scr = scr; cl.st = st; cl.device = j->device; cl.t0 = t0;
    cl.pixels = plan.pixels; cl.waves = plan.waves;
    HIP_TRY(hipEventCreate(&cl.a));
    HIP_TRY(hipEventCreate(&cl.b));
    LaunchScratch *ls = (LaunchScratch *) scr;
    JobWords *jw = (JobWords *) (scr + RT_SCRATCH_BYTES);
    unsigned char *ws = scr + RT_SCRATCH_BYTES + JOB_WORDS_BYTES;
    p.counters = ls->counters;
    p.queue = &ls->queue;
    p.queue_b = &ls->queue_b;
    p.live_count = &ls->live_count;
    p.cam_ptr = &ls->cam;
    p.park_pool = ws + pairsBytes + listBytes + sortBytes;
    hipLaunchKernelGGL(launch_init_kernel, dim3(1), dim3(64), 0, st, scr, camera_params(&j->camera, j->max_w, j->max_h));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(jw, 0, JOB_WORDS_BYTES, st));
    JobControl *dctl = nullptr; // the control block as the device addresses it
    HIP_TRY(hipHostGetDevicePointer((void **) &dctl, j->ctl, 0));
    JobCtl ctl{};
    ctl.stop = &dctl->stop; ctl.progress = &dctl->progress; ctl.done = &jw->done;
    HIP_TRY(hipEventRecord(cl.a, st));
    if (!plan.two_pass) {
        set_plan_fields(p, plan.one);
        ctl.limit = limits[0];
        hipLaunchKernelGGL(fn, dim3((unsigned) plan.one.grid), dim3((unsigned) block), plan.one.lds_bytes, st, p, ctl);
        HIP_TRY(hipGetLastError());
    } else {
        unsigned int *sortBuf = (unsigned int *) (ws + pairsBytes + listBytes);
        HIP_TRY(hipMemsetAsync(sortBuf, 0, sortBytes, st));
        p.pairs = (unsigned long long *) ws;
        p.live_list = (const unsigned int *) (ws + pairsBytes);
        RenderParams pa = p;
        set_plan_fields(pa, plan.a);
        set_plan_fields(p, plan.b);
        const uint32_t n1 = (uint32_t) (2 * p.k + 1);
        JobCtl ca = ctl, cb = ctl;
        ca.limit = limits[0]; cb.limit = limits[1];
        hipLaunchKernelGGL(fa, dim3((unsigned) plan.a.grid), dim3((unsigned) block), plan.a.lds_bytes, st, pa, ca);
        hipLaunchKernelGGL(sort_hist_kernel, dim3(256), dim3(256), 0, st, (const unsigned long long *) p.pairs, (const unsigned int *) p.live_count, n1, sortBuf);
        hipLaunchKernelGGL(sort_offsets_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) sortBuf, sortBuf + RTD_COST_BUCKETS);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(256), dim3(256), 0, st, (const unsigned long long *) p.pairs, (const unsigned int *) p.live_count, n1,
                           (const unsigned int *) (sortBuf + RTD_COST_BUCKETS), sortBuf + 2 * RTD_COST_BUCKETS, (unsigned int *) (ws + pairsBytes));
        hipLaunchKernelGGL(fb, dim3((unsigned) plan.b.grid), dim3((unsigned) block), plan.b.lds_bytes, st, p, cb);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("two-pass job launch: ") + hipGetErrorString(e));
    }
    // the finishing kernels: the present set (rt_job_plan.h), absent pixels zeroed, the count, the result -- before the scratch is released
    const unsigned long long nLocal = plan.pixels;
    const unsigned long long want = (nLocal + 255ull) / 256ull, most = (unsigned long long) ds->cu_count * 8ull;
    const unsigned fgrid = (unsigned) (want < most ? want : most);
    hipLaunchKernelGGL(job_seal_kernel, dim3(1), dim3(64), 0, st, (const unsigned int *) p.queue, (const unsigned long long *) p.queue_b, (const unsigned int *) p.live_count, jp,
                       (long long) limits[0], (long long) limits[1], jw->seal, &dctl->res);
    hipLaunchKernelGGL(job_units_kernel, dim3(fgrid), dim3(256), 0, st, jp, (const unsigned long long *) jw->seal, (uint8_t *) j->d_present);
    if (plan.two_pass)
        hipLaunchKernelGGL(job_pending_kernel, dim3(fgrid), dim3(256), 0, st, p.live_list, (const unsigned int *) p.live_count, (const unsigned long long *) jw->seal,
                           (uint8_t *) j->d_present);
    hipLaunchKernelGGL(job_zero_kernel, dim3(fgrid), dim3(256), 0, st, nLocal, (const uint8_t *) j->d_present, p.accum, p.rgb, jw->seal);
    hipLaunchKernelGGL(job_result_kernel, dim3(1), dim3(64), 0, st, nLocal, (const unsigned long long *) jw->seal, (const unsigned long long *) p.counters, &dctl->res,
                       &dctl->progress, &dctl->finished);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(cl.b, st));
    cl.launched = true;
    j->launched = true;
    return RT_OK;
}

static void job_free(rt_render_job *j) { // (the device current, the stream idle)
    j->pd.release();
    if (j->ctl) (void) hipHostFree(j->ctl);
    delete j;
}

extern "C" {

int rt_dev_set_job_limits(int64_t limit_a, int64_t limit_b) {
    if (limit_a < -1 || limit_b < -1) return fail(RT_ERR_INVALID_ARGUMENT, "a job limit is -1 (none) or a count >= 0");
    g_job_limits[0] = limit_a; g_job_limits[1] = limit_b;
    return RT_OK;
}

int rt_dev_last_job_plan(int64_t out[8]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = g_last_job_plan[i];
    return RT_OK;
}

int rt_render_job_start(const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, uint64_t seed, int32_t device, int32_t row_first,
                        int32_t row_stride, int32_t n_rows, uint32_t flags, void *d_accum, void *d_rgb, void *d_present, void *stream,
                        const rt_render_options *options, rt_render_job **out) {
    RT_TRY(check_frame(scene, camera, max_w, max_h, row_first, row_stride, n_rows, d_accum, "d_accum is NULL", options));
    if (n_rows > 0 && !d_present) return fail(RT_ERR_INVALID_ARGUMENT, "d_present is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    RT_TRY(check_list_frame(max_w, max_h));
    if (flags & RT_RENDER_COUNTERS) return fail(RT_ERR_UNSUPPORTED, "a render job has no counting variant (RT_RENDER_COUNTERS)");
    return guarded("rt_render_job_start", [&]() {
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        const int64_t limits[2] = {g_job_limits[0], g_job_limits[1]}; // consumed by this job
        g_job_limits[0] = g_job_limits[1] = -1;
        rt_render_job *j = new rt_render_job();
        j->device = device; j->st = (hipStream_t) stream;
        j->scene = scene; j->camera = *camera;
        j->max_w = max_w; j->max_h = max_h; j->row_first = row_first; j->row_stride = row_stride; j->n_rows = n_rows;
        j->seed = seed; j->flags = flags;
        if (options) { // (only the bytes the caller's struct has)
            j->has_options = true;
            memcpy(&j->options, options, options->struct_size < sizeof(rt_render_options) ? options->struct_size : sizeof(rt_render_options));
        }
        j->d_accum = d_accum; j->d_rgb = d_rgb; j->d_present = d_present;
        j->pixels_total = (int64_t) n_rows * (int64_t) (2 * max_w + 1);
        hipError_t e = hipHostMalloc((void **) &j->ctl, sizeof(JobControl), hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) { j->ctl = nullptr; job_free(j); return fail(RT_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
        memset(j->ctl, 0, sizeof(JobControl));
        int rc = RT_OK;
        if (j->pixels_total == 0) { // an empty shard: nothing to launch, complete at once
            j->ctl->res.complete = 1;
            j->ctl->finished = 1u;
        } else rc = enqueue_job(j, limits);
        if (rc != RT_OK) { // whatever was launched polls the control block: wait for it before the block goes
            (void) hipStreamSynchronize(j->st);
            job_free(j);
            return rc;
        }
        for (int i = 0; i < 8; ++i) g_last_job_plan[i] = j->plan[i]; // (done_a, done_b and n_list: after the wait)
        *out = j;
        return (int) RT_OK;
    });
}

int rt_render_job_progress(const rt_render_job *job, rt_job_progress *progress) {
    if (!job) return fail(RT_ERR_INVALID_ARGUMENT, "job is NULL");
    if (!progress || progress->struct_size < sizeof(rt_job_progress)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_job_progress.struct_size is not set");
    const uint32_t finished = __atomic_load_n(&job->ctl->finished, __ATOMIC_ACQUIRE), stop = __atomic_load_n(&job->ctl->stop, __ATOMIC_RELAXED);
    long long now = (long long) __atomic_load_n(&job->ctl->progress, __ATOMIC_RELAXED);
    if (now > (long long) job->pixels_total) now = (long long) job->pixels_total;
    long long best = job->seen.load(std::memory_order_relaxed);
    while (now > best && !job->seen.compare_exchange_weak(best, now, std::memory_order_relaxed)) {}
    progress->state = finished ? 2 : (stop ? 1 : 0);
    progress->pixels_total = job->pixels_total;
    progress->pixels_final = now > best ? now : best;
    return RT_OK;
}

int rt_render_job_stop(rt_render_job *job) {
    if (!job) return fail(RT_ERR_INVALID_ARGUMENT, "job is NULL");
    __atomic_store_n(&job->ctl->stop, 1u, __ATOMIC_RELAXED);
    return RT_OK;
}

int rt_render_job_wait(rt_render_job *job, rt_job_result *result, rt_stats *stats) {
    if (!job) return fail(RT_ERR_INVALID_ARGUMENT, "job is NULL");
    if (result && result->struct_size < sizeof(rt_job_result)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_job_result.struct_size is not set");
    std::lock_guard<std::mutex> lock(job->mu);
    if (!job->waited) {
        DeviceGuard guard;
        RT_TRY(guard.enter(job->device));
        HIP_TRY(hipStreamSynchronize(job->st));
        const JobResult r = job->ctl->res;
        float ms = 0.f;
        if (job->launched) HIP_TRY(hipEventElapsedTime(&ms, job->pd.a, job->pd.b));
        memset(&job->stats, 0, sizeof(job->stats));
        job->stats.pixels = (uint64_t) r.n_present;
        job->stats.samples = r.samples;
        job->stats.kernel_ms = ms;
        job->stats.total_ms = job->launched ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - job->pd.t0).count() : 0.0;
        job->result.struct_size = (uint32_t) sizeof(rt_job_result);
        job->result.complete = (int32_t) r.complete;
        job->result.stop_requested = __atomic_load_n(&job->ctl->stop, __ATOMIC_RELAXED) ? 1 : 0;
        job->result.pixels_total = job->pixels_total;
        job->result.n_present = r.n_present;
        job->plan[3] = r.n_list; job->plan[4] = r.done_a; job->plan[5] = r.done_b;
        job->seen.store((long long) r.n_present, std::memory_order_relaxed); // the exact count: no mirrored value exceeds it
        job->pd.release();
        job->waited = true;
    }
    for (int i = 0; i < 8; ++i) g_last_job_plan[i] = job->plan[i];
    if (result) { const uint32_t size = result->struct_size; *result = job->result; result->struct_size = size; }
    if (stats) *stats = job->stats;
    return RT_OK;
}

int rt_render_job_finish(rt_render_job *job, void *stream, rt_stats *stats) {
    if (!job) return fail(RT_ERR_INVALID_ARGUMENT, "job is NULL");
    std::lock_guard<std::mutex> lock(job->mu);
    if (!job->waited) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_job_finish needs a preceding rt_render_job_wait");
    if (job->result.complete) return nothing_to_do(stats);
    DeviceGuard guard;
    RT_TRY(guard.enter(job->device));
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = (hipStream_t) stream;
    const int32_t cols = 2 * job->max_w + 1;
    const size_t npx = (size_t) job->pixels_total;
    StreamBuf lists; // the absent pixels as local indices [npx] int32, then as the frame's
    lists.st = st;
    HIP_TRY(hipMallocAsync((void **) &lists.p, npx * 8u, st));
    int64_t missing = 0;
    {
        FormatPending fp;
        RT_TRY(enqueue_missing(job->d_present, job->n_rows, cols, lists.p, npx, nullptr, st, fp));
        RT_TRY(finish_missing(fp, lists.p, npx, &missing));
    }
    rt_stats local;
    memset(&local, 0, sizeof(local));
    if (missing > 0) {
        const size_t n = (size_t) missing, rgb_at = n * 16u;
        const int32_t *d_local = (const int32_t *) lists.p;
        int32_t *d_global = (int32_t *) (lists.p + npx * 4u);
        StreamBuf outb; // accum [n][4] int32, then rgb [n][3]
        outb.st = st;
        HIP_TRY(hipMallocAsync((void **) &outb.p, rgb_at + n * 3u, st));
        const rtjob::Shard shard{cols, job->row_first, job->row_stride, job->n_rows};
        const unsigned g = grid_for(n);
        hipLaunchKernelGGL(job_global_list_kernel, dim3(g), dim3(256), 0, st, (unsigned long long) n, d_local, shard, d_global);
        HIP_TRY(hipGetLastError());
        {
            Pending pd;
            RT_TRY(launch_pixels(job->scene, &job->camera, job->max_w, job->max_h, job->seed, job->device, n, d_global, job->flags, outb.p,
                                 job->d_rgb ? outb.p + rgb_at : nullptr, stream, job->has_options ? &job->options : nullptr, true, pd));
            RT_TRY(collect_stats(pd, &local));
        }
        hipLaunchKernelGGL(job_scatter_kernel, dim3(g), dim3(256), 0, st, (unsigned long long) n, d_local, (const int32_t *) outb.p,
                           (const uint8_t *) (job->d_rgb ? outb.p + rgb_at : nullptr), (int32_t *) job->d_accum, (uint8_t *) job->d_rgb, (uint8_t *) job->d_present);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    job->result.complete = 1;
    job->result.n_present = job->pixels_total;
    job->seen.store((long long) job->pixels_total, std::memory_order_relaxed);
    __atomic_store_n(&job->ctl->progress, (unsigned long long) job->pixels_total, __ATOMIC_RELAXED);
    if (stats) {
        *stats = local;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return RT_OK;
}

void rt_render_job_destroy(rt_render_job *job) {
    if (!job) return;
    DeviceGuard guard;
    if (guard.enter(job->device) == RT_OK && !job->waited && job->launched) (void) hipStreamSynchronize(job->st); // the kernels poll the control block
    job_free(job);
}

int64_t rt_format_pixel_map_present(const uint8_t *rgb, const uint8_t *present, int32_t rows, int32_t cols, uint8_t *out, size_t out_capacity) {
    if (!rgb || !present || rows <= 0 || cols <= 0) { fail(RT_ERR_INVALID_ARGUMENT, "bad image"); return -RT_ERR_INVALID_ARGUMENT; }
    return guarded<int64_t>("rt_format_pixel_map_present", [&]() {
        std::string s = rth::format_pixel_map_present(rgb, present, rows, cols);
        if (out && out_capacity >= s.size()) memcpy(out, s.data(), s.size());
        return (int64_t) s.size();
    }, -RT_ERR_HOST);
}

int rt_format_pixel_map_present_device(int32_t device, const void *d_rgb, const void *d_present, int32_t rows, int32_t cols, void *d_out, size_t out_capacity,
                                       void *d_bytes, void *stream, int64_t *bytes) {
    if (!d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "d_rgb is NULL");
    if (!d_present) return fail(RT_ERR_INVALID_ARGUMENT, "d_present is NULL");
    RT_TRY(check_image_size(rows, cols));
    if (d_out && out_capacity == 0) return fail(RT_ERR_INVALID_ARGUMENT, "d_out is given but out_capacity is 0");
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    hipStream_t st = (hipStream_t) stream;
    const uint32_t npx = (uint32_t) ((uint64_t) rows * (uint64_t) cols);
    const uint32_t n_tiles = (npx + (uint32_t) RTO_TILE_PIXELS - 1u) / (uint32_t) RTO_TILE_PIXELS;
    FormatPending fp;
    HIP_TRY(hipMallocAsync((void **) &fp.scr, RTO_SCRATCH_HEAD + (size_t) n_tiles * sizeof(unsigned long long), st));
    fp.st = st;
    rto::FormatScratch *head = (rto::FormatScratch *) fp.scr;
    unsigned long long *tiles = (unsigned long long *) (fp.scr + RTO_SCRATCH_HEAD);
    hipLaunchKernelGGL(rtjob::present_sums_kernel, dim3(n_tiles), dim3(RTO_BLOCK), 0, st, (const unsigned char *) d_present, npx, (uint32_t) cols, tiles);
    hipLaunchKernelGGL(rto::format_scan_kernel, dim3(1), dim3(RTO_SCAN_THREADS), 0, st, tiles, n_tiles, 0ull, head, (long long *) d_bytes, (unsigned long long) out_capacity,
                       d_out ? 1 : 0);
    if (d_out)
        hipLaunchKernelGGL(rtjob::present_scatter_kernel, dim3(n_tiles), dim3(RTO_BLOCK), 0, st, (const unsigned char *) d_rgb, (const unsigned char *) d_present, npx,
                           (uint32_t) cols, (const unsigned long long *) tiles, (const rto::FormatScratch *) head, (unsigned char *) d_out);
    HIP_TRY(hipGetLastError());
    if (!bytes) return RT_OK;
    const FormatJob fj{rto::FMT_MAP, d_rgb, rows, cols, false, d_out, out_capacity, d_bytes};
    return finish_format(fp, fj, bytes);
}

} // extern "C"

// ============================================================================================================
// Device unit hooks: tiny kernels that call the SAME inlined device functions the render kernel uses.
// ============================================================================================================
namespace {

// A device buffer of a hook: `from` is uploaded before the launch, `to` downloaded after it (either may be null).
template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n;
    const T *from;
    T *to;
    DevBuf(size_t count, const T *from_, T *to_) : n(count), from(from_), to(to_) {}
    DevBuf(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void) hipFree(p); }
    hipError_t up() {
        if (!n) return hipSuccess;
        const hipError_t e = hipMalloc((void **) &p, n * sizeof(T));
        return e != hipSuccess || !from ? e : hipMemcpy(p, from, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t down() { return n && to ? hipMemcpy(to, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
};
template <typename T> static DevBuf<T> dev_in(const T *h, size_t n) { return DevBuf<T>(n, h, nullptr); }
template <typename T> static DevBuf<T> dev_out(T *h, size_t n) { return DevBuf<T>(n, nullptr, h); }
template <typename T> static DevBuf<T> dev_inout(T *h, size_t n) { return DevBuf<T>(n, h, h); }

__global__ void k_float_producer(Rng r, int n, double *out) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        for (int i = 0; i < n; ++i) out[i] = rng_get(r);
}
__global__ void k_stream_state(uint64_t seedKey, int n, const uint64_t *pixel, const uint32_t *sample, uint32_t *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng r = stream_for(pixel_key(seedKey, pixel[i]), sample[i]);
    out[i * 4] = r.x; out[i * 4 + 1] = r.y; out[i * 4 + 2] = r.z; out[i * 4 + 3] = r.w;
}
__global__ void k_bbox_hits(int n, const double *rays, const double *boxes, int32_t *hit) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = rays + i * 6, *b = boxes + i * 6;
    d2 bx, by, bz;
    bx.x = b[0]; bx.y = b[3]; by.x = b[1]; by.y = b[4]; bz.x = b[2]; bz.y = b[5];
    hit[i] = bbox_hits(1.0 / r[3], 1.0 / r[4], 1.0 / r[5], mk(r[0], r[1], r[2]), bx, by, bz) ? 1 : 0;
}
__global__ void k_sphere_isect(int n, const double *rays, const double *sph, double *t) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = rays + i * 6, *s = sph + i * 4;
    t[i] = sphere_first_intersection<true>(mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), mk(s[0], s[1], s[2]), s[3] * s[3]);
}
__global__ void k_plane_isect(int n, const double *rays, const double *pl, double *t) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = rays + i * 6, *p = pl + i * 6;
    t[i] = plane_intersection(mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), mk(p[0], p[1], p[2]), mk(p[3], p[4], p[5]));
}
RTD_INLINE uint32_t ld_rgb(const uint8_t *p) { return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16); }
RTD_INLINE void st_rgb(uint8_t *p, uint32_t c) { p[0] = (uint8_t) c; p[1] = (uint8_t) (c >> 8); p[2] = (uint8_t) (c >> 16); }
__global__ void k_pixel_combine(int n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st_rgb(out + i * 3, pix_combine(ld_rgb(a + i * 3), ld_rgb(b + i * 3)));
}
__global__ void k_pixel_darken(int n, const uint8_t *p, const double *albedo, uint8_t *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st_rgb(out + i * 3, pix_darken(albedo[i], ld_rgb(p + i * 3)));
}
__global__ void k_arith(int op, int n, const double *a, const double *b, double *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r;
    switch (op) {
    case 0: r = 1.0 / a[i]; break;
    case 1: r = sqrt(a[i]); break;
    case 2: r = rint(a[i]); break;
    case 3: r = a[i] / b[i]; break;
    case 4: r = pow5(a[i]); break;
    case 5: r = sqrt_above_tol(a[i]); break;
    case 6: r = inv_sqrt_above_tol(a[i]); break;
    case 7: r = rtt::cr_acos(a[i]); break;
    case 8: r = rtt::cr_sin(a[i]); break;
    default: r = rtt::cr_atan2(a[i], b[i]); break;
    }
    out[i] = r;
}

__global__ void k_reflection(const RenderParams p, int n, const int32_t *obj, const double *ray_in, const uint8_t *col_in,
                             const double *strike, uint32_t *rng, int32_t *absorbed, uint8_t *col_out, double *ray_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SceneView<false> sc = make_view<false>(p, nullptr);
    const double *r = ray_in + i * 6, *s = strike + i * 3;
    V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    uint32_t c = ld_rgb(col_in + i * 3);
    Rng g; g.x = rng[i * 4]; g.y = rng[i * 4 + 1]; g.z = rng[i * 4 + 2]; g.w = rng[i * 4 + 3];
    bool ab = reflection<false, 2>(sc, obj[i], mk(s[0], s[1], s[2]), o, d, c, g);
    absorbed[i] = ab ? 1 : 0;
    st_rgb(col_out + i * 3, c);
    double *ro = ray_out + i * 6;
    ro[0] = o.x; ro[1] = o.y; ro[2] = o.z; ro[3] = d.x; ro[4] = d.y; ro[5] = d.z;
    rng[i * 4] = g.x; rng[i * 4 + 1] = g.y; rng[i * 4 + 2] = g.z; rng[i * 4 + 3] = g.w;
}
__global__ void k_hit_object(const RenderParams p, int n, const double *rays, int32_t *hit, double *strike, uint32_t *counters) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SceneView<false> sc = make_view<false>(p, nullptr);
    const double *r = rays + i * 6;
    V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Counters cnt; cnt.rays = cnt.aabb = cnt.prim = cnt.refl = 0;
    double t;
    int obj = hit_object<false, true>(sc, o, d, t, cnt);
    hit[i] = obj;
    V3 sp = walk(o, d, t);
    if (strike) {
        const double nanv = __builtin_nan("");
        strike[i * 3] = obj < 0 ? nanv : sp.x; strike[i * 3 + 1] = obj < 0 ? nanv : sp.y; strike[i * 3 + 2] = obj < 0 ? nanv : sp.z;
    }
    if (counters) { counters[i * 2] = cnt.aabb; counters[i * 2 + 1] = cnt.prim; }
}
// Scene.hitObject as the render kernel's timed variant runs it: scene staged into LDS, the hand-written single-precision filter
// loop (node_loop_lds32), the leaf pass with the exact box and sphere tests between its runs, the unbounded objects last.  One ray
// per lane, 1024 rays per workgroup.
__global__ void __launch_bounds__(1024) k_hit_object_lds(const RenderParams p, int n, const double *rays, int32_t *hit, double *strike) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    (void) stage_scene<1024, true>(p, smem);
    const SceneView<true> sc = make_view<true, true>(p, smem);
    const int i = blockIdx.x * 1024 + threadIdx.x;
    const bool valid = i < n;
    const double *r = rays + (size_t) (valid ? i : 0) * 6;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    Walk w;
    walk_begin(w, sc.first);
    if (!valid) w.off = sc.end;
    const WalkCtx32 f = walk_ctx32(o, d, p.off.bmax);
    double bestF = __builtin_inf();
    // the claim that lets the leaf pass skip the exact box test needs unit directions: this hook's rays are arbitrary, so it holds
    // a lane to the claim only when its direction is one (|d|^2 within 1e-15 of 1, as Ray.make' leaves it)
    const double n2 = dot(d, d);
    const bool implied = p.off.box_implied != 0 && n2 >= 1.0 - 1e-15 && n2 <= 1.0 + 1e-15;
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
    Counters cnt; cnt.rays = cnt.aabb = cnt.prim = cnt.refl = 0;
    unbounded_tests<true, false>(sc, o, d, w, cnt);
    if (!valid) return;
    hit[i] = w.best;
    const V3 sp = walk(o, d, w.bestLen);
    const double nanv = __builtin_nan("");
    strike[i * 3] = w.best < 0 ? nanv : sp.x; strike[i * 3 + 1] = w.best < 0 ? nanv : sp.y; strike[i * 3 + 2] = w.best < 0 ? nanv : sp.z;
}
// pixel_candidates (rt_device.h) for n pixels of a camera: the Leaves a pixel's camera rays can reach, as the render kernel computes
// them once per pixel (scene staged into LDS exactly as the timed kernel stages it).  out[i*2], out[i*2+1] = the two queue words.
__global__ void __launch_bounds__(1024) k_pixel_candidates(const RenderParams p, const CameraParams cam, int n, const int32_t *rowcol, uint32_t *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    (void) stage_scene<1024, true>(p, smem);
    const SceneView<true> sc = make_view<true, true>(p, smem);
    const int i = blockIdx.x * 1024 + threadIdx.x;
    if (i >= n) return;
    uint32_t second = 0u;
    const uint32_t first = pixel_candidates<true, true>(sc, cam, rowcol[i * 2], rowcol[i * 2 + 1], second);
    out[i * 2] = first;
    out[i * 2 + 1] = second;
}
// The same for a scene that does not fit the LDS: the timed variant's global-memory view (make_view<false, true>), whose
// pixel_candidates reads every record from global memory (the hybrid LDS copy of the tree's top serves only the node loop)
__global__ void k_pixel_candidates_glb(const RenderParams p, const CameraParams cam, int n, const int32_t *rowcol, uint32_t *out) {
    const SceneView<false> sc = make_view<false, true>(p, nullptr);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t second = 0u;
    const uint32_t first = pixel_candidates<false, true>(sc, cam, rowcol[i * 2], rowcol[i * 2 + 1], second);
    out[i * 2] = first;
    out[i * 2 + 1] = second;
}
// The single-precision filter of the timed node loop next to the exact test, box by box: out[i] = exact | filter << 1.
// Boxes arrive as (min, max) doubles; the host rounds them outward exactly as the scene image does (rth::f32_down / f32_up).
__global__ void k_bbox_filter(int n, const double *rays, const double *boxes, const float *boxes32, float bmax, int32_t *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = rays + i * 6, *b = boxes + i * 6;
    const float *f = boxes32 + i * 6;
    d2 bx, by, bz;
    bx.x = b[0]; bx.y = b[3]; by.x = b[1]; by.y = b[4]; bz.x = b[2]; bz.y = b[5];
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const bool exact = bbox_hits(1.0 / d.x, 1.0 / d.y, 1.0 / d.z, o, bx, by, bz);
    const WalkCtx32 c = walk_ctx32(o, d, bmax);
    // the loop's own instruction forms (v_max3 / v_min3 / v_max / v_cmp_nlt): NaN handling is theirs
    const float nx = c.nX ? f[3] : f[0], fx = c.nX ? f[0] : f[3], ny = c.nY ? f[4] : f[1], fy = c.nY ? f[1] : f[4], nz = c.nZ ? f[5] : f[2], fz = c.nZ ? f[2] : f[5];
    float t0 = nx, t1 = fx, t2 = ny, t3 = fy, t4 = nz, t5 = fz;
    unsigned long long m;
    asm volatile("v_fma_f32 %0, %0, %7, %10\n\tv_fma_f32 %1, %1, %7, %13\n\t"
                 "v_fma_f32 %2, %2, %8, %11\n\tv_fma_f32 %3, %3, %8, %14\n\t"
                 "v_fma_f32 %4, %4, %9, %12\n\tv_fma_f32 %5, %5, %9, %15\n\t"
                 "v_max3_f32 %0, %0, %2, %4\n\tv_min3_f32 %1, %1, %3, %5\n\tv_max_f32 %0, 0, %0\n\tv_cmp_nlt_f32_e64 %6, %1, %0"
                 : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3), "+v"(t4), "+v"(t5), "=s"(m)
                 : "v"(c.ix), "v"(c.iy), "v"(c.iz), "v"(c.cnx), "v"(c.cny), "v"(c.cnz), "v"(c.cfx), "v"(c.cfy), "v"(c.cfz));
    const bool filter = (m >> (threadIdx.x & 63)) & 1ull;
    out[i] = (exact ? 1 : 0) | (filter ? 2 : 0) | (bbox_filter(c, f[0], f[3], f[1], f[4], f[2], f[5]) ? 4 : 0);
}
__global__ void k_trace_ray(const RenderParams p, int depth, int n, const double *rays, uint32_t *rng, uint8_t *col_out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SceneView<false> sc = make_view<false>(p, nullptr);
    const double *r = rays + i * 6;
    Rng g; g.x = rng[i * 4]; g.y = rng[i * 4 + 1]; g.z = rng[i * 4 + 2]; g.w = rng[i * 4 + 3];
    Counters cnt; cnt.rays = cnt.aabb = cnt.prim = cnt.refl = 0;
    uint32_t c = trace_ray<false, false>(sc, depth, mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), g, cnt);
    st_rgb(col_out + i * 3, c);
    rng[i * 4] = g.x; rng[i * 4 + 1] = g.y; rng[i * 4 + 2] = g.z; rng[i * 4 + 3] = g.w;
}
__global__ void k_texture(const RenderParams p, int tex, int n, const double *pts, double *uv, uint8_t *col, int prog) { // prog: the scene holds a texture program
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double u[2] = {__builtin_nan(""), __builtin_nan("")};
    uint32_t c = prog ? texture_colour_at_prog(p.tex, p.texels, tex, mk(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]), u) : texture_colour_at(p.tex, p.texels, tex, mk(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]), u);
    if (uv) { uv[i * 2] = u[0]; uv[i * 2 + 1] = u[1]; }
    st_rgb(col + i * 3, c);
}

template <class K, class... A> static void launch_n(K kernel, int n, A... args) { // n items, 256 per block, on the null stream
    if (n) hipLaunchKernelGGL(kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, 0, args...);
}

// What every rt_dev_* entry point shares (each keeps its argument check, its kernel, its buffer shapes and its host pre/post step).
// hook(): the body runs inside guarded() with `device` current; scene_hook(): the same, with the scene's device copy described in a
// RenderParams.  hook_run(): the buffers go up, `launch` enqueues the kernel, the device is waited for, the buffers come down.
template <class F> static int hook(const char *entry, int32_t device, F &&body) {
    return guarded(entry, [&]() -> int {
        DeviceGuard guard;
        const int rc = guard.enter(device);
        return rc != RT_OK ? rc : body();
    });
}
template <class F> static int scene_hook(const char *entry, int32_t device, const rt_scene *scene, F &&body) {
    return guarded(entry, [&]() -> int {
        if (!scene) return fail(RT_ERR_INVALID_ARGUMENT, "scene is NULL");
        DeviceGuard guard;
        int rc = guard.enter(device);
        if (rc != RT_OK) return rc;
        DeviceScene *ds = nullptr;
        rc = device_scene(const_cast<rt_scene *>(scene), device, &ds);
        if (rc != RT_OK) return rc;
        RenderParams p{};
        p.off = scene->host.off;
        p.scene_image = ds->image;
        p.tex = ds->tex;
        p.texels = ds->texels;
        return body(p);
    });
}
template <class Launch, class... Bufs> static int hook_run(Launch &&launch, Bufs &...bufs) {
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e : bufs.up()), ...);
    if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("hook buffers: ") + hipGetErrorString(e));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    ((e = e != hipSuccess ? e : bufs.down()), ...);
    if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("hook results: ") + hipGetErrorString(e));
    return RT_OK;
}

} // namespace

extern "C" {

int rt_dev_float_producer(int32_t device, const uint32_t state[4], int32_t n, double *out) {
    if (!state || !out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_float_producer", device, [&]() -> int {
        auto d = dev_out(out, (size_t) n);
        Rng r; r.x = state[0]; r.y = state[1]; r.z = state[2]; r.w = state[3];
        return hook_run([&] { if (n) hipLaunchKernelGGL(k_float_producer, dim3(1), dim3(64), 0, 0, r, n, d.p); }, d);
    });
}

int rt_dev_stream_state(int32_t device, uint64_t seed, int32_t n, const uint64_t *pixel, const uint32_t *sample, uint32_t *state_out) {
    if (!pixel || !sample || !state_out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_stream_state", device, [&]() -> int {
        auto dp = dev_in(pixel, (size_t) n);
        auto dsm = dev_in(sample, (size_t) n);
        auto dout = dev_out(state_out, (size_t) n * 4);
        return hook_run([&] { launch_n(k_stream_state, n, mix64(seed + 0x9E3779B97F4A7C15ull), n, dp.p, dsm.p, dout.p); }, dp, dsm, dout);
    });
}

int rt_dev_bbox_hits(int32_t device, int32_t n, const double *rays, const double *boxes, int32_t *hit_out) {
    if (!rays || !boxes || !hit_out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_bbox_hits", device, [&]() -> int {
        auto dr = dev_in(rays, (size_t) n * 6), db = dev_in(boxes, (size_t) n * 6);
        auto dh = dev_out(hit_out, (size_t) n);
        return hook_run([&] { launch_n(k_bbox_hits, n, n, dr.p, db.p, dh.p); }, dr, db, dh);
    });
}

int rt_dev_bbox_filter(int32_t device, int32_t n, const double *rays, const double *boxes, double bmax, int32_t *out) {
    if (!rays || !boxes || !out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_bbox_filter", device, [&]() -> int {
        std::vector<float> b32((size_t) n * 6);
        float bm = 1e-30f; // as encode_image: >= every |coordinate| of the batch's rounded boxes, unless the caller names a larger scale
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) {
                const float lo = rth::f32_down(boxes[(size_t) i * 6 + a]), hi = rth::f32_up(boxes[(size_t) i * 6 + 3 + a]);
                b32[(size_t) i * 6 + a] = lo; b32[(size_t) i * 6 + 3 + a] = hi;
                if (std::fabs(lo) > bm) bm = std::fabs(lo);
                if (std::fabs(hi) > bm) bm = std::fabs(hi);
            }
        if (bmax > (double) bm) bm = rth::f32_up(bmax);
        auto dr = dev_in(rays, (size_t) n * 6), db = dev_in(boxes, (size_t) n * 6);
        auto df = dev_in((const float *) b32.data(), (size_t) n * 6);
        auto dh = dev_out(out, (size_t) n);
        return hook_run([&] { launch_n(k_bbox_filter, n, n, dr.p, db.p, df.p, bm, dh.p); }, dr, db, df, dh);
    });
}

int rt_dev_sphere_first_intersection(int32_t device, int32_t n, const double *rays, const double *spheres, double *t_out) {
    if (!rays || !spheres || !t_out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_sphere_first_intersection", device, [&]() -> int {
        auto dr = dev_in(rays, (size_t) n * 6), dsph = dev_in(spheres, (size_t) n * 4);
        auto dt = dev_out(t_out, (size_t) n);
        return hook_run([&] { launch_n(k_sphere_isect, n, n, dr.p, dsph.p, dt.p); }, dr, dsph, dt);
    });
}

int rt_dev_plane_intersection(int32_t device, int32_t n, const double *rays, const double *planes, double *t_out) {
    if (!rays || !planes || !t_out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_plane_intersection", device, [&]() -> int {
        auto dr = dev_in(rays, (size_t) n * 6), dpl = dev_in(planes, (size_t) n * 6);
        auto dt = dev_out(t_out, (size_t) n);
        return hook_run([&] { launch_n(k_plane_isect, n, n, dr.p, dpl.p, dt.p); }, dr, dpl, dt);
    });
}

int rt_dev_pixel_combine(int32_t device, int32_t n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
    if (!a || !b || !out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_pixel_combine", device, [&]() -> int {
        auto da = dev_in(a, (size_t) n * 3), db = dev_in(b, (size_t) n * 3);
        auto dout = dev_out(out, (size_t) n * 3);
        return hook_run([&] { launch_n(k_pixel_combine, n, n, da.p, db.p, dout.p); }, da, db, dout);
    });
}

int rt_dev_pixel_darken(int32_t device, int32_t n, const uint8_t *p, const double *albedo, uint8_t *out) {
    if (!p || !albedo || !out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_pixel_darken", device, [&]() -> int {
        auto dp = dev_in(p, (size_t) n * 3);
        auto da = dev_in(albedo, (size_t) n);
        auto dout = dev_out(out, (size_t) n * 3);
        return hook_run([&] { launch_n(k_pixel_darken, n, n, dp.p, da.p, dout.p); }, dp, da, dout);
    });
}

int rt_dev_arith(int32_t device, int32_t op, int32_t n, const double *a, const double *b, double *out) {
    if (!a || !out || n < 0 || op < 0 || op > 9 || ((op == 3 || op == 9) && !b)) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return hook("rt_dev_arith", device, [&]() -> int {
        auto da = dev_in(a, (size_t) n), db = dev_in(b, b ? (size_t) n : 0);
        auto dout = dev_out(out, (size_t) n);
        return hook_run([&] { launch_n(k_arith, n, op, n, da.p, db.p, dout.p); }, da, db, dout);
    });
}

int rt_dev_reflection(int32_t device, const rt_scene *scene, int32_t n, const int32_t *index, const double *ray_in, const uint8_t *colour_in,
                      const double *strike, uint32_t *rng_state, int32_t *absorbed, uint8_t *colour_out, double *ray_out) {
    if (!index || !ray_in || !colour_in || !strike || !rng_state || !absorbed || !colour_out || !ray_out || n < 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return scene_hook("rt_dev_reflection", device, scene, [&](const RenderParams &p) -> int {
        std::vector<int32_t> obj((size_t) n);
        RT_TRY(ensure_host_mirror(scene));
        for (int i = 0; i < n; ++i) {
            if (index[i] < 0 || (size_t) index[i] >= scene->host.origToObj.size()) return fail(RT_ERR_INVALID_ARGUMENT, "hittable index out of range");
            obj[(size_t) i] = scene->host.origToObj[(size_t) index[i]];
        }
        auto dobj = dev_in((const int32_t *) obj.data(), (size_t) n);
        auto dab = dev_out(absorbed, (size_t) n);
        auto dri = dev_in(ray_in, (size_t) n * 6), dst = dev_in(strike, (size_t) n * 3);
        auto dro = dev_out(ray_out, (size_t) n * 6);
        auto dci = dev_in(colour_in, (size_t) n * 3);
        auto dco = dev_out(colour_out, (size_t) n * 3);
        auto drng = dev_inout(rng_state, (size_t) n * 4);
        return hook_run([&] { launch_n(k_reflection, n, p, n, dobj.p, dri.p, dci.p, dst.p, drng.p, dab.p, dco.p, dro.p); }, dobj, dab, dri, dst, dro, dci, dco, drng);
    });
}

// hittable indices of the scene's object table -> rt_scene_create's
static int to_orig(const rt_scene *scene, int32_t n, int32_t *hit_index) {
    RT_TRY(ensure_host_mirror(scene));
    for (int i = 0; i < n; ++i) if (hit_index[i] >= 0) hit_index[i] = scene->host.objToOrig[(size_t) hit_index[i]];
    return RT_OK;
}

int rt_dev_hit_object(int32_t device, const rt_scene *scene, int32_t n, const double *rays, int32_t *hit_index, double *strike, uint32_t *counters) {
    if (!rays || !hit_index || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return scene_hook("rt_dev_hit_object", device, scene, [&](const RenderParams &p) -> int {
        auto dr = dev_in(rays, (size_t) n * 6);
        auto dh = dev_out(hit_index, (size_t) n);
        auto dsk = dev_out(strike, strike ? (size_t) n * 3 : 0);
        auto dc = dev_out(counters, counters ? (size_t) n * 2 : 0);
        const int rc = hook_run([&] { launch_n(k_hit_object, n, p, n, dr.p, dh.p, dsk.p, dc.p); }, dr, dh, dsk, dc);
        return rc == RT_OK ? to_orig(scene, n, hit_index) : rc;
    });
}

int rt_dev_hit_object_lds(int32_t device, const rt_scene *scene, int32_t n, const double *rays, int32_t *hit_index, double *strike) {
    if (!rays || !hit_index || !strike || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return scene_hook("rt_dev_hit_object_lds", device, scene, [&](const RenderParams &p) -> int {
        // (a fit test of its own: the image alone, no wave scratch -- this kernel has none)
        const size_t ldsBytes = scene->host.off.lds32_total;
        if (ldsBytes > RT_LDS_BYTES || scene->host.nBounded + scene->host.nUnbounded >= 16384u) return fail(RT_ERR_UNSUPPORTED, "the scene does not fit the LDS");
        int rc = allow_full_lds((const void *) k_hit_object_lds);
        if (rc != RT_OK) return rc;
        auto dr = dev_in(rays, (size_t) n * 6);
        auto dh = dev_out(hit_index, (size_t) n);
        auto dsk = dev_out(strike, (size_t) n * 3);
        rc = hook_run([&] { if (n) hipLaunchKernelGGL(k_hit_object_lds, dim3((unsigned) ((n + 1023) / 1024)), dim3(1024), ldsBytes, 0, p, n, dr.p, dh.p, dsk.p); }, dr, dh, dsk);
        return rc == RT_OK ? to_orig(scene, n, hit_index) : rc;
    });
}

// (on the device, inside guarded: rt_dev_pixel_candidates)
static int pixel_candidates(const RenderParams &p, const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, int32_t n,
                            const int32_t *row_col, int32_t *leaves_out) {
    const size_t ldsBytes = scene->host.off.lds32_total;
    const bool narrow = scene->host.nBounded + scene->host.nUnbounded < 16384u;
    const bool lds = default_lds_resident(scene->host); // the timed render's view of this scene (rt_scene_info.lds_resident)
    const CameraParams cam = camera_params(camera, max_w, max_h);
    if (lds) {
        const int rc = allow_full_lds((const void *) k_pixel_candidates);
        if (rc != RT_OK) return rc;
    }
    std::vector<uint32_t> w((size_t) n * 2);
    auto drc = dev_in(row_col, (size_t) n * 2);
    auto dout = dev_out(w.data(), (size_t) n * 2);
    const int rc = hook_run([&] {
        if (lds && n) hipLaunchKernelGGL(k_pixel_candidates, dim3((unsigned) ((n + 1023) / 1024)), dim3(1024), ldsBytes, 0, p, cam, n, drc.p, dout.p);
        if (!lds) launch_n(k_pixel_candidates_glb, n, p, cam, n, drc.p, dout.p);
    }, drc, dout);
    if (rc != RT_OK) return rc;
    // decode: up to four hittable indices per pixel (-1 = none); leaves_out[i*4] = -2 when the pixel's camera rays walk the tree.
    // Below 16384 objects the words hold two 16-bit entries each (RTD_PEND_MARK | object); beyond, one full-width entry each
    // (RTD_PEND_WIDE | object, at most two candidates).
    RT_TRY(ensure_host_mirror(scene));
    const size_t nObj = scene->host.objToOrig.size();
    for (int i = 0; i < n; ++i) {
        int32_t *o = leaves_out + (size_t) i * 4;
        o[0] = o[1] = o[2] = o[3] = -1;
        if (w[(size_t) i * 2] == RTD_CAND_WALK) { o[0] = -2; continue; }
        int k = 0;
        for (int h = 0; h < 2; ++h) {
            const uint32_t word = w[(size_t) i * 2 + (size_t) h];
            for (int half = 0; half < (narrow ? 2 : 1); ++half) {
                const uint32_t e = !narrow ? word : half == 0 ? (word & 0xFFFFu) : (word >> 16);
                if (e == 0u || k >= 4) continue;
                const uint32_t obj = narrow ? (e & (RTD_PEND_MARK - 1u)) : (e & ~RTD_PEND_WIDE);
                if (obj >= nObj) return fail(RT_ERR_HIP, "pixel_candidates returned an object out of range");
                o[k++] = scene->host.objToOrig[(size_t) obj];
            }
        }
    }
    return RT_OK;
}
int rt_dev_pixel_candidates(int32_t device, const rt_scene *scene, const rt_camera *camera, int32_t max_w, int32_t max_h, int32_t n,
                            const int32_t *row_col, int32_t *leaves_out) {
    if (!camera || !row_col || !leaves_out || n < 0 || max_w <= 0 || max_h <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return scene_hook("rt_dev_pixel_candidates", device, scene, [&](const RenderParams &p) -> int {
        return pixel_candidates(p, scene, camera, max_w, max_h, n, row_col, leaves_out);
    });
}

int rt_dev_trace_ray(int32_t device, const rt_scene *scene, int32_t bounce_depth, int32_t n, const double *rays, uint32_t *rng_state, uint8_t *colour_out) {
    if (!rays || !rng_state || !colour_out || n < 0 || bounce_depth < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    return scene_hook("rt_dev_trace_ray", device, scene, [&](const RenderParams &p) -> int {
        auto dr = dev_in(rays, (size_t) n * 6);
        auto drng = dev_inout(rng_state, (size_t) n * 4);
        auto dc = dev_out(colour_out, (size_t) n * 3);
        return hook_run([&] { launch_n(k_trace_ray, n, p, bounce_depth, n, dr.p, drng.p, dc.p); }, dr, drng, dc);
    });
}

int rt_dev_texture_colour_at(int32_t device, const rt_scene *scene, int32_t texture, int32_t n, const double *points, double *uv_out, uint8_t *colour_out) {
    if (!points || !colour_out || n < 0) return fail(RT_ERR_INVALID_ARGUMENT, "bad argument");
    if (!scene || texture < 0 || (size_t) texture >= scene->host.texRecs.size()) return fail(RT_ERR_INVALID_ARGUMENT, "texture index out of range");
    return scene_hook("rt_dev_texture_colour_at", device, scene, [&](const RenderParams &p) -> int {
        auto dp = dev_in(points, (size_t) n * 3);
        auto duv = dev_out(uv_out, uv_out ? (size_t) n * 2 : 0);
        auto dc = dev_out(colour_out, (size_t) n * 3);
        return hook_run([&] { launch_n(k_texture, n, p, texture, n, dp.p, duv.p, dc.p, scene->host.hasPrograms ? 1 : 0); }, dp, duv, dc);
    });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// BoundingBoxTree.make's tree on the device (rt_tree_plan.h, rt_tree_kernels.h; DESIGN.md "The reference tree on the device")
// ------------------------------------------------------------------------------------------------------------
static int create_scene_on_device(const char *entry, const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                                  const rt_scene_options *options, int32_t device, bool walk_tree_too, rt_scene **out);
struct TexelSources; // (rt_scene_create_*textures, below: where each IMAGE record's texels come from)
static int scene_from_host_records(const char *entry, const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures, int walk,
                                   int32_t device, bool walk_tree_too, rt_scene **out, const TexelSources *sources = nullptr, hipStream_t st = nullptr);
static const uint8_t *external_flags(const TexelSources *sources);
// The texel blob of `h` (laid out by build_textures) on the current device, each image from its source, on `st`; waits for the stream.
// *out: the blob (hipMalloc; the caller's to free), NULL when the scene has no image.
static int place_texels(const rth::HostScene &h, const rt_texture *textures, size_t n_textures, const TexelSources &sources, hipStream_t st, unsigned char **out);
static const char *const kNanBox = "a box coordinate is NaN: it has no order; nothing was written";

static int check_tree_host(size_t n, const double *boxes) {
    if (n > 0 && !boxes) return fail(RT_ERR_INVALID_ARGUMENT, "boxes is NULL");
    if (n > (size_t) RTT_MAX_BOXES) return fail(RT_ERR_UNSUPPORTED, "more than 4,500,000 boxes (the scene's own limit)");
    return RT_OK;
}
static int check_tree_device(size_t n, const void *d_boxes, const void *d_skip, const void *d_prim, const void *d_node_boxes, const void *d_order) {
    if (n > 0 && !d_boxes) return fail(RT_ERR_INVALID_ARGUMENT, "d_boxes is NULL");
    if ((uintptr_t) d_boxes % 8u) return fail(RT_ERR_INVALID_ARGUMENT, "d_boxes is not 8-byte aligned");
    if ((uintptr_t) d_node_boxes % 8u) return fail(RT_ERR_INVALID_ARGUMENT, "d_node_boxes is not 8-byte aligned");
    if ((uintptr_t) d_skip % 4u) return fail(RT_ERR_INVALID_ARGUMENT, "d_skip is not 4-byte aligned");
    if ((uintptr_t) d_prim % 4u) return fail(RT_ERR_INVALID_ARGUMENT, "d_prim is not 4-byte aligned");
    if ((uintptr_t) d_order % 4u) return fail(RT_ERR_INVALID_ARGUMENT, "d_order is not 4-byte aligned");
    if (n > (size_t) RTT_MAX_BOXES) return fail(RT_ERR_UNSUPPORTED, "more than 4,500,000 boxes (the scene's own limit)");
    return RT_OK;
}
static bool any_nan(const double *v, size_t count) {
    for (size_t i = 0; i < count; ++i) if (v[i] != v[i]) return true;
    return false;
}
// TreeBuilder on the caller's boxes (n > 0, checked)
static void tree_on_host(size_t n, const double *boxes, rth::FlatTree &t) {
    std::vector<rth::Box> ob(n);
    for (size_t j = 0; j < n; ++j)
        for (int a = 0; a < 3; ++a) { ob[j].mn[a] = boxes[j * 6 + (size_t) a * 2]; ob[j].mx[a] = boxes[j * 6 + (size_t) a * 2 + 1]; }
    std::vector<int32_t> ids(n);
    for (size_t j = 0; j < n; ++j) ids[j] = (int32_t) j;
    rth::TreeBuilder(ob, t).go(ids, 1);
}

// Enqueues one build on `st` (n > 0, arguments checked, the device current).  Scratch, stream-ordered: the NaN flag; above RTT_S boxes also
// the order (twice), the slots, the winning axes, three arrays of sort records and the partial boxes.  Never waits for the device.
static int enqueue_tree(size_t n_boxes, const void *d_boxes, void *d_skip, void *d_prim, void *d_node_boxes, void *d_order, hipStream_t st, FormatPending &fp) {
    const uint32_t n = (uint32_t) n_boxes;
    const double *boxes = (const double *) d_boxes;
    const rtk::Outputs out{(int32_t *) d_skip, (int32_t *) d_prim, (double *) d_node_boxes, (int32_t *) d_order};
    const int32_t Lg = rtt::levels_above(n, RTT_S);
    uint32_t P = RTK_TILE;
    while (P < n) P <<= 1;
    size_t partials = (n + RTT_PART - 1u) / RTT_PART;
    for (int32_t l = 0; l < Lg; ++l) {
        const size_t parts = (rtt::left_count(rtt::max_count(n, l)) + RTT_PART - 1u) / RTT_PART;
        partials = std::max(partials, ((size_t) 1 << l) * parts * 6u);
    }
    auto up = [](size_t v) { return (v + 15u) & ~(size_t) 15u; };
    const size_t ids_at = 16, slot_at = ids_at + up((size_t) n * 8u), best_at = slot_at + up((size_t) n * 4u), rec_at = best_at + up(((size_t) 1 << Lg) * 4u),
                 part_at = rec_at + (size_t) P * 3u * sizeof(rtk::Rec), total = part_at + partials * sizeof(rtt::Box);
    HIP_TRY(hipMallocAsync((void **) &fp.scr, Lg == 0 ? 16 : total, st));
    fp.st = st;
    HIP_TRY(hipMemsetAsync(fp.scr, 0, 16, st));
    int *bad = (int *) fp.scr;
    {
        const uint64_t count = (uint64_t) n * 6u;
        const uint64_t want = (count + RTK_BLOCK - 1u) / RTK_BLOCK;
        hipLaunchKernelGGL(rtk::tree_check_kernel, dim3((unsigned) (want < 4096u ? want : 4096u)), dim3(RTK_BLOCK), 0, st, boxes, count, bad);
    }
    if (Lg == 0) {
        hipLaunchKernelGGL(rtk::tree_lds_kernel, dim3(1), dim3(RTK_LDS_THREADS), 0, st, n, 0, (const uint32_t *) nullptr, boxes, out, (const int *) bad);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
    uint32_t *ids[2] = {(uint32_t *) (fp.scr + ids_at), (uint32_t *) (fp.scr + ids_at) + n};
    uint32_t *slot = (uint32_t *) (fp.scr + slot_at), *best = (uint32_t *) (fp.scr + best_at);
    rtk::Rec *rec = (rtk::Rec *) (fp.scr + rec_at);
    rtt::Box *partial = (rtt::Box *) (fp.scr + part_at);
    const unsigned per_n = (n + RTK_BLOCK - 1u) / RTK_BLOCK, per_P = P / RTK_BLOCK;
    hipLaunchKernelGGL(rtk::tree_init_kernel, dim3(per_n), dim3(RTK_BLOCK), 0, st, n, ids[0], slot, (const int *) bad);
    {
        const uint32_t parts = (n + RTT_PART - 1u) / RTT_PART;
        hipLaunchKernelGGL(rtk::tree_root_parts_kernel, dim3(parts), dim3(RTK_BLOCK), 0, st, n, boxes, partial, (const int *) bad);
        hipLaunchKernelGGL(rtk::tree_root_finish_kernel, dim3(1), dim3(64), 0, st, n, parts, (const rtt::Box *) partial, out, (const int *) bad);
    }
    for (int32_t l = 0; l < Lg; ++l) {
        const uint32_t *cur = ids[l & 1];
        uint32_t *nxt = ids[(l + 1) & 1];
        hipLaunchKernelGGL(rtk::tree_fill_kernel, dim3(per_P), dim3(RTK_BLOCK), 0, st, n, P, cur, (const uint32_t *) slot, boxes, rec, (const int *) bad);
        hipLaunchKernelGGL(rtk::tree_sort_tile_kernel, dim3(P / RTK_TILE, 3), dim3(RTK_TILE_THREADS), 0, st, rec, P, 2u, (uint32_t) RTK_TILE, (const int *) bad);
        for (uint32_t k = 2u * RTK_TILE; k <= P && k != 0u; k <<= 1) {
            for (uint32_t j = k >> 1; j >= (uint32_t) RTK_TILE; j >>= 1)
                hipLaunchKernelGGL(rtk::tree_sort_step_kernel, dim3(P / 2u / RTK_BLOCK, 3), dim3(RTK_BLOCK), 0, st, rec, P, k, j, (const int *) bad);
            hipLaunchKernelGGL(rtk::tree_sort_tile_kernel, dim3(P / RTK_TILE, 3), dim3(RTK_TILE_THREADS), 0, st, rec, P, k, k, (const int *) bad);
        }
        const uint32_t slots = 1u << l, parts = (rtt::left_count(rtt::max_count(n, l)) + RTT_PART - 1u) / RTT_PART;
        hipLaunchKernelGGL(rtk::tree_parts_kernel, dim3(slots * parts, 6), dim3(RTK_BLOCK), 0, st, n, P, l, parts, cur, (const rtk::Rec *) rec, boxes, partial,
                           (const int *) bad);
        hipLaunchKernelGGL(rtk::tree_choose_kernel, dim3((slots + RTK_BLOCK - 1u) / RTK_BLOCK), dim3(RTK_BLOCK), 0, st, n, P, l, parts, cur, (const rtk::Rec *) rec,
                           boxes, (const rtt::Box *) partial, best, out, (const int *) bad);
        hipLaunchKernelGGL(rtk::tree_reorder_kernel, dim3(per_n), dim3(RTK_BLOCK), 0, st, n, P, l, cur, nxt, slot, (const rtk::Rec *) rec, (const uint32_t *) best,
                           (const int *) bad);
    }
    hipLaunchKernelGGL(rtk::tree_lds_kernel, dim3(1u << Lg), dim3(RTK_LDS_THREADS), 0, st, n, Lg, (const uint32_t *) ids[Lg & 1], boxes, out, (const int *) bad);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
// Waits for the stream and reads what the check found: a NaN coordinate, of which nothing was written.
static int finish_tree(FormatPending &fp) {
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, fp.scr, sizeof(bad), hipMemcpyDeviceToHost, fp.st));
    HIP_TRY(hipStreamSynchronize(fp.st));
    if (bad) return fail(RT_ERR_INVALID_ARGUMENT, kNanBox);
    return RT_OK;
}

extern "C" {

int64_t rt_tree_nodes(size_t n) { return rtt::node_count((uint64_t) n); }
int32_t rt_tree_depth(size_t n) { return rtt::depth((uint64_t) n); }
int32_t rt_tree_lds_boxes(void) { return RTT_S; }

int rt_tree_make_host(size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes, int32_t *order) {
    RT_TRY(check_tree_host(n, boxes));
    if (n == 0) return RT_OK;
    return guarded("rt_tree_make_host", [&]() {
        if (any_nan(boxes, n * 6u)) return fail(RT_ERR_INVALID_ARGUMENT, kNanBox);
        rth::FlatTree t;
        tree_on_host(n, boxes, t);
        size_t leaf = 0;
        for (size_t i = 0; i < t.skip.size(); ++i) {
            if (skip) skip[i] = t.skip[i];
            if (prim) prim[i] = t.prim[i];
            if (node_boxes) for (int a = 0; a < 3; ++a) { node_boxes[i * 6 + (size_t) a * 2] = t.box[i].mn[a]; node_boxes[i * 6 + (size_t) a * 2 + 1] = t.box[i].mx[a]; }
            if (t.prim[i] >= 0) { if (order) order[leaf] = t.prim[i]; ++leaf; }
        }
        return (int) RT_OK;
    });
}

int rt_tree_make_device(int32_t device, size_t n, const void *d_boxes, void *d_skip, void *d_prim, void *d_node_boxes, void *d_order, void *stream) {
    RT_TRY(check_tree_device(n, d_boxes, d_skip, d_prim, d_node_boxes, d_order));
    if (n == 0) return RT_OK;
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    FormatPending fp;
    RT_TRY(enqueue_tree(n, d_boxes, d_skip, d_prim, d_node_boxes, d_order, (hipStream_t) stream, fp));
    return finish_tree(fp);
}

int rt_tree_make(int32_t device, size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes, int32_t *order) {
    RT_TRY(check_tree_host(n, boxes));
    if (n == 0) return RT_OK;
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const size_t nn = (size_t) rtt::node_count(n);
    Staging sg;
    RT_TRY(sg.in({{boxes, n * 48u, SEG_IN}, {skip, nn * 4u, SEG_OUT}, {prim, nn * 4u, SEG_OUT}, {node_boxes, nn * 48u, SEG_OUT}, {order, n * 4u, SEG_OUT}}));
    FormatPending fp;
    RT_TRY(enqueue_tree(n, sg.dev[0], sg.dev[1], sg.dev[2], sg.dev[3], sg.dev[4], nullptr, fp));
    RT_TRY(finish_tree(fp));
    return sg.out();
}

int rt_scene_create_gpu_tree(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                             const rt_scene_options *options, int32_t device, rt_scene **out) {
    return create_scene_on_device("rt_scene_create_gpu_tree", hittables, n_hittables, textures, n_textures, options, device, false, out);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// The tree the device walks, built on the device (rt_walk_plan.h, rt_walk_kernels.h; DESIGN.md "The walk tree on the device")
// ------------------------------------------------------------------------------------------------------------
static const char *const kNonFiniteBox = "a box coordinate is not finite: a scene never builds the walk tree over such boxes; nothing was written";

static bool any_non_finite(const double *v, size_t count) {
    for (size_t i = 0; i < count; ++i) if (!(v[i] - v[i] == 0.0)) return true;
    return false;
}
static void boxes_of(size_t n, const double *boxes, std::vector<rth::Box> &ob) {
    ob.resize(n);
    for (size_t j = 0; j < n; ++j)
        for (int a = 0; a < 3; ++a) { ob[j].mn[a] = boxes[j * 6 + (size_t) a * 2]; ob[j].mx[a] = boxes[j * 6 + (size_t) a * 2 + 1]; }
}
// the longest root-to-leaf path of a pre-order tree with skip links
static int depth_of(const std::vector<int32_t> &skip) {
    std::vector<int32_t> up; // the ends of the subtrees the walk is inside
    int depth = 0;
    for (size_t i = 0; i < skip.size(); ++i) {
        while (!up.empty() && (int32_t) i >= up.back()) up.pop_back();
        up.push_back(skip[i]);
        if ((int) up.size() > depth) depth = (int) up.size();
    }
    return depth;
}

// One build on `st` (n > 0, arguments checked, the device current); returns when the stream has finished it.  Scratch, stream-ordered: the
// counters, the order (twice), the segment lists, and per segment of a level its bounds, bins, choice and children's boxes.  The host reads
// two counters per level of segments above RTW_SWEEP (how many, the largest) and sizes the next level's launches from them; the number of
// levels is bounded by rtw::levels_below.
static int build_walk_tree(size_t n_boxes, const void *d_boxes, void *d_skip, void *d_prim, void *d_node_boxes, hipStream_t st) {
    using namespace rtwk;
    const uint32_t n = (uint32_t) n_boxes;
    const double *boxes = (const double *) d_boxes;
    const Outputs out{(int32_t *) d_skip, (int32_t *) d_prim, (double *) d_node_boxes, nullptr};
    const uint32_t capBig = n / (uint32_t) (RTW_SWEEP + 1) + 1u, capSmall = n / 2u + 1u;
    auto up = [](size_t v) { return (v + 63u) & ~(size_t) 63u; };
    const size_t ids_at = up(sizeof(Ctrl)), big_at = ids_at + up((size_t) n * 8u), small_at = big_at + up((size_t) capBig * 2u * sizeof(Seg)),
                 dec_at = small_at + up((size_t) capSmall * sizeof(Seg)), ones_at = dec_at + up((size_t) capBig * sizeof(Dec)),
                 zeros_at = ones_at + up((size_t) capBig * sizeof(Ones)), total = zeros_at + up((size_t) capBig * sizeof(Zeros));
    FormatPending fp;
    HIP_TRY(hipMallocAsync((void **) &fp.scr, total, st));
    fp.st = st;
    HIP_TRY(hipMemsetAsync(fp.scr, 0, sizeof(Ctrl), st));
    Ctrl *ctrl = (Ctrl *) fp.scr;
    uint32_t *ids[2] = {(uint32_t *) (fp.scr + ids_at), (uint32_t *) (fp.scr + ids_at) + n};
    Seg *big[2] = {(Seg *) (fp.scr + big_at), (Seg *) (fp.scr + big_at) + capBig};
    Seg *small = (Seg *) (fp.scr + small_at);
    Dec *dec = (Dec *) (fp.scr + dec_at);
    Ones *ones = (Ones *) (fp.scr + ones_at);
    Zeros *zeros = (Zeros *) (fp.scr + zeros_at);
    {
        const uint64_t count = (uint64_t) n * 6u, want = (count + RTWK_BLOCK - 1u) / RTWK_BLOCK;
        hipLaunchKernelGGL(walk_check_kernel, dim3((unsigned) (want < 4096u ? want : 4096u)), dim3(RTWK_BLOCK), 0, st, boxes, count, &ctrl->bad);
    }
    HIP_TRY(hipMemsetAsync(ones, 0xFF, sizeof(Ones), st));
    HIP_TRY(hipMemsetAsync(zeros, 0, sizeof(Zeros), st));
    hipLaunchKernelGGL(walk_root_box_kernel, dim3((n + RTWK_PART - 1u) / RTWK_PART), dim3(RTWK_BLOCK), 0, st, n, boxes, ids[0], ones, zeros, (const int *) &ctrl->bad);
    hipLaunchKernelGGL(walk_root_emit_kernel, dim3(1), dim3(64), 0, st, n, boxes, (const uint32_t *) ids[0], (const Ones *) ones, (const Zeros *) zeros, ctrl, big[0], capBig,
                       small, capSmall, out);
    Ctrl h{};
    HIP_TRY(hipMemcpyAsync(&h, ctrl, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t bound = rtw::levels_below(n, 1);
    uint32_t sel = 0u;
    for (int32_t l = 0; l < bound && !h.bad && h.nbig[sel] > 0u; ++l, sel ^= 1u) {
        const uint32_t nbig = h.nbig[sel], parts = (h.maxcount[sel] + RTWK_PART - 1u) / RTWK_PART, nxt = sel ^ 1u;
        if (nbig > capBig) return fail(RT_ERR_HIP, "walk tree build: more segments than boxes allow");
        const Seg *cur = big[sel];
        HIP_TRY(hipMemsetAsync(ones, 0xFF, (size_t) nbig * sizeof(Ones), st));
        HIP_TRY(hipMemsetAsync(zeros, 0, (size_t) nbig * sizeof(Zeros), st));
        hipLaunchKernelGGL(walk_bounds_kernel, dim3(nbig, parts), dim3(RTWK_BLOCK), 0, st, cur, (const uint32_t *) ids[0], (const uint32_t *) ids[1], boxes, ones, zeros, ctrl, nxt);
        hipLaunchKernelGGL(walk_bins_kernel, dim3(nbig, parts), dim3(RTWK_BLOCK), 0, st, cur, (const uint32_t *) ids[0], (const uint32_t *) ids[1], boxes, ones, zeros,
                           (const Ctrl *) ctrl);
        hipLaunchKernelGGL(walk_choose_kernel, dim3((nbig + 63u) / 64u), dim3(64), 0, st, nbig, cur, (const Ones *) ones, (const Zeros *) zeros, dec, (const Ctrl *) ctrl);
        hipLaunchKernelGGL(walk_select_kernel, dim3(nbig), dim3(RTWK_SELECT_THREADS), 0, st, cur, (const uint32_t *) ids[0], (const uint32_t *) ids[1], boxes, dec,
                           (const Ctrl *) ctrl);
        hipLaunchKernelGGL(walk_partition_kernel, dim3(nbig, parts), dim3(RTWK_BLOCK), 0, st, cur, (const uint32_t *) ids[0], (const uint32_t *) ids[1], ids[0], ids[1], boxes,
                           (const Dec *) dec, ones, zeros, (const Ctrl *) ctrl);
        hipLaunchKernelGGL(walk_emit_kernel, dim3((nbig + 63u) / 64u), dim3(64), 0, st, nbig, cur, (const uint32_t *) ids[0], (const uint32_t *) ids[1], boxes, (const Dec *) dec,
                           (const Ones *) ones, (const Zeros *) zeros, ctrl, nxt, big[nxt], capBig, small, capSmall, out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, ctrl, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (h.bad) return fail(RT_ERR_INVALID_ARGUMENT, kNonFiniteBox);
    if (h.nbig[sel] > 0u || h.nsmall > capSmall) return fail(RT_ERR_HIP, "walk tree build: the level bound was reached");
    if (h.nsmall > 0u) {
        hipLaunchKernelGGL(walk_subtree_kernel, dim3(h.nsmall), dim3(RTWK_SUB_THREADS), 0, st, (const Seg *) small, (const uint32_t *) ids[0], (const uint32_t *) ids[1], boxes,
                           out, (const Ctrl *) ctrl);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

extern "C" {

int rt_walk_tree_make_host(size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes) {
    RT_TRY(check_tree_host(n, boxes));
    if (n == 0) return RT_OK;
    return guarded("rt_walk_tree_make_host", [&]() {
        if (any_non_finite(boxes, n * 6u)) return fail(RT_ERR_INVALID_ARGUMENT, kNonFiniteBox);
        std::vector<rth::Box> ob;
        boxes_of(n, boxes, ob);
        rth::FlatTree t;
        rth::SahBuilder(ob, t).build();
        for (size_t i = 0; i < t.skip.size(); ++i) {
            if (skip) skip[i] = t.skip[i];
            if (prim) prim[i] = t.prim[i];
            if (node_boxes) for (int a = 0; a < 3; ++a) { node_boxes[i * 6 + (size_t) a * 2] = t.box[i].mn[a]; node_boxes[i * 6 + (size_t) a * 2 + 1] = t.box[i].mx[a]; }
        }
        return (int) RT_OK;
    });
}

int rt_walk_tree_make_device(int32_t device, size_t n, const void *d_boxes, void *d_skip, void *d_prim, void *d_node_boxes, void *stream) {
    RT_TRY(check_tree_device(n, d_boxes, d_skip, d_prim, d_node_boxes, nullptr));
    if (n == 0) return RT_OK;
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    return build_walk_tree(n, d_boxes, d_skip, d_prim, d_node_boxes, (hipStream_t) stream);
}

int rt_walk_tree_make(int32_t device, size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes) {
    RT_TRY(check_tree_host(n, boxes));
    if (n == 0) return RT_OK;
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    const size_t nn = (size_t) rtt::node_count(n);
    Staging sg;
    RT_TRY(sg.in({{boxes, n * 48u, SEG_IN}, {skip, nn * 4u, SEG_OUT}, {prim, nn * 4u, SEG_OUT}, {node_boxes, nn * 48u, SEG_OUT}}));
    RT_TRY(build_walk_tree(n, sg.dev[0], sg.dev[1], sg.dev[2], sg.dev[3], nullptr));
    return sg.out();
}

int rt_scene_create_gpu_trees(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                              const rt_scene_options *options, int32_t device, rt_scene **out) {
    return create_scene_on_device("rt_scene_create_gpu_trees", hittables, n_hittables, textures, n_textures, options, device, true, out);
}

} // extern "C"

// rt_scene_create_ex with BoundingBoxTree.make's tree from the device build on `device`, and (walk_tree_too) the surface-area walk tree as well
static int create_scene_on_device(const char *entry, const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                                  const rt_scene_options *options, int32_t device, bool walk_tree_too, rt_scene **out) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    int walk = -1;
    if (options && options->struct_size >= offsetof(rt_scene_options, walk_tree) + sizeof(int32_t)) walk = options->walk_tree;
    if (walk == -1) walk = g_walk_tree.load();
    if (walk != RT_WALK_TREE_SAH && walk != RT_WALK_TREE_REFERENCE) return fail(RT_ERR_INVALID_ARGUMENT, "walk_tree must be RT_WALK_TREE_SAH, RT_WALK_TREE_REFERENCE or -1");
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    return scene_from_host_records(entry, hittables, n_hittables, textures, n_textures, walk, device, walk_tree_too, out);
}
// (the device entered, the arguments checked)
static int scene_from_host_records(const char *entry, const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures, int walk,
                                   int32_t device, bool walk_tree_too, rt_scene **out, const TexelSources *sources, hipStream_t st) {
    return guarded(entry, [&]() {
        // either tree through its staged call: the boxes flattened, the arrays back into a FlatTree
        auto via = [&](bool sah, const std::vector<rth::Box> &ob, rth::FlatTree &t, std::string &msg) -> int {
            const size_t n = ob.size(), nn = (size_t) rtt::node_count(n);
            std::vector<double> flat(n * 6u), nb(nn * 6u);
            for (size_t j = 0; j < n; ++j)
                for (int a = 0; a < 3; ++a) { flat[j * 6 + (size_t) a * 2] = ob[j].mn[a]; flat[j * 6 + (size_t) a * 2 + 1] = ob[j].mx[a]; }
            t.skip.resize(nn); t.prim.resize(nn); t.box.resize(nn);
            const int rc = sah ? rt_walk_tree_make(device, n, flat.data(), t.skip.data(), t.prim.data(), nb.data())
                               : rt_tree_make(device, n, flat.data(), t.skip.data(), t.prim.data(), nb.data(), nullptr);
            if (rc != RT_OK) { msg = g_err; return rc; }
            for (size_t i = 0; i < nn; ++i)
                for (int a = 0; a < 3; ++a) { t.box[i].mn[a] = nb[i * 6 + (size_t) a * 2]; t.box[i].mx[a] = nb[i * 6 + (size_t) a * 2 + 1]; }
            t.depth = sah ? depth_of(t.skip) : rtt::depth(n);
            return RT_OK;
        };
        const rth::TreeMaker maker = [&](const std::vector<rth::Box> &ob, rth::FlatTree &t, std::string &msg) { return via(false, ob, t, msg); };
        const rth::TreeMaker walkMaker = [&](const std::vector<rth::Box> &ob, rth::FlatTree &t, std::string &msg) { return via(true, ob, t, msg); };
        std::unique_ptr<rt_scene> s(new rt_scene());
        int status = RT_OK;
        std::string msg = rth::build_scene(hittables, n_hittables, textures, n_textures, walk, s->host, status, &maker, walk_tree_too ? &walkMaker : nullptr,
                                           external_flags(sources));
        if (status != RT_OK) return fail(status, msg);
        if (sources) { // the texels go to `device` and stay there: its copy of the scene is installed now, the host's blob is fetched when wanted
            unsigned char *placed = nullptr;
            RT_TRY(place_texels(s->host, textures, n_textures, *sources, st, &placed));
            if (placed) {
                std::lock_guard<std::mutex> lock(s->mu);
                DeviceScene *ds = nullptr;
                const int rc = device_scene_locked(s.get(), device, &ds, placed);
                if (rc != RT_OK) { (void) hipFree(placed); return rc; }
                s->texelsOnHost = false;
                s->texDevice = device;
                s->mirrored.store(false, std::memory_order_release);
            }
        }
        *out = s.release();
        return (int) RT_OK;
    });
}

// ------------------------------------------------------------------------------------------------------------
// Scene.make from hittables in device memory (rt_scene_plan.h, rt_scene_kernels.h; DESIGN.md "Scene.make on the device")
// ------------------------------------------------------------------------------------------------------------
static_assert(RTS_LEAF == RTD_LEAF && RTS_PEND_MARK == RTD_PEND_MARK && RTS_PEND_WIDE == RTD_PEND_WIDE && RTS_KIND_SPHERE == RTD_KIND_SPHERE &&
              RTS_KIND_PLANE == RTD_KIND_PLANE && RTS_MAX_BOUNDED == RTT_MAX_BOXES, "rt_scene_plan.h restates rt_device.h");
static_assert(sizeof(rts::Offsets) >= 11 * 4 && offsetof(rtd::SceneOffsets, bmax) == 11 * 4, "rts::Offsets' first eleven words are SceneOffsets'");

namespace {

// Stream-ordered scratch of one build: every block is freed on the stream by whichever path leaves.
struct StreamScratch {
    hipStream_t st = nullptr;
    std::vector<void *> blocks;
    ~StreamScratch() { for (void *q : blocks) (void) hipFreeAsync(q, st); }
    template <class T> int get(T **out, size_t count) {
        void *q = nullptr;
        blocks.reserve(blocks.size() + 1);
        HIP_TRY(hipMallocAsync(&q, count ? count * sizeof(T) : 16, st));
        blocks.push_back(q);
        *out = (T *) q;
        return RT_OK;
    }
};
struct DeviceBlock { // hipMalloc'd memory that belongs to the scene once the build has succeeded
    unsigned char *p = nullptr;
    ~DeviceBlock() { if (p) (void) hipFree(p); }
    unsigned char *release() { unsigned char *q = p; p = nullptr; return q; }
};

} // namespace

static rtsk::Ctrl fresh_ctrl() {
    rtsk::Ctrl c{};
    c.err = ~0ull;
    const float tiny = 1e-30f;
    memcpy(&c.bmax_bits, &tiny, sizeof(tiny));
    return c;
}
static unsigned blocks_for(uint64_t count, unsigned per) { return (unsigned) ((count + per - 1u) / per); }
// a[0 .. m) scanned into out (which may be a); sums: m / RTSK_TILE + 2 words.  sums[tiles] ends as the sum of all.
static void enqueue_scan(const uint32_t *a, uint32_t m, uint32_t *out, bool inclusive, uint32_t *sums, hipStream_t st) {
    const unsigned tiles = blocks_for(m, RTSK_TILE);
    hipLaunchKernelGGL(rtsk::scan_sums_kernel, dim3(tiles), dim3(RTSK_BLOCK), 0, st, a, m, sums);
    hipLaunchKernelGGL(rtsk::scan_top_kernel, dim3(1), dim3(RTSK_BLOCK), 0, st, sums, tiles);
    hipLaunchKernelGGL(rtsk::scan_apply_kernel, dim3(tiles), dim3(RTSK_BLOCK), 0, st, a, m, (const uint32_t *) sums, out, inclusive ? 1 : 0);
}

// Stages 3 and 4 on `st` (the device current): the image of a pre-order skip tree of nn nodes (boxes: nn * 6 doubles in the ABI's form) and of
// the object table, into `image` (ro.image_bytes).  ctrl is a fresh Ctrl on the device; it ends with bmax, the radii and the largest depth,
// which the caller reads.  Waits for the stream once, for the largest depth (which says how many passes the order by depth needs).
static int encode_on_device(uint32_t nn, uint32_t nb, uint32_t nobj, uint64_t n_hittables, const rt_hittable *d_h, const int32_t *d_skip, const int32_t *d_prim,
                            const double *d_box, const int32_t *d_o2o, const rts::Offsets &ro, unsigned char *image, rtsk::Ctrl *ctrl, hipStream_t st,
                            StreamScratch &sc, uint32_t digit_bits = 8u) {
    HIP_TRY(hipMemsetAsync(image, 0, (size_t) ro.image_bytes, st));
    if (nn > 0u) {
        const unsigned tiles = blocks_for(nn, RTSK_TILE), per = blocks_for(nn, RTSK_BLOCK);
        const uint32_t hist_words = (uint32_t) RTSK_RADIX * tiles;
        uint32_t *key[2], *idx[2], *hist, *sums, *place;
        RT_TRY(sc.get(&key[0], (size_t) nn + 1u));
        RT_TRY(sc.get(&key[1], nn));
        RT_TRY(sc.get(&idx[0], nn));
        RT_TRY(sc.get(&idx[1], nn));
        RT_TRY(sc.get(&hist, hist_words));
        RT_TRY(sc.get(&sums, (size_t) std::max(hist_words, nn) / RTSK_TILE + 2u));
        RT_TRY(sc.get(&place, (size_t) nn + 1u));
        HIP_TRY(hipMemsetAsync(key[0], 0, ((size_t) nn + 1u) * 4u, st));
        hipLaunchKernelGGL(rtsk::scene_diff_kernel, dim3(per), dim3(RTSK_BLOCK), 0, st, nn, d_skip, d_prim, key[0]);
        enqueue_scan(key[0], nn, key[0], true, sums, st); // the depth of every node
        uint32_t maxDepth = 0;
        int cur = 0;
        const uint32_t mask = (1u << digit_bits) - 1u;
        for (uint32_t shift = 0; shift < 32u; shift += digit_bits) {
            if (shift > 0u && (maxDepth >> shift) == 0u) break;
            hipLaunchKernelGGL(rtsk::sort_hist_kernel, dim3(tiles), dim3(RTSK_BLOCK), 0, st, (const uint32_t *) key[cur], nn, shift, mask, hist, tiles,
                               shift == 0u ? &ctrl->max_depth : (uint32_t *) nullptr);
            enqueue_scan(hist, hist_words, hist, false, sums, st);
            hipLaunchKernelGGL(rtsk::sort_scatter_kernel, dim3(tiles), dim3(RTSK_BLOCK), 0, st, (const uint32_t *) key[cur],
                               shift == 0u ? (const uint32_t *) nullptr : (const uint32_t *) idx[cur], nn, shift, mask, (const uint32_t *) hist, tiles, key[cur ^ 1], idx[cur ^ 1]);
            cur ^= 1;
            if (shift == 0u) {
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(&maxDepth, &ctrl->max_depth, sizeof(maxDepth), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
        }
        hipLaunchKernelGGL(rtsk::scene_place_kernel, dim3(blocks_for((uint64_t) nn + 1u, RTSK_BLOCK)), dim3(RTSK_BLOCK), 0, st, nn, (const uint32_t *) idx[cur], place);
        hipLaunchKernelGGL(rtsk::scene_nodes_kernel, dim3(per), dim3(RTSK_BLOCK), 0, st, nn, (uint64_t) nobj, d_skip, d_prim, d_box, (const uint32_t *) place,
                           image + ro.node, image + ro.node32, ctrl);
    }
    if (nobj > 0u)
        hipLaunchKernelGGL(rtsk::scene_objects_kernel, dim3(blocks_for(nobj, RTSK_BLOCK)), dim3(RTSK_BLOCK), 0, st, nobj, nb, n_hittables, d_h, d_o2o, image + ro.geo,
                           image + ro.meta, image + ro.mat, ctrl);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
// SceneOffsets from the plan's offsets and what the encoder's Ctrl ended with
static rtd::SceneOffsets scene_offsets(const rts::Offsets &ro, const rtsk::Ctrl &c) {
    rtd::SceneOffsets off{};
    off.node = ro.node; off.geo = ro.geo; off.meta = ro.meta; off.node32 = ro.node32; off.mat = ro.mat; off.total = ro.total;
    off.lds_total = ro.lds_total; off.lds32_total = ro.lds32_total;
    off.n_nodes = ro.n_nodes; off.n_bounded = ro.n_bounded; off.n_unbounded = ro.n_unbounded;
    memcpy(&off.bmax, &c.bmax_bits, sizeof(float));
    double rmax = 0.0;
    memcpy(&rmax, &c.rmax_key, sizeof(double));
    off.box_implied = rts::box_implied(off.bmax, c.bad_radius == 0u, rmax);
    return off;
}
static int upload(unsigned char **out, const void *src, size_t bytes) {
    HIP_TRY(hipMalloc((void **) out, bytes));
    HIP_TRY(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

static int fetch_hittables_locked(rt_scene *s);
static int ensure_host_mirror_locked(rt_scene *s) {
    if (s->mirrored.load(std::memory_order_acquire)) return RT_OK;
    return guarded("host mirror of a scene made on the device", [&]() -> int {
        RT_TRY(fetch_hittables_locked(s));
        if (!s->texelsOnHost) { // the texels: placed on texDevice by a rt_scene_create_*textures call or by rt_scene_set_texels_device
            rth::HostScene &h = s->host;
            DeviceGuard guard;
            RT_TRY(guard.enter(s->texDevice));
            const DeviceScene &ds = s->dev.at(s->texDevice);
            h.texelBlob.resize((size_t) h.texelBytes);
            HIP_TRY(hipDeviceSynchronize()); // (a replacement enqueued on a stream of the caller's)
            if (h.texelBytes) HIP_TRY(hipMemcpy(h.texelBlob.data(), ds.texels, (size_t) h.texelBytes, hipMemcpyDeviceToHost));
            g_last_texture_plan[7] += (int64_t) h.texelBytes;
            s->texelsOnHost = true;
        }
        s->mirrored.store(true, std::memory_order_release);
        return RT_OK;
    });
}
// the hittables' half of the mirror (s->mu held; inside guarded())
static int fetch_hittables_locked(rt_scene *s) {
    if (!s->src.keep) return RT_OK;
    {
        const MirrorSource &m = s->src;
        rth::HostScene &h = s->host;
        DeviceGuard guard;
        RT_TRY(guard.enter(m.device));
        const DeviceScene &ds = s->dev.at(m.device);
        auto down = [&](void *dst, const void *src, size_t bytes) -> int {
            if (bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            return RT_OK;
        };
        auto tree = [&](const size_t at[3], rth::FlatTree &t) -> int {
            const int depth = t.depth;
            std::vector<double> flat(m.nn * 6u);
            t.skip.resize(m.nn); t.prim.resize(m.nn); t.box.resize(m.nn);
            RT_TRY(down(t.skip.data(), m.keep + at[0], m.nn * 4u));
            RT_TRY(down(t.prim.data(), m.keep + at[1], m.nn * 4u));
            RT_TRY(down(flat.data(), m.keep + at[2], m.nn * 48u));
            for (size_t i = 0; i < m.nn; ++i)
                for (int a = 0; a < 3; ++a) { t.box[i].mn[a] = flat[i * 6 + (size_t) a * 2]; t.box[i].mx[a] = flat[i * 6 + (size_t) a * 2 + 1]; }
            t.depth = depth;
            return RT_OK;
        };
        h.hittables.resize(m.n);
        RT_TRY(down(h.hittables.data(), m.keep + m.records_at, m.n * sizeof(rt_hittable)));
        RT_TRY(tree(m.tree_at, h.tree));
        if (m.walk_at[0] == m.tree_at[0]) { const int depth = h.walkTree.depth; h.walkTree = h.tree; h.walkTree.depth = depth; }
        else RT_TRY(tree(m.walk_at, h.walkTree));
        {
            std::vector<double> flat(m.nb * 6u);
            RT_TRY(down(flat.data(), m.keep + m.leaf_at, m.nb * 48u));
            h.leafBoxes.resize(m.nb);
            for (size_t j = 0; j < m.nb; ++j)
                for (int a = 0; a < 3; ++a) { h.leafBoxes[j].mn[a] = flat[j * 6 + (size_t) a * 2]; h.leafBoxes[j].mx[a] = flat[j * 6 + (size_t) a * 2 + 1]; }
        }
        h.objToOrig.resize(m.n);
        RT_TRY(down(h.objToOrig.data(), ds.obj_to_orig, m.n * 4u));
        h.origToObj.assign(m.n, -1);
        for (size_t j = 0; j < m.n; ++j) h.origToObj[(size_t) h.objToOrig[j]] = (int32_t) j;
        h.image.resize(h.off.total);
        RT_TRY(down(h.image.data(), ds.image, h.off.total));
        (void) hipFree(s->src.keep);
        s->src.keep = nullptr;
        return RT_OK;
    }
}

// rt_scene_create_device behind its argument checks, the device entered
static int scene_on_device(int32_t device, const rt_hittable *d_h, size_t n, const rt_texture *textures, size_t n_textures, int walk, hipStream_t st, rt_scene **out,
                           const TexelSources *sources = nullptr) {
    return guarded("rt_scene_create_device", [&]() -> int {
        std::unique_ptr<rt_scene> s(new rt_scene());
        rth::HostScene &h = s->host;
        {
            int status = RT_OK;
            const std::string msg = rth::build_textures(textures, n_textures, h, status, external_flags(sources));
            if (status != RT_OK) return fail(status, msg);
        }
        StreamScratch sc;
        sc.st = st;
        rtsk::Ctrl *ctrl = nullptr, c = fresh_ctrl();
        RT_TRY(sc.get(&ctrl, 1));
        HIP_TRY(hipMemcpyAsync(ctrl, &c, sizeof(c), hipMemcpyHostToDevice, st));
        // ---- stage 1: check, classify, partition, boxes ----
        const bool countable = n <= (size_t) RTS_MAX_OBJECTS;
        uint32_t *flag = nullptr, *pos = nullptr, *sums = nullptr;
        uint32_t nb32 = 0;
        if (n > 0) {
            if (countable) {
                RT_TRY(sc.get(&flag, n));
                RT_TRY(sc.get(&pos, n));
                RT_TRY(sc.get(&sums, n / RTSK_TILE + 2u));
            }
            hipLaunchKernelGGL(rtsk::scene_check_kernel, dim3(blocks_for(std::min(n, (size_t) RTS_MAX_OBJECTS), RTSK_BLOCK)), dim3(RTSK_BLOCK), 0, st, d_h, (uint64_t) n, (int64_t) n_textures, ctrl, flag);
            if (countable) {
                enqueue_scan(flag, (uint32_t) n, pos, false, sums, st);
                HIP_TRY(hipMemcpyAsync(&nb32, sums + blocks_for(n, RTSK_TILE), sizeof(nb32), hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(&c, ctrl, sizeof(c), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (c.err != ~0ull) return fail(RT_ERR_INVALID_ARGUMENT, "hittable " + std::to_string(c.err / 8u) + ": " + rts::reason_text((int) (c.err % 8u)));
        const size_t nb = nb32, nu = n - nb, nobj = n;
        if (!countable || rts::too_large(nb, nobj)) return fail(RT_ERR_UNSUPPORTED, rts::too_large_text());
        DeviceBlock o2o, image, keep, tex, texels;
        int32_t *bounded = nullptr;
        double *boxes = nullptr;
        if (n > 0) {
            HIP_TRY(hipMalloc((void **) &o2o.p, n * sizeof(int32_t)));
            RT_TRY(sc.get(&bounded, nb));
            RT_TRY(sc.get(&boxes, nb * 6u));
            hipLaunchKernelGGL(rtsk::scene_partition_kernel, dim3(blocks_for(n, RTSK_BLOCK)), dim3(RTSK_BLOCK), 0, st, d_h, (uint32_t) n, (const uint32_t *) flag,
                               (const uint32_t *) pos, (const uint32_t *) (sums + blocks_for(n, RTSK_TILE)), ctrl, bounded, boxes, (int32_t *) o2o.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&c, ctrl, sizeof(c), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        if (n == 0 || c.nan_box) {
            // The host's ground: nothing at all, or a NaN coordinate, which has no order.  The records come down and the scene is
            // rt_scene_create_gpu_trees' (slow for many records, but the same scene).
            std::vector<rt_hittable> rec(n);
            if (n) HIP_TRY(hipMemcpy(rec.data(), d_h, n * sizeof(rt_hittable), hipMemcpyDeviceToHost));
            return scene_from_host_records("rt_scene_create_device", rec.data(), n, textures, n_textures, walk, device, true, out, sources, st);
        }
        // ---- both trees, from and into device memory; the ranks between them ----
        const size_t nn = (size_t) rtt::node_count(nb);
        const int walkKind = (walk == RT_WALK_TREE_REFERENCE || c.non_finite || nb < 3u) ? RT_WALK_TREE_REFERENCE : RT_WALK_TREE_SAH; // (build_scene's rule)
        MirrorSource src;
        src.device = device; src.n = n; src.nb = nb; src.nn = nn;
        {
            auto up = [](size_t v) { return (v + 15u) & ~(size_t) 15u; };
            size_t at = 0;
            src.records_at = at; at += up(n * sizeof(rt_hittable));
            for (int k = 0; k < 3; ++k) { src.tree_at[k] = at; at += up(nn * (k == 2 ? 48u : 4u)); }
            for (int k = 0; k < 3; ++k) {
                if (walkKind == RT_WALK_TREE_SAH) { src.walk_at[k] = at; at += up(nn * (k == 2 ? 48u : 4u)); }
                else src.walk_at[k] = src.tree_at[k];
            }
            src.leaf_at = at; at += up(nb * 48u);
            HIP_TRY(hipMalloc((void **) &keep.p, at));
        }
        HIP_TRY(hipMemcpyAsync(keep.p + src.records_at, d_h, n * sizeof(rt_hittable), hipMemcpyDeviceToDevice, st));
        int32_t *tskip = (int32_t *) (keep.p + src.tree_at[0]), *tprim = (int32_t *) (keep.p + src.tree_at[1]);
        int32_t *wskip = (int32_t *) (keep.p + src.walk_at[0]), *wprim = (int32_t *) (keep.p + src.walk_at[1]);
        double *tbox = (double *) (keep.p + src.tree_at[2]), *wbox = (double *) (keep.p + src.walk_at[2]), *leaf = (double *) (keep.p + src.leaf_at);
        int32_t *order = nullptr, *rankOf = nullptr;
        RT_TRY(sc.get(&order, nb));
        RT_TRY(sc.get(&rankOf, nb));
        if (nb >= 3u) {
            FormatPending fp;
            RT_TRY(enqueue_tree(nb, boxes, tskip, tprim, tbox, order, st, fp));
        } else if (nb > 0u) // fewer than 3 spheres: the tree is trivial and is written directly
            hipLaunchKernelGGL(rtsk::scene_small_tree_kernel, dim3(1), dim3(64), 0, st, (uint32_t) nb, (const double *) boxes, tskip, tprim, tbox, order);
        if (nb > 0u) hipLaunchKernelGGL(rtsk::scene_rank_kernel, dim3(blocks_for(nb, RTSK_BLOCK)), dim3(RTSK_BLOCK), 0, st, (uint32_t) nb, (const int32_t *) order, (const int32_t *) bounded,
                           (const double *) boxes, (int32_t *) o2o.p, rankOf, leaf);
        if (nb > 0u) hipLaunchKernelGGL(rtsk::scene_prim_kernel, dim3(blocks_for(nn, RTSK_BLOCK)), dim3(RTSK_BLOCK), 0, st, (uint32_t) nn, tprim, (const int32_t *) rankOf);
        HIP_TRY(hipGetLastError());
        if (walkKind == RT_WALK_TREE_SAH) RT_TRY(build_walk_tree(nb, leaf, wskip, wprim, wbox, st));
        // ---- the image ----
        const rts::Offsets ro = rts::offsets(nn, nb, nu);
        HIP_TRY(hipMalloc((void **) &image.p, (size_t) ro.image_bytes));
        RT_TRY(encode_on_device((uint32_t) nn, (uint32_t) nb, (uint32_t) nobj, n, d_h, wskip, wprim, wbox, (const int32_t *) o2o.p, ro, image.p, ctrl, st, sc));
        HIP_TRY(hipMemcpyAsync(&c, ctrl, sizeof(c), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // ---- what the host keeps: O(1) and the textures ----
        h.off = scene_offsets(ro, c);
        h.nBounded = nb; h.nUnbounded = nu;
        h.walkKind = walkKind;
        h.tree.depth = rtt::depth(nb);
        h.walkTree.depth = walkKind == RT_WALK_TREE_SAH ? (int) c.max_depth + 1 : h.tree.depth;
        DeviceScene d;
        if (!h.texRecs.empty()) RT_TRY(upload(&tex.p, h.texRecs.data(), h.texRecs.size() * sizeof(TexRec)));
        if (sources) RT_TRY(place_texels(h, textures, n_textures, *sources, st, &texels.p));
        else if (!h.texelBlob.empty()) RT_TRY(upload(&texels.p, h.texelBlob.data(), h.texelBlob.size()));
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        d.cu_count = prop.multiProcessorCount;
        d.image = image.p; d.tex = (TexRec *) tex.p; d.texels = texels.p; d.obj_to_orig = (int32_t *) o2o.p;
        s->dev.emplace(device, d);
        (void) image.release(); (void) tex.release(); (void) texels.release(); (void) o2o.release();
        src.keep = keep.release();
        s->src = src;
        if (sources && h.texelBytes) { s->texelsOnHost = false; s->texDevice = device; }
        s->mirrored.store(false, std::memory_order_release);
        *out = s.release();
        return (int) RT_OK;
    });
}

extern "C" {

int rt_scene_create_device(int32_t device, const void *d_hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                           const rt_scene_options *options, void *stream, rt_scene **out) {
    if (n_hittables > 0 && !d_hittables) return fail(RT_ERR_INVALID_ARGUMENT, "d_hittables is NULL");
    if (n_textures > 0 && !textures) return fail(RT_ERR_INVALID_ARGUMENT, "textures is NULL");
    if ((uintptr_t) d_hittables % 8u) return fail(RT_ERR_INVALID_ARGUMENT, "d_hittables is not 8-byte aligned");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    int walk = -1;
    if (options && options->struct_size >= offsetof(rt_scene_options, walk_tree) + sizeof(int32_t)) walk = options->walk_tree;
    if (walk == -1) walk = g_walk_tree.load();
    if (walk != RT_WALK_TREE_SAH && walk != RT_WALK_TREE_REFERENCE) return fail(RT_ERR_INVALID_ARGUMENT, "walk_tree must be RT_WALK_TREE_SAH, RT_WALK_TREE_REFERENCE or -1");
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    return scene_on_device(device, (const rt_hittable *) d_hittables, n_hittables, textures, n_textures, walk, (hipStream_t) stream, out);
}

int rt_dev_scene_has_host_mirror(const rt_scene *scene) { return scene && scene->mirrored.load(std::memory_order_acquire) ? 1 : 0; }

int rt_dev_scene_image(const rt_scene *scene, int32_t device, void *out, size_t cap, size_t *bytes, uint32_t offsets[16]) {
    if (!scene || !bytes) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    return guarded("rt_dev_scene_image", [&]() -> int {
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        DeviceScene *ds = nullptr;
        RT_TRY(device_scene(const_cast<rt_scene *>(scene), device, &ds));
        const rtd::SceneOffsets off = scene->host.off;
        *bytes = off.total;
        if (offsets) { memset(offsets, 0, 16 * sizeof(uint32_t)); memcpy(offsets, &off, sizeof(off)); }
        if (!out) return RT_OK;
        if (cap < off.total) return fail(RT_ERR_INVALID_ARGUMENT, "out is smaller than the image");
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, ds->image, off.total, hipMemcpyDeviceToHost));
        return RT_OK;
    });
}
static_assert(sizeof(rtd::SceneOffsets) <= 16 * sizeof(uint32_t), "rt_dev_scene_image's offsets");

int rt_dev_encode_image(int32_t device, const rt_scene *host_made, void *out, size_t cap, size_t *bytes) {
    return rt_dev_encode_image_radix(device, host_made, 8, out, cap, bytes);
}
int rt_dev_encode_image_radix(int32_t device, const rt_scene *host_made, int32_t digit_bits, void *out, size_t cap, size_t *bytes) {
    if (!host_made || !bytes) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (digit_bits < 1 || digit_bits > 8) return fail(RT_ERR_INVALID_ARGUMENT, "digit_bits must be 1 .. 8");
    return guarded("rt_dev_encode_image", [&]() -> int {
        RT_TRY(ensure_host_mirror(host_made));
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        std::lock_guard<std::mutex> lock(const_cast<rt_scene *>(host_made)->mu); // (rt_scene_tune* changes the walk tree under it)
        const rth::HostScene &h = host_made->host;
        const rth::FlatTree &wt = h.walkTree;
        const size_t nn = wt.skip.size(), nb = h.nBounded, nu = h.nUnbounded, nobj = nb + nu, n = h.hittables.size();
        const rts::Offsets ro = rts::offsets(nn, nb, nu);
        *bytes = ro.total;
        if (!out) return RT_OK;
        if (cap < ro.total) return fail(RT_ERR_INVALID_ARGUMENT, "out is smaller than the image");
        std::vector<double> flat(nn * 6u);
        for (size_t i = 0; i < nn; ++i)
            for (int a = 0; a < 3; ++a) { flat[i * 6 + (size_t) a * 2] = wt.box[i].mn[a]; flat[i * 6 + (size_t) a * 2 + 1] = wt.box[i].mx[a]; }
        const rtsk::Ctrl c = fresh_ctrl();
        std::vector<unsigned char> img((size_t) ro.image_bytes);
        Staging sg;
        RT_TRY(sg.in({{h.hittables.data(), n * sizeof(rt_hittable), SEG_IN}, {wt.skip.data(), nn * 4u, SEG_IN}, {wt.prim.data(), nn * 4u, SEG_IN},
                      {flat.data(), nn * 48u, SEG_IN}, {h.objToOrig.data(), nobj * 4u, SEG_IN}, {&c, sizeof(c), SEG_IN}, {img.data(), img.size(), SEG_OUT}}));
        StreamScratch sc;
        RT_TRY(encode_on_device((uint32_t) nn, (uint32_t) nb, (uint32_t) nobj, n, (const rt_hittable *) sg.dev[0], (const int32_t *) sg.dev[1], (const int32_t *) sg.dev[2],
                                (const double *) sg.dev[3], (const int32_t *) sg.dev[4], ro, (unsigned char *) sg.dev[6], (rtsk::Ctrl *) sg.dev[5], nullptr, sc,
                                (uint32_t) digit_bits));
        HIP_TRY(hipStreamSynchronize(nullptr));
        RT_TRY(sg.out());
        memcpy(out, img.data(), ro.total);
        return RT_OK;
    });
}

} // extern "C"

// ============================================================================================================
// LoadImage.fromResource: baseline JPEG (rt_jpeg.h; the kernels: rt_jpeg_kernels.h)
// ============================================================================================================
static_assert(rtj::INVALID == RT_ERR_INVALID_ARGUMENT && rtj::UNSUPPORTED == RT_ERR_UNSUPPORTED && rtj::OK == RT_OK, "rt_jpeg.h restates the status codes");
static_assert(rtj::GREY == RT_JPEG_GREY && rtj::S444 == RT_JPEG_444 && rtj::S422 == RT_JPEG_422 && rtj::S420 == RT_JPEG_420, "rt_jpeg.h restates the sampling classes");
static thread_local int64_t g_last_jpeg_plan[8] = {0};

static int check_jpeg(const uint8_t *data, size_t n, const void *out) {
    if (!data) return fail(RT_ERR_INVALID_ARGUMENT, "data is NULL");
    if (n == 0) return fail(RT_ERR_INVALID_ARGUMENT, "jpeg: no SOI marker at byte 0");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "the output is NULL");
    return RT_OK;
}
static int parse_jpeg(const uint8_t *data, size_t n, rtj::Parsed &ps) {
    std::string err;
    const int rc = rtj::parse(data, n, ps, err);
    return rc == RT_OK ? RT_OK : fail(rc, err);
}

// The decode of `ps` on `st` (the device current) into d_rgb, in subsequences of S bytes.  plan: rt_dev_last_jpeg_plan's words.  With
// `wait` it synchronises and reports what the device found in the entropy-coded data.
static int jpeg_on_device(const uint8_t *data, const rtj::Parsed &ps, uint32_t S, uint8_t *d_rgb, hipStream_t st, bool wait, int64_t plan[8]) {
    const rtj::Frame &f = ps.f;
    const uint32_t n_raw = (uint32_t) ps.ecs_raw, n_clean = ps.n_clean, nb = ps.n_rst, nbits = n_clean * 8u, ns = (n_clean + S - 1u) / S;
    plan[0] = S; plan[1] = ns; plan[2] = plan[3] = plan[4] = 0; plan[5] = nb; plan[6] = plan[7] = 0;
    if (ns == 0u) return wait ? fail(RT_ERR_INVALID_ARGUMENT, rtj::stream_error(rtj::BAD_COUNT)) : RT_OK; // no entropy-coded byte: nothing to launch
    StreamScratch sc;
    sc.st = st;
    uint8_t *raw, *clean, *planes;
    uint32_t *keep, *rst, *sums, *bounds, *count, *first, *dcarr, *head_words;
    rtj::Tables *tables;
    rtj::State *start, *end[2];
    int16_t *coefs;
    const uint32_t scan_most = std::max(std::max(n_raw, ns), f.total);
    RT_TRY(sc.get(&raw, n_raw));
    RT_TRY(sc.get(&clean, (size_t) n_clean + 8u));
    RT_TRY(sc.get(&keep, n_raw));
    RT_TRY(sc.get(&rst, n_raw));
    RT_TRY(sc.get(&sums, (size_t) scan_most / RTSK_TILE + 2u));
    RT_TRY(sc.get(&bounds, (size_t) nb + 1u));
    RT_TRY(sc.get(&tables, 1));
    RT_TRY(sc.get(&start, ns));
    RT_TRY(sc.get(&end[0], ns));
    RT_TRY(sc.get(&end[1], ns));
    RT_TRY(sc.get(&count, ns));
    RT_TRY(sc.get(&first, ns));
    RT_TRY(sc.get(&head_words, sizeof(rtjk::Head) / 4u + (size_t) ns));
    RT_TRY(sc.get(&coefs, (size_t) f.total * 64u));
    RT_TRY(sc.get(&dcarr, f.total));
    RT_TRY(sc.get(&planes, (size_t) f.plane_bytes));
    rtjk::Head *head = (rtjk::Head *) head_words;
    uint32_t *ran = head_words + sizeof(rtjk::Head) / 4u;
    HIP_TRY(hipMemcpyAsync(raw, data + ps.ecs_at, n_raw, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(tables, &ps.t, sizeof(rtj::Tables), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(head_words, 0, sizeof(rtjk::Head) + (size_t) ns * 4u, st));
    HIP_TRY(hipMemsetAsync(coefs, 0, (size_t) f.total * 128u, st));
    // (a) clean
    hipLaunchKernelGGL(rtjk::clean_flags_kernel, dim3(blocks_for(n_raw, RTJK_BLOCK)), dim3(RTJK_BLOCK), 0, st, (const uint8_t *) raw, n_raw, keep, rst);
    enqueue_scan(keep, n_raw, keep, false, sums, st);
    enqueue_scan(rst, n_raw, rst, false, sums, st);
    hipLaunchKernelGGL(rtjk::clean_scatter_kernel, dim3(blocks_for(n_raw, RTJK_BLOCK)), dim3(RTJK_BLOCK), 0, st, (const uint8_t *) raw, n_raw, (const uint32_t *) keep,
                       (const uint32_t *) rst, clean, n_clean, bounds, nb);
    HIP_TRY(hipGetLastError());
    // (b) synchronise: after round r the first r + 1 subsequences are true, so round ns - 1 is the last one there can be
    const unsigned sync_grid = blocks_for(ns, RTJK_SYNC_BLOCK);
    uint32_t rounds = 0;
    uint64_t decodes = 0;
    for (uint32_t r0 = 0; r0 < ns;) {
        const uint32_t batch = std::min<uint32_t>(RTJK_ROUND_BATCH, ns - r0);
        for (uint32_t r = r0; r < r0 + batch; ++r)
            hipLaunchKernelGGL(rtjk::sync_kernel, dim3(sync_grid), dim3(RTJK_SYNC_BLOCK), 0, st, f, (const rtj::Tables *) tables, (const uint8_t *) clean, nbits,
                               (const uint32_t *) bounds, nb, S, ns, r, start, (const rtj::State *) end[(r + 1u) & 1u], end[r & 1u], count, ran);
        HIP_TRY(hipGetLastError());
        uint32_t got[RTJK_ROUND_BATCH] = {0};
        HIP_TRY(hipMemcpyAsync(got, ran + r0, batch * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool done = false;
        for (uint32_t k = 0; k < batch && !done; ++k) {
            if (got[k] == 0u) done = true;
            else { ++rounds; decodes += got[k]; }
        }
        if (done) break;
        r0 += batch;
    }
    plan[2] = rounds; plan[3] = (int64_t) decodes;
    // (c) place, (d) DC, (e) samples, (f) colours
    enqueue_scan(count, ns, first, false, sums, st);
    hipLaunchKernelGGL(rtjk::place_kernel, dim3(sync_grid), dim3(RTJK_SYNC_BLOCK), 0, st, f, (const rtj::Tables *) tables, (const uint8_t *) clean, nbits,
                       (const uint32_t *) bounds, nb, S, ns, (const rtj::State *) start, (const uint32_t *) first, (const uint32_t *) (sums + blocks_for(ns, RTSK_TILE)),
                       coefs, head);
    hipLaunchKernelGGL(rtjk::dc_gather_kernel, dim3(blocks_for(f.total, RTJK_BLOCK)), dim3(RTJK_BLOCK), 0, st, f, (const int16_t *) coefs, dcarr, (const rtjk::Head *) head);
    uint32_t *sums2;
    RT_TRY(sc.get(&sums2, (size_t) f.total / RTSK_TILE + 2u)); // (place_kernel still reads the sum of all in `sums`)
    enqueue_scan(dcarr, f.total, dcarr, true, sums2, st);
    hipLaunchKernelGGL(rtjk::idct_kernel, dim3(blocks_for(f.total, RTJK_BLOCK)), dim3(RTJK_BLOCK), 0, st, f, (const int16_t *) coefs, (const uint32_t *) dcarr, planes,
                       (const rtjk::Head *) head);
    hipLaunchKernelGGL(rtjk::colour_kernel, dim3(blocks_for((uint64_t) f.W * f.H, RTJK_BLOCK)), dim3(RTJK_BLOCK), 0, st, f, (const uint8_t *) planes, d_rgb,
                       (const rtjk::Head *) head);
    HIP_TRY(hipGetLastError());
    plan[4] = f.total;
    if (!wait) return RT_OK;
    rtjk::Head found{};
    uint32_t blocks = 0;
    HIP_TRY(hipMemcpyAsync(&found, head, sizeof(found), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&blocks, sums + blocks_for(ns, RTSK_TILE), sizeof(blocks), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    plan[4] = blocks;
    return found.flags ? fail(RT_ERR_INVALID_ARGUMENT, rtj::stream_error(found.flags)) : RT_OK;
}

static int decode_jpeg_device(int32_t device, const uint8_t *data, size_t n, int32_t subsequence_bytes, void *d_rgb, size_t capacity, hipStream_t st, bool wait,
                              rt_jpeg_stats *stats) {
    RT_TRY(check_jpeg(data, n, d_rgb));
    if (subsequence_bytes != 0 && subsequence_bytes < RTJ_MIN_SUBSEQUENCE) return fail(RT_ERR_INVALID_ARGUMENT, "subsequence_bytes must be at least 4");
    return guarded("rt_decode_jpeg_device", [&]() -> int {
        const auto t0 = std::chrono::steady_clock::now();
        rtj::Parsed ps;
        RT_TRY(parse_jpeg(data, n, ps));
        const size_t need = (size_t) ps.f.W * ps.f.H * 3u;
        if (capacity < need) return fail(RT_ERR_INVALID_ARGUMENT, "jpeg: capacity " + std::to_string(capacity) + " below the " + std::to_string(need) + " bytes of the bitmap");
        if (rtj::marker_flags(ps)) return fail(RT_ERR_INVALID_ARGUMENT, rtj::stream_error(rtj::marker_flags(ps))); // known on the host: before any device call
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        int64_t *plan = g_last_jpeg_plan;
        const int rc = jpeg_on_device(data, ps, subsequence_bytes ? (uint32_t) subsequence_bytes : (uint32_t) RTJ_DEFAULT_SUBSEQUENCE, (uint8_t *) d_rgb, st, wait, plan);
        if (stats && stats->struct_size >= sizeof(rt_jpeg_stats)) {
            stats->subsequence_bytes = (int32_t) plan[0]; stats->subsequences = plan[1]; stats->rounds = plan[2]; stats->decodes = plan[3];
            stats->blocks = plan[4]; stats->boundaries = plan[5];
            stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        return rc;
    });
}

extern "C" {

int rt_jpeg_get_info(const uint8_t *data, size_t n, rt_jpeg_info *out) {
    RT_TRY(check_jpeg(data, n, out));
    if (out->struct_size < sizeof(rt_jpeg_info)) return fail(RT_ERR_INVALID_ARGUMENT, "out->struct_size is smaller than rt_jpeg_info");
    return guarded("rt_jpeg_get_info", [&]() -> int {
        rtj::Parsed ps;
        RT_TRY(parse_jpeg(data, n, ps));
        out->width = (int32_t) ps.f.W; out->height = (int32_t) ps.f.H; out->components = (int32_t) ps.f.ncomp; out->sampling = (int32_t) ps.f.cls;
        out->restart_interval = (int32_t) ps.f.Ri; out->entropy_bytes = (int64_t) ps.ecs_raw;
        return RT_OK;
    });
}

int rt_decode_jpeg(const uint8_t *data, size_t n, uint8_t *rgb, size_t capacity) {
    RT_TRY(check_jpeg(data, n, rgb));
    return guarded("rt_decode_jpeg", [&]() -> int {
        std::string err;
        const int rc = rtj::decode_host(data, n, rgb, capacity, 0u, nullptr, err);
        return rc == RT_OK ? RT_OK : fail(rc, err);
    });
}

int rt_decode_jpeg_device(int32_t device, const uint8_t *data, size_t n, void *d_rgb, size_t capacity, void *stream, rt_jpeg_stats *stats) {
    if (stats && stats->struct_size < sizeof(rt_jpeg_stats)) return fail(RT_ERR_INVALID_ARGUMENT, "stats->struct_size is smaller than rt_jpeg_stats");
    return decode_jpeg_device(device, data, n, 0, d_rgb, capacity, (hipStream_t) stream, stats != nullptr, stats);
}

int rt_dev_decode_jpeg(int32_t device, const uint8_t *data, size_t n, int32_t subsequence_bytes, void *d_rgb, size_t capacity) {
    return decode_jpeg_device(device, data, n, subsequence_bytes, d_rgb, capacity, nullptr, true, nullptr);
}

int rt_dev_last_jpeg_plan(int64_t out[8]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = g_last_jpeg_plan[i];
    return RT_OK;
}

} // extern "C"

// ============================================================================================================
// Image textures from device memory (rt_texture_plan.h, rt_texture_kernels.h; DESIGN.md "Textures from device memory")
// ============================================================================================================
static_assert(RTX_TOP_FIRST == RT_TEXELS_TOP_FIRST && RTX_MAX_IMAGES == RTD_MAX_TEXTURES, "rt_texture_plan.h restates the ABI");

struct TexelSources {
    const rt_texels_source *src = nullptr;     // n_textures entries
    std::vector<uint8_t> external;             // per record: its texels are not rt_texture.texels
    std::vector<std::unique_ptr<rtj::Parsed>> jpeg; // per record: the parsed header of a RT_TEXELS_JPEG source
};
static const uint8_t *external_flags(const TexelSources *sources) { return sources ? sources->external.data() : nullptr; }

// The argument checks of `sources`, before any device call.
static int check_sources(const rt_texture *textures, size_t n_textures, const rt_texels_source *sources, TexelSources &ts) {
    ts.src = sources;
    ts.external.assign(n_textures ? n_textures : 1, 0);
    ts.jpeg.resize(n_textures);
    for (size_t i = 0; i < n_textures; ++i) {
        const rt_texels_source &q = sources[i];
        const std::string who = "source " + std::to_string(i) + ": ";
        if (q.struct_size != sizeof(rt_texels_source)) return fail(RT_ERR_INVALID_ARGUMENT, who + "struct_size is not sizeof(rt_texels_source)");
        if (q.kind > RT_TEXELS_JPEG) return fail(RT_ERR_INVALID_ARGUMENT, who + "unknown kind");
        if (q.flags & ~RT_TEXELS_TOP_FIRST) return fail(RT_ERR_INVALID_ARGUMENT, who + "unknown flag bit");
        if (q.kind == RT_TEXELS_RECORD) continue;
        const rt_texture &t = textures[i];
        if (t.kind == RT_TEXTURE_PROGRAM) return fail(RT_ERR_INVALID_ARGUMENT, who + "a program's bytes come from the record (RT_TEXELS_RECORD)");
        if (t.kind != RT_TEXTURE_IMAGE) return fail(RT_ERR_INVALID_ARGUMENT, who + "texels for a texture that is not an image");
        if (!q.data) return fail(RT_ERR_INVALID_ARGUMENT, who + "data is NULL");
        if (q.kind == RT_TEXELS_DEVICE && t.width > 0 && t.height > 0 && q.bytes < rtt::image_bytes(t.width, t.height))
            return fail(RT_ERR_INVALID_ARGUMENT, who + "bytes is below width * height * 3");
        ts.external[i] = 1;
    }
    return RT_OK;
}
// The JPEG sources' headers, on the host: rt_decode_jpeg's refusals, and the file's size against the record's.
static int parse_sources(const rt_texture *textures, size_t n_textures, TexelSources &ts) {
    for (size_t i = 0; i < n_textures; ++i) {
        const rt_texels_source &q = ts.src[i];
        if (q.kind != RT_TEXELS_JPEG) continue;
        const std::string who = "texture " + std::to_string(i) + ": ";
        if (q.bytes == 0) return fail(RT_ERR_INVALID_ARGUMENT, who + "jpeg: no SOI marker at byte 0");
        ts.jpeg[i].reset(new rtj::Parsed());
        std::string err;
        const int rc = rtj::parse((const uint8_t *) q.data, q.bytes, *ts.jpeg[i], err);
        if (rc != RT_OK) return fail(rc, who + err);
        const rtj::Frame &f = ts.jpeg[i]->f;
        if ((int64_t) f.W != (int64_t) textures[i].width || (int64_t) f.H != (int64_t) textures[i].height)
            return fail(RT_ERR_INVALID_ARGUMENT, who + "the jpeg is " + std::to_string(f.W) + " x " + std::to_string(f.H) + ", the record " +
                                                     std::to_string(textures[i].width) + " x " + std::to_string(textures[i].height));
    }
    return RT_OK;
}

// of_image_kernel over `units` 16-byte units from unit0 on.  table: device memory (n entries), or NULL with the one entry by value.
static int launch_of_image(bool aligned, const rtt::ImageEntry *table, uint32_t n, const rtt::ImageEntry &one, uint8_t *blob, uint64_t unit0, uint64_t units, hipStream_t st) {
    if (units == 0u) return RT_OK;
    const uint64_t grid = (units + RTXK_BLOCK - 1u) / RTXK_BLOCK;
    if (grid > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, "the image is too large for one launch");
    if (aligned) hipLaunchKernelGGL(rtxk::of_image_kernel<true>, dim3((unsigned) grid), dim3(RTXK_BLOCK), 0, st, table, n, one, blob, unit0, units);
    else hipLaunchKernelGGL(rtxk::of_image_kernel<false>, dim3((unsigned) grid), dim3(RTXK_BLOCK), 0, st, table, n, one, blob, unit0, units);
    HIP_TRY(hipGetLastError());
    g_last_texture_plan[5] += 1;
    return RT_OK;
}

static int place_texels(const rth::HostScene &h, const rt_texture *textures, size_t n_textures, const TexelSources &ts, hipStream_t st, unsigned char **out) {
    int64_t *plan = g_last_texture_plan;
    for (int k = 0; k < 8; ++k) plan[k] = 0;
    plan[0] = (int64_t) n_textures; plan[4] = (int64_t) h.texelBytes;
    *out = nullptr;
    DeviceBlock blob;
    StreamScratch sc;
    sc.st = st;
    if (h.texelBytes) HIP_TRY(hipMalloc((void **) &blob.p, (size_t) h.texelBytes));
    std::vector<rtt::ImageEntry> table;
    bool any = false;
    for (size_t i = 0; i < n_textures; ++i) {
        if (textures[i].kind == RT_TEXTURE_PROGRAM) { // its bytes, from the record (check_sources), zero-padded; of_image_kernel leaves the range alone
            const size_t off = h.texRecs[i].texel_off, bytes = (size_t) textures[i].width, padded = (bytes + 15u) & ~(size_t) 15u;
            HIP_TRY(hipMemcpyAsync(blob.p + off, textures[i].texels, bytes, hipMemcpyHostToDevice, st));
            if (padded > bytes) HIP_TRY(hipMemsetAsync(blob.p + off + bytes, 0, padded - bytes, st));
            plan[6] += (int64_t) bytes;
            continue;
        }
        if (textures[i].kind != RT_TEXTURE_IMAGE) continue;
        const rt_texels_source &q = ts.src[i];
        const int32_t w = textures[i].width, hgt = textures[i].height;
        const uint64_t bytes = rtt::image_bytes(w, hgt), padded = rtt::padded_bytes(w, hgt);
        rtt::ImageEntry e{};
        e.off = h.texRecs[i].texel_off; e.width = w; e.height = hgt;
        ++plan[1];
        if (q.kind == RT_TEXELS_RECORD) { // as the existing routes: the record's host texels, already img.[y]
            HIP_TRY(hipMemcpyAsync(blob.p + e.off, textures[i].texels, (size_t) bytes, hipMemcpyHostToDevice, st));
            if (padded > bytes) HIP_TRY(hipMemsetAsync(blob.p + e.off + bytes, 0, (size_t) (padded - bytes), st));
            plan[6] += (int64_t) bytes;
        } else if (q.kind == RT_TEXELS_DEVICE) {
            e.src = (const uint8_t *) q.data;
            e.flags = RTX_FROM_DEVICE | (q.flags & RT_TEXELS_TOP_FIRST ? RTX_TOP_FIRST : 0u);
            ++plan[2]; any = true;
        } else { // a JPEG: decoded by the device decoder into scratch of this stream, top first
            const rtj::Parsed &ps = *ts.jpeg[i];
            if (rtj::marker_flags(ps)) return fail(RT_ERR_INVALID_ARGUMENT, rtj::stream_error(rtj::marker_flags(ps)));
            uint8_t *bitmap = nullptr;
            RT_TRY(sc.get(&bitmap, (size_t) bytes));
            int64_t jplan[8];
            const int rc = jpeg_on_device((const uint8_t *) q.data, ps, (uint32_t) RTJ_DEFAULT_SUBSEQUENCE, bitmap, st, true, jplan);
            if (rc != RT_OK) { (void) hipStreamSynchronize(st); return rc; } // (a damaged stream: the call waits for what it enqueued, then fails)
            e.src = bitmap;
            e.flags = RTX_FROM_DEVICE | RTX_TOP_FIRST;
            ++plan[3]; any = true;
        }
        table.push_back(e);
    }
    if (any) {
        rtt::ImageEntry *d_table = nullptr;
        RT_TRY(sc.get(&d_table, table.size()));
        HIP_TRY(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(rtt::ImageEntry), hipMemcpyHostToDevice, st)); // (`table` outlives the wait below)
        RT_TRY(launch_of_image(true, d_table, (uint32_t) table.size(), rtt::ImageEntry{}, blob.p, 0u, h.texelBytes / RTX_UNIT, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *out = blob.release();
    return RT_OK;
}

// The walk_tree option of a create call (-1 / absent: the process default); false: not a creation option
static bool creation_walk(const rt_scene_options *options, int &walk) {
    walk = -1;
    if (options && options->struct_size >= offsetof(rt_scene_options, walk_tree) + sizeof(int32_t)) walk = options->walk_tree;
    if (walk == -1) walk = g_walk_tree.load();
    return walk == RT_WALK_TREE_SAH || walk == RT_WALK_TREE_REFERENCE;
}

extern "C" {

int rt_scene_create_textures(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                             const rt_texels_source *sources, const rt_scene_options *options, int32_t device, void *stream, rt_scene **out) {
    if (!sources) return rt_scene_create_gpu_trees(hittables, n_hittables, textures, n_textures, options, device, out);
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    if (n_textures > 0 && !textures) return fail(RT_ERR_INVALID_ARGUMENT, "textures is NULL");
    int walk = -1;
    if (!creation_walk(options, walk)) return fail(RT_ERR_INVALID_ARGUMENT, "walk_tree must be RT_WALK_TREE_SAH, RT_WALK_TREE_REFERENCE or -1");
    return guarded("rt_scene_create_textures", [&]() -> int {
        TexelSources ts;
        RT_TRY(check_sources(textures, n_textures, sources, ts));
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        RT_TRY(parse_sources(textures, n_textures, ts));
        return scene_from_host_records("rt_scene_create_textures", hittables, n_hittables, textures, n_textures, walk, device, true, out, &ts, (hipStream_t) stream);
    });
}

int rt_scene_create_device_textures(int32_t device, const void *d_hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                                    const rt_texels_source *sources, const rt_scene_options *options, void *stream, rt_scene **out) {
    if (!sources) return rt_scene_create_device(device, d_hittables, n_hittables, textures, n_textures, options, stream, out);
    if (n_hittables > 0 && !d_hittables) return fail(RT_ERR_INVALID_ARGUMENT, "d_hittables is NULL");
    if (n_textures > 0 && !textures) return fail(RT_ERR_INVALID_ARGUMENT, "textures is NULL");
    if ((uintptr_t) d_hittables % 8u) return fail(RT_ERR_INVALID_ARGUMENT, "d_hittables is not 8-byte aligned");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    int walk = -1;
    if (!creation_walk(options, walk)) return fail(RT_ERR_INVALID_ARGUMENT, "walk_tree must be RT_WALK_TREE_SAH, RT_WALK_TREE_REFERENCE or -1");
    return guarded("rt_scene_create_device_textures", [&]() -> int {
        TexelSources ts;
        RT_TRY(check_sources(textures, n_textures, sources, ts));
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        RT_TRY(parse_sources(textures, n_textures, ts));
        return scene_on_device(device, (const rt_hittable *) d_hittables, n_hittables, textures, n_textures, walk, (hipStream_t) stream, out, &ts);
    });
}

int rt_of_image_device(int32_t device, const void *d_bitmap, int32_t width, int32_t height, void *d_texels, size_t capacity, void *stream) {
    if (!d_bitmap || !d_texels) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width <= 0 || height <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "width and height must be positive");
    const uint64_t bytes = rtt::image_bytes(width, height);
    if ((uint64_t) capacity < bytes) return fail(RT_ERR_INVALID_ARGUMENT, "capacity is below width * height * 3");
    const uintptr_t a = (uintptr_t) d_bitmap, b = (uintptr_t) d_texels;
    if (a < b + bytes && b < a + bytes) return fail(RT_ERR_INVALID_ARGUMENT, "d_texels overlaps d_bitmap: the reversal is not done in place");
    DeviceGuard guard;
    RT_TRY(guard.enter(device));
    rtt::ImageEntry e{};
    e.src = (const uint8_t *) d_bitmap; e.width = width; e.height = height; e.flags = RTX_FROM_DEVICE | RTX_TOP_FIRST;
    return launch_of_image(false, nullptr, 1u, e, (uint8_t *) d_texels, 0u, rtt::padded_bytes(width, height) / RTX_UNIT, (hipStream_t) stream);
}

int rt_scene_set_texels_device(rt_scene *scene, int32_t texture, int32_t device, const void *d_rgb, size_t bytes, uint32_t flags, void *stream) {
    if (!scene || !d_rgb) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (flags & ~RT_TEXELS_TOP_FIRST) return fail(RT_ERR_INVALID_ARGUMENT, "unknown flag bit");
    return guarded("rt_scene_set_texels_device", [&]() -> int {
        std::lock_guard<std::mutex> lock(scene->mu);
        rth::HostScene &h = scene->host;
        if (texture < 0 || (size_t) texture >= h.texRecs.size()) return fail(RT_ERR_INVALID_ARGUMENT, "texture index out of range");
        const rtd::TexRec &r = h.texRecs[(size_t) texture];
        if (r.kind == RT_TEXTURE_PROGRAM) return fail(RT_ERR_INVALID_ARGUMENT, "texture " + std::to_string(texture) + " is a program: its bytes are fixed at creation");
        if (r.kind != RT_TEXTURE_IMAGE) return fail(RT_ERR_INVALID_ARGUMENT, "texture " + std::to_string(texture) + " is not an image");
        if ((uint64_t) bytes < rtt::image_bytes(r.width, r.height)) return fail(RT_ERR_INVALID_ARGUMENT, "bytes is below width * height * 3");
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        for (const auto &kv : scene->dev)
            if (kv.first != device) return fail(RT_ERR_UNSUPPORTED, "the scene has a copy on another device: its texels cannot be replaced");
        DeviceScene *ds = nullptr;
        RT_TRY(device_scene_locked(scene, device, &ds));
        rtt::ImageEntry e{};
        e.off = r.texel_off; e.src = (const uint8_t *) d_rgb; e.width = r.width; e.height = r.height;
        e.flags = RTX_FROM_DEVICE | (flags & RT_TEXELS_TOP_FIRST ? RTX_TOP_FIRST : 0u);
        RT_TRY(launch_of_image(true, nullptr, 1u, e, ds->texels, e.off / RTX_UNIT, rtt::padded_bytes(r.width, r.height) / RTX_UNIT, (hipStream_t) stream));
        // the host's blob is out of date from here: dropped, and fetched again when something wants it
        std::vector<uint8_t>().swap(h.texelBlob);
        scene->texelsOnHost = false;
        scene->texDevice = device;
        scene->mirrored.store(false, std::memory_order_release);
        return RT_OK;
    });
}

int rt_dev_scene_texels(const rt_scene *scene, int32_t device, void *out, size_t cap, size_t *bytes, uint32_t *texel_off) {
    if (!scene || !bytes) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    return guarded("rt_dev_scene_texels", [&]() -> int {
        DeviceGuard guard;
        RT_TRY(guard.enter(device));
        DeviceScene *ds = nullptr;
        RT_TRY(device_scene(const_cast<rt_scene *>(scene), device, &ds));
        const rth::HostScene &h = scene->host;
        *bytes = (size_t) h.texelBytes;
        if (texel_off)
            for (size_t i = 0; i < h.texRecs.size(); ++i) texel_off[i] = h.texRecs[i].kind == RT_TEXTURE_IMAGE ? h.texRecs[i].texel_off : UINT32_MAX;
        if (!out) return RT_OK;
        if (cap < h.texelBytes) return fail(RT_ERR_INVALID_ARGUMENT, "out is smaller than the texels");
        HIP_TRY(hipDeviceSynchronize());
        if (h.texelBytes) HIP_TRY(hipMemcpy(out, ds->texels, (size_t) h.texelBytes, hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_dev_last_texture_plan(int64_t out[8]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = g_last_texture_plan[i];
    return RT_OK;
}

} // extern "C"
