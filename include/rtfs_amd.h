/*
 * rtfs_amd.h -- C ABI of the MI355X-native per-pixel sampling path.
 *
 * This is the drop-in boundary for ONE hot path of Smaug123/ray-tracing-fsharp:
 *   Scene.render -> renderPixel -> traceOnce -> traceRay -> hitObject ->
 *   {BoundingBox.hits, Sphere.firstIntersection, InfinitePlane.intersection} -> Hittable.Reflection
 * (reference: RayTracing/Scene.fs:62-236).  The reference has no FFI of its own; every entry point
 * below names the reference function (file:line under /root/reference) whose role it takes, and
 * INTEGRATION.md shows the F# P/Invoke binding a maintainer would add.
 *
 * Conventions: POD only, caller-allocated outputs, int status (0 = RT_OK), no exceptions cross the
 * boundary, rt_last_error() is thread-local.  All geometry is IEEE double (Float.fs:82: `float` is
 * 64-bit); all colour is 8-bit (Pixel.fs:9-15); accumulators are int32 (Pixel.fs:78-85).
 *
 * The library is libamdhip64-only: no torch types appear here.  Device pointers are plain `void*`
 * so that any allocator (hipMalloc, torch.empty(..., device="cuda").data_ptr()) can own the memory.
 */
#ifndef RTFS_AMD_H
#define RTFS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 7 /* 5 (round 3): rt_scene_info.leaf_box_implied (was reserved), rt_dev_bbox_filter, rt_dev_pixel_candidates;
                          * 6: rt_scene_get_filter_tree; 7: rt_hit_objects(_device), rt_trace_rays(_device) */

/* ---- status codes ------------------------------------------------------------------------ */
enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = 1, /* the reference would `failwith` / throw (e.g. Program.fs:69) */
    RT_ERR_NO_DEVICE = 2,        /* no HIP device visible: the product path never falls back to a CPU */
    RT_ERR_HIP = 3,              /* a HIP runtime call failed; rt_last_error() carries hipGetErrorString */
    RT_ERR_UNSUPPORTED = 4,      /* e.g. Texture.Arbitrary closures (Texture.fs:8,24) cannot cross a C ABI */
    RT_ERR_IO = 5,
    RT_ERR_HOST = 6              /* host resources exhausted: memory (std::bad_alloc) or threads; the call changed nothing.
                                  * A new return value only -- no struct, field or symbol changed, so RT_ABI_VERSION stays 7: a
                                  * binding that treats any nonzero status as a failure needs no change. */
};

/* ---- Hittable (Hittable.fs:3-6) ------------------------------------------------------------ */
enum rt_hittable_kind {
    RT_HITTABLE_SPHERE = 0,           /* Hittable.Sphere: bounded, goes into the BoundingBoxTree */
    RT_HITTABLE_UNBOUNDED_SPHERE = 1, /* Hittable.UnboundedSphere: tested for every ray (Scene.fs:77-86) */
    RT_HITTABLE_INFINITE_PLANE = 2    /* Hittable.InfinitePlane: never in the tree (Hittable.fs:17-18) */
};

/* SphereStyle (Sphere.fs:10-37), in declaration order. */
enum rt_sphere_style {
    RT_SPHERE_LIGHT_SOURCE = 0,       /* LightSource of Texture */
    RT_SPHERE_LIGHT_SOURCE_CAP = 1,   /* LightSourceCap of Pixel */
    RT_SPHERE_PURE_REFLECTION = 2,    /* PureReflection of albedo * texture */
    RT_SPHERE_FUZZED_REFLECTION = 3,  /* FuzzedReflection of albedo * texture * fuzz * FloatProducer */
    RT_SPHERE_LAMBERT_REFLECTION = 4, /* LambertReflection of albedo * texture * FloatProducer */
    RT_SPHERE_DIELECTRIC = 5,         /* Dielectric of albedo * texture * ior * prob * FloatProducer */
    RT_SPHERE_GLASS = 6               /* Glass of albedo * texture * ior * FloatProducer */
};

/* InfinitePlaneStyle (InfinitePlane.fs:3-13), in declaration order. */
enum rt_plane_style {
    RT_PLANE_LIGHT_SOURCE = 0,
    RT_PLANE_PURE_REFLECTION = 1,
    RT_PLANE_LAMBERT_REFLECTION = 2,
    RT_PLANE_FUZZED_REFLECTION = 3
};

/*
 * One element of the `Hittable array` handed to Scene.make (Scene.fs:15).
 * Sphere.make style centre radius (Sphere.fs:325-337) / InfinitePlane.make style point normal
 * (InfinitePlane.fs:114-119).  FloatProducer arguments of the styles do not cross the boundary:
 * randomness comes from rt_render's `seed` (see DESIGN.md "Seeding").
 */
typedef struct rt_hittable {
    uint32_t kind;      /* rt_hittable_kind */
    uint32_t style;     /* rt_sphere_style or rt_plane_style, by kind */
    double   point[3];  /* sphere centre | a point on the plane */
    double   normal[3]; /* plane normal, already unitised by the caller (InfinitePlane.make takes a UnitVector); spheres: ignored */
    double   radius;    /* spheres; may be negative (Sphere.fs:321 "flipped") */
    double   albedo;    /* float<albedo>, must lie in [0,1] (Pixel.fs:143) */
    double   fuzz;      /* FuzzedReflection */
    double   ior;       /* Dielectric / Glass boundaryRefractance */
    double   prob;      /* Dielectric refraction probability */
    uint8_t  rgb[3];    /* Texture.Colour / LightSourceCap colour / plane colour */
    uint8_t  reserved;
    int32_t  texture;   /* -1: Texture.Colour rgb.  >=0: index into the rt_texture array (sphere styles with a texture only) */
} rt_hittable;

/* ---- Textures (Texture.fs:6-72): closures are enumerated ----------------------------------- */
enum rt_texture_kind {
    RT_TEXTURE_COLOUR = 0,    /* ParameterisedTexture.Colour */
    RT_TEXTURE_CHECKERED = 1, /* ParameterisedTexture.Checkered (even, odd, gridSize), Texture.fs:56-62 */
    RT_TEXTURE_IMAGE = 2,     /* ParameterisedTexture.Image rows (Texture.fs:63-67) */
    RT_TEXTURE_UV_RAMP = 3,   /* the two ParameterisedTexture.Arbitrary closures of SampleImages.fs:606-627 */
    /* 4 is not a kind and never will be: it stays RT_ERR_UNSUPPORTED, as does every number above 5 (bindings and tests use 4 and 17 as
     * stand-ins for "a closure that was not lowered"). */
    RT_TEXTURE_PROGRAM = 5    /* Texture.Arbitrary / ParameterisedTexture.Arbitrary (Texture.fs:8,24) lowered to an expression program:
                                 csrc/rt_texprog.h is the definition (encoding, check, evaluation, the byte rule); DESIGN.md
                                 "Texture programs".  `texels` points at the program's bytes (copied at creation, as texels are), `width` is
                                 their count, `height` is 1; map_centre / map_radius are read as for every root record.  The program sees
                                 U, V (interpret's x, y -- what Checkered and Image see) and the strike point.  It may be the root a
                                 hittable wears or the even / odd child of a Checkered record.  A malformed program is
                                 RT_ERR_INVALID_ARGUMENT; rt_last_error() names the record, the instruction and the reason.  On the routes
                                 that take rt_texels_source its source must be RT_TEXELS_RECORD, and rt_scene_set_texels_device refuses
                                 it (both RT_ERR_INVALID_ARGUMENT).  A scene that holds a program runs kernels of its own (built for
                                 blocks of 256 and 1024 threads: 512 and 768 run at 1024); every other scene runs what it always ran. */
};
/* rt_texprog.h's check of a program's n bytes, without a GPU: 0 = a program the scene routes accept; otherwise RT_ERR_INVALID_ARGUMENT
 * with rt_last_error() = "program: instruction K: <reason>" (unknown opcode, constant index out of range, stack underflow, stack depth
 * above 8, not exactly three results, too long, non-finite constant, byte count does not match the header). */
int rt_texture_program_check(const uint8_t *program, size_t n);

enum rt_ramp_source { RT_RAMP_CONST = 0, RT_RAMP_U = 1, RT_RAMP_V = 2 };
enum rt_walk_tree { RT_WALK_TREE_SAH = 0, RT_WALK_TREE_REFERENCE = 1, RT_WALK_TREE_TUNED = 2 /* reported after rt_scene_tune; not a creation option */ };

typedef struct rt_texture {
    uint32_t kind;          /* rt_texture_kind */
    uint8_t  rgb[3];        /* COLOUR; UV_RAMP constants */
    uint8_t  ramp_src[3];   /* UV_RAMP: per channel rt_ramp_source; U -> byte(u*255.0), V -> byte(v*255.0) (truncating) */
    uint8_t  reserved[2];
    int32_t  even, odd;     /* CHECKERED: indices into the same texture array (must be < own index) */
    double   grid_size;     /* CHECKERED */
    int32_t  width, height; /* IMAGE */
    const uint8_t *texels;  /* IMAGE: height*width*3 bytes, laid out as ParameterisedTexture.Image img.[y].[x]
                               i.e. AFTER ofImage's row reversal (Texture.fs:34); copied by rt_scene_create */
    double   map_centre[3]; /* interpret = Sphere.planeMapInverse map_radius map_centre (Sphere.fs:55-61), */
    double   map_radius;    /*   read from the texture a hittable points at (the root of a Checkered tree)  */
} rt_texture;

/* ---- Camera (Camera.fs:3-28) ----------------------------------------------------------------- */
typedef struct rt_camera {
    double  view_origin[3], view_dir[3];   /* View : Ray */
    double  xaxis_origin[3], xaxis_dir[3]; /* ViewportXAxis : Ray */
    double  yaxis_origin[3], yaxis_dir[3]; /* ViewportYAxis : Ray (only its direction is used, Scene.fs:140) */
    double  viewport_width, viewport_height, focal_length;
    int32_t samples_per_pixel;
    int32_t bounce_depth;                  /* Camera.fs:58 hard-codes 150; callers may override */
} rt_camera;

/* Camera.makeBasic samplesPerPixel focalLength aspectRatio origin viewDirection viewUp (Camera.fs:34-59;
 * Plane.makeNormalTo' Plane.fs:22-38; Plane.basis Plane.fs:82-97).  view_direction must be unit length. */
int rt_camera_make_basic(int32_t samples_per_pixel, double focal_length, double aspect_ratio,
                         const double origin[3], const double view_direction[3], const double view_up[3],
                         rt_camera *out);

/* ---- Scene (Scene.fs:5-28, BoundingBoxTree.fs:9-43) ------------------------------------------ */
typedef struct rt_scene rt_scene;

typedef struct rt_scene_info {
    int32_t n_bounded;      /* Hittable.Sphere count (leaves of the tree) */
    int32_t n_unbounded;    /* UnboundedSphere + InfinitePlane count, original order kept (Array.partition) */
    int32_t n_nodes;        /* BoundingBoxTree nodes, leaves included (2*n_bounded-1): the size of rt_scene_get_tree's arrays */
    int32_t tree_depth;     /* of BoundingBoxTree.make's tree (what rt_scene_get_tree reports) */
    int32_t n_textures;
    int32_t lds_resident;   /* 1 if the flattened scene fits the 160 KiB LDS image and the LDS kernel is used */
    int32_t walk_tree;      /* RT_WALK_TREE_*: the tree the device image holds */
    int32_t walk_tree_depth;
    int64_t scene_bytes;    /* bytes of the flattened device image (without texels) */
    int64_t texel_bytes;
    int32_t walk_tree_nodes; /* nodes of the tree the device image holds: the size of rt_scene_get_walk_tree's arrays (= n_nodes
                                until rt_scene_tune thins the tree) */
    int32_t leaf_box_implied; /* 1: the scene meets the bounds under which the timed kernel's leaf pass need not evaluate a Leaf's own
                                 BoundingBox.hits when Sphere.firstIntersection has found a hit (csrc/rt_device.h,
                                 leaf_test_object_exact: every bounded radius in (0, 100], coordinates within 1000, r_max * extent <= 500);
                                 0: the leaf pass evaluates it for every candidate.  Diagnostic; results never depend on it. */
} rt_scene_info;

/* Scene.make (Scene.fs:15-28): partitions bounded/unbounded, builds the BoundingBoxTree on the host,
 * builds the tree the device walks over the same Leaf boxes (rt_set_walk_tree), flattens that (DFS pre-order, on-hit and
 * on-miss successor per node) and keeps a host copy; device copies are made lazily per device.
 * Textures: at most 254 records (more: RT_ERR_UNSUPPORTED); a Checkered tree of any depth that fits them is evaluated as the
 * reference's recursion evaluates it (Texture.fs:56-62), with the map of the record the hittable points at; |grid_size| <= 5e5
 * (beyond, or NaN: RT_ERR_UNSUPPORTED); a child index at or above its parent's or negative, an image without texels or with a
 * non-positive size, a ramp source that is no rt_ramp_source, a texture id on a style that carries a Pixel:
 * RT_ERR_INVALID_ARGUMENT. */
int rt_scene_create(const rt_hittable *hittables, size_t n_hittables,
                    const rt_texture *textures, size_t n_textures, rt_scene **out);
/* Per-scene settings, handed over at creation instead of through the process-wide rt_set_walk_tree default. */
typedef struct rt_scene_options {
    uint32_t struct_size; /* sizeof(rt_scene_options) as the caller compiled it (fields beyond it keep their defaults) */
    int32_t  walk_tree;   /* RT_WALK_TREE_*; -1 = the process default (rt_set_walk_tree) */
} rt_scene_options;
/* rt_scene_create with explicit options (NULL = all defaults).  Thread-safe: reads no process-wide setting when every
 * option is given. */
int rt_scene_create_ex(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                       const rt_scene_options *options, rt_scene **out);
void rt_scene_destroy(rt_scene *scene);
int rt_scene_get_info(const rt_scene *scene, rt_scene_info *out);
/* Flattened tree for inspection/tests: skip[n_nodes], prim[n_nodes] (-1 for Branch), boxes[n_nodes*6] as
 * (minx,maxx,miny,maxy,minz,maxz).  Any pointer may be NULL. */
int rt_scene_get_tree(const rt_scene *scene, int32_t *skip, int32_t *prim, double *boxes);
/* The same arrays for the tree the device image holds (rt_set_walk_tree): identical to rt_scene_get_tree's under
 * RT_WALK_TREE_REFERENCE; under RT_WALK_TREE_SAH another binary tree over the same Leaf boxes, every Branch box again the
 * exact union of the Leaf boxes below it. */
int rt_scene_get_walk_tree(const rt_scene *scene, int32_t *skip, int32_t *prim, double *boxes);
/* The same tree as the TIMED kernel walks it (csrc/rt_device.h, "the node loop of the timed variant"): walk_tree_nodes records in the
 * order the device image stores them -- by depth, so that the top of the tree is a prefix (what a scene too large for the LDS keeps
 * there) -- with explicit links.  boxes[p*6 ..] = lo, hi per axis in single precision, rounded outward from the walk tree's boxes;
 * links[p*5 ..] = { record visited after a hit, record visited after a miss, queue entry of a Leaf (0 for a Branch: 0x4000 | index
 * in the image's object order, or 0x80000000 | index from 16384 objects), shift that pushes it, the Leaf's hittable as an index
 * into rt_scene_create's input (-1 for a Branch) }, records counted from 0, walk_tree_nodes = "tree exhausted".  A Leaf's two links are equal (its exact tests are queued, the walk goes on).  Host-side
 * only (no device needed): for tests of the layout; the format is this build's, not part of the boundary's contract. */
int rt_scene_get_filter_tree(const rt_scene *scene, float *boxes, int32_t *links);

/* ---- Tuning the walk tree to a camera (no counterpart in the reference: BoundingBoxTree.make knows no rays) ----------
 * Renders a PROBE with the scene as it stands -- 16 image rows spread over the frame, through the counting kernel, which logs a
 * thinned-out sample of the rays it traces (8192 are used: origin and direction) -- and rebuilds the tree the device walks
 * from them: split costs are the number of probe rays that hit a candidate box (not its area), and Branch boxes that nearly
 * every arriving ray hits are not tested at all (their children take their place; csrc/rt_scene.h "thinning").  Every pixel
 * stays the same bit for bit, as under rt_set_walk_tree and for the same reason; what changes is aabb_tests (final scene:
 * 23.8 -> about 17 per ray) and the frame time.  rt_scene_get_walk_tree then reports an n-ary tree in the same pre-order/skip
 * form, rt_scene_get_info.walk_tree = RT_WALK_TREE_TUNED, walk_tree_nodes shrinks (n_nodes stays the size of BoundingBoxTree.make's
 * own tree; size rt_scene_get_walk_tree's arrays by walk_tree_nodes).  The probe is deterministic (which rays are logged depends
 * on their random streams only, and the log is sorted), so the same call yields the same tree; a probe whose log still overflows
 * after being thinned to one ray in 2^20 would hold a scheduling-dependent subset, and such a scene is left untuned (tuned = 0).
 * The replacement is failure-atomic: host tree and device copies change together or not at all.
 * A scene that walks the reference's own tree (RT_WALK_TREE_REFERENCE, or fewer than 3 bounded spheres, or non-finite boxes)
 * is left alone: tuned = 0.  Must not run concurrently with renders of the same scene: it replaces the device images (after
 * waiting for the devices that hold one).  Typical use: once after rt_scene_create, with the camera and image size of the
 * frames to come.  Cost on the final scene (round 3): ~1.3 ms of GPU time for the probe (16 rows at a reduced sample count, the
 * timed kernel variant) + ~4 ms of host time for the build (subtrees on separate threads), ~6.5 ms wall in all, against ~13 ms
 * saved per 2401x1601x500spp frame: it pays on the FIRST frame of such a scene (123 ms against 130 ms untuned, 116.6 ms from the
 * second frame on; bench.py reports all three). */
typedef struct rt_tune_info {
    uint32_t struct_size;      /* sizeof(rt_tune_info) as the caller compiled it */
    int32_t  tuned;            /* 1: the walk tree was replaced */
    int32_t  probe_rows;       /* image rows rendered for the probe */
    int32_t  probe_rays;       /* rays the build used */
    int32_t  nodes_before, nodes_after;
    double   box_tests_before, box_tests_after; /* BoundingBox.hits calls per probe ray, counted on the host */
    double   probe_ms, build_ms;
} rt_tune_info;
int rt_scene_tune(rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                  int32_t device, rt_tune_info *info /* may be NULL */);
/* The host half alone, with the caller's own probe: rays[n_rays][6] = origin xyz, direction xyz (at most 8192 of them are used,
 * evenly spaced).  Touches a GPU only to replace device copies of the image that already exist.  probe_rows and probe_ms stay 0. */
int rt_scene_tune_rays(rt_scene *scene, const double *rays, size_t n_rays, rt_tune_info *info /* may be NULL */);

/* ---- Render (Scene.render, Scene.fs:196-236) ---------------------------------------------------- */
typedef struct rt_stats {
    uint64_t rays;        /* Scene.hitObject calls (Scene.fs:62) = primary + secondary rays */
    uint64_t aabb_tests;  /* BoundingBox.hits calls (BoundingBox.fs:30) */
    uint64_t prim_tests;  /* Hittable.hits calls (Hittable.fs:27): sphere + plane tests, unbounded included */
    uint64_t reflections; /* Hittable.Reflection calls (Hittable.fs:8-12) = path vertices shaded */
    uint64_t samples;     /* Scene.traceOnce calls (Scene.fs:118) */
    uint64_t pixels;      /* pixels rendered by this call */
    uint64_t pixels_early;/* pixels that stopped after 2*firstTrial+1 samples (Scene.fs:185-188) */
    double   kernel_ms;   /* device time of the render kernel, HIP events on the launch stream */
    double   total_ms;    /* wall time of the call, host side */
} rt_stats;

#define RT_RENDER_COUNTERS 1u /* fill rays/aabb_tests/prim_tests/reflections (slightly slower kernel variant) */

/*
 * Image geometry (Scene.fs:208-209,219,226): rows = 2*max_height_coord+1, cols = 2*max_width_coord+1;
 * image row index r (0 = top) maps to row = max_height_coord - r - 1, column index c to col = c - max_width_coord.
 *
 * A call renders the image rows r = row_first + i*row_stride for i in [0, n_rows): (0, 1, rows) is the whole
 * frame; (rank, world, ceil((rows-rank)/world)) is one rank's interleaved shard.  RNG streams are keyed by
 * (seed, global pixel index r*cols+c, sample index), so a shard's output does not depend on the sharding.
 *
 * accum: n_rows*cols*4 int32 = PixelStats {Count; SumRed; SumGreen; SumBlue} (Pixel.fs:78-85).
 * rgb:   n_rows*cols*3 uint8 = PixelStats.mean (Pixel.fs:103-108); may be NULL.
 */
int rt_render(const rt_scene *scene, const rt_camera *camera,
              int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
              int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
              uint32_t flags, int32_t *accum_host, uint8_t *rgb_host, rt_stats *stats);

/* Same, with outputs left in device memory (d_accum / d_rgb are device pointers on `device`) and the launch
 * enqueued on `stream` (a hipStream_t, NULL = the null stream).  If `stats` is non-NULL the call synchronises
 * the stream and fills it; with stats == NULL it returns right after the launch.  Any number of launches may be in flight:
 * each takes its counters, work queue and camera from stream-ordered scratch of its own.  The caller's current HIP device
 * is left as it was. */
int rt_render_device(const rt_scene *scene, const rt_camera *camera,
                     int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                     int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
                     uint32_t flags, void *d_accum, void *d_rgb, void *stream, rt_stats *stats);

/* Launch settings of one render call.  0 in any field = that field's process default (the rt_set_* calls below, which
 * exist for bench sweeps); a call that passes a fully specified struct reads no process-wide state.  No setting ever
 * changes a result -- only which wave traces which sample when. */
typedef struct rt_render_options {
    uint32_t struct_size;   /* sizeof(rt_render_options) as the caller compiled it */
    int32_t  block_threads; /* 256, 512, 768 or 1024 threads per workgroup */
    int32_t  chunk_pixels;  /* pixels per wave work unit, <= 64 */
    int32_t  blocks_per_cu; /* cap on resident workgroups per CU */
    int32_t  yield_lanes;   /* lane-scheduling thresholds (DESIGN.md "Kernel") */
    int32_t  refill_lanes;
    int32_t  passes;        /* 1 fused kernel, 2 two passes (phase 1 + decision, cost-ordered phase 2); 0 = default (by shard size) */
    int32_t  park_lanes;    /* capacity of a wave's pool of parked rare-style paths (<= 256); 0 = default, -1 = never park */
} rt_render_options;
int rt_render_device_ex(const rt_scene *scene, const rt_camera *camera,
                        int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                        int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
                        uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                        const rt_render_options *options, rt_stats *stats);

/*
 * Scene.render for a whole frame on SEVERAL GPUs of one node from ONE process (Scene.fs:196-236):
 * device i of `devices[0..n_devices)` renders the image rows r = i, i + n_devices, ... (interleaved: adaptive sampling makes
 * sky rows ~11/spp the cost of object rows) on a stream of its own, all devices concurrently; then ONE gather brings the
 * per-device PixelStats buffers together and the frame is handed back de-interleaved in host memory:
 * accum_host rows*cols*4 int32, rgb_host rows*cols*3 uint8 (may be NULL).  Streams are keyed by the global pixel index, so
 * the frame is bit-identical for any device count.
 *
 * gather: RT_GATHER_RCCL   ncclGroupStart / ncclRecv x (n-1) on devices[0] / ncclSend on the others / ncclGroupEnd over
 *                          xGMI (librccl.so is loaded on first use), then one strided device-to-host copy from devices[0];
 *         RT_GATHER_PEER   hipMemcpyPeerAsync to devices[0] instead of RCCL (also works when `devices` repeats an id);
 *         RT_GATHER_HOST   every device copies its own shard to the host over its own PCIe link (no device-side gather);
 *         RT_GATHER_AUTO   RCCL when n_devices > 1, the ids are distinct and librccl.so loads; else PEER.
 * Calls from several threads over the same device list share its RCCL communicators; each call's group of sends and receives is
 * issued under a mutex of that list, so the groups of two calls never interleave.
 * stats (may be NULL): n_devices entries, one per device's shard; kernel_ms is that device's render time, total_ms the
 * wall time of the whole call (the same in every entry).
 */
enum rt_gather { RT_GATHER_AUTO = 0, RT_GATHER_RCCL = 1, RT_GATHER_PEER = 2, RT_GATHER_HOST = 3 };
int rt_render_frame(const rt_scene *scene, const rt_camera *camera,
                    int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                    const int32_t *devices, int32_t n_devices, uint32_t flags, int32_t gather,
                    const rt_render_options *options,
                    int32_t *accum_host, uint8_t *rgb_host, rt_stats *stats);

/* ---- Ray lists: the caller's own rays (Scene.hitObject, Scene.traceRay) ------------------------------------------------
 * The render kernel's persistent grid, work queue, scene placement and lane scheduler, fed with the caller's rays instead of
 * a camera's (DESIGN.md "Ray lists").  Results are the reference's, bit for bit, for any launch settings.
 *
 * Argument checks come before any device call: RT_ERR_INVALID_ARGUMENT for a NULL scene, a NULL rays / hit_index / colour
 * pointer when n > 0, n > INT32_MAX, bounce_depth < 0 (or > 0xFFFFFF), or bad options; nothing is written then.  n = 0 is a
 * no-op returning RT_OK.  flags: RT_RENDER_COUNTERS runs the counting variant (the exact walk) and fills stats->rays,
 * aabb_tests, prim_tests and reflections; kernel_ms and total_ms are always filled; samples and pixels stay 0.
 *
 * Device variants follow rt_render_device's contract: the launch is enqueued on `stream` (device pointers on `device`),
 * with stats == NULL the call returns right after the launch, scratch is stream-ordered (any number of calls may be in
 * flight), the caller's current device is left as it was.  Host variants copy in, run the device variant and copy out.
 * options: as for rt_render_device_ex; chunk_pixels counts RAYS per work unit here (default 64); a block of 512 or 768
 * threads runs as 1024. */

/* Scene.hitObject (Scene.fs:62-91) for n caller rays.  rays: n*6 doubles (origin xyz, vector xyz); ray i is
 * Ray.make'(origin, vector) (Ray.fs:26-34), computed on the device.  hit_index: n int32, index into
 * rt_scene_create's array, -1 = ValueNone, -2 = Ray.make' gave ValueNone.  strike: n*3 doubles (Ray.walkAlong ray
 * bestLength, Scene.fs:91), NaN where hit_index < 0; may be NULL. */
int rt_hit_objects(const rt_scene *scene, int32_t device, size_t n, const double *rays,
                   uint32_t flags, int32_t *hit_index, double *strike, rt_stats *stats);
int rt_hit_objects_device(const rt_scene *scene, int32_t device, size_t n, const void *d_rays,
                          uint32_t flags, void *d_hit_index, void *d_strike, void *stream,
                          const rt_render_options *options, rt_stats *stats);

/* Scene.traceRay (Scene.fs:93-114) from LightRay {Ray.make'(origin, vector); Colour.White}, at most
 * bounce_depth+1 hits.  colour: n*3 uint8; HotPink at the bounce limit; Black (0,0,0) where Ray.make' fails.
 * rng: n*4 uint32 xorshift128 states (FloatProducer, Float.fs:14-76), read, then written back advanced (unchanged where
 * Ray.make' fails).  If rng is NULL, ray i draws from the stream keyed (seed, stream_base + i, sample), the same keying
 * as a render's (pixel, sample), and no state is returned. */
int rt_trace_rays(const rt_scene *scene, int32_t device, size_t n, const double *rays, uint32_t *rng,
                  uint64_t seed, uint64_t stream_base, uint32_t sample, int32_t bounce_depth,
                  uint32_t flags, uint8_t *colour, rt_stats *stats);
int rt_trace_rays_device(const rt_scene *scene, int32_t device, size_t n, const void *d_rays, void *d_rng,
                         uint64_t seed, uint64_t stream_base, uint32_t sample, int32_t bounce_depth,
                         uint32_t flags, void *d_colour, void *stream,
                         const rt_render_options *options, rt_stats *stats);

/* ---- Footprints: Scene.renderPixel for caller-defined cameras ----------------------------------------------------------
 * A pixel's camera as data (DESIGN.md "Footprints"): footprint i is 12 doubles, origin[3] base[3] du[3] dv[3].  Sample s
 * (0, 1, 2, ... as a render counts them) of pixel i draws (r1, r2) = GetTwo from the stream keyed (seed, stream_base + i, s)
 * -- a render's (pixel, sample) keying -- and traces Ray.make'(origin, (base + r1*du) + r2*dv) (each product and sum rounded
 * on its own) from White with the same generator, at most bounce_depth+1 hits.  Where Ray.make' gives ValueNone the sample is
 * Black: Count goes up, the sums do not, nothing more is drawn.  How many samples a pixel gets is Scene.renderPixel's rule
 * (Scene.fs:172-194) with samples_per_pixel: firstTrial = min 5 (spp/2); firstTrial+1 samples, then firstTrial more; the
 * pixel stops there if Pixel.difference of the two means is 0, else takes the remaining spp - 2*firstTrial - 1.
 * accum: n*4 int32 {Count, SumRed, SumGreen, SumBlue}; rgb: n*3 uint8 = PixelStats.mean, may be NULL.  Which image the n
 * pixels form is the caller's business; the slice [a, b) of a list rendered with stream_base + a equals that slice of the
 * whole list's result.  One launch (or pass A, the ordering and pass B) through the kernel stages of a frame; the footprints'
 * first rays walk the tree as every other ray does.
 *
 * Argument checks come before any device call: RT_ERR_INVALID_ARGUMENT for a NULL scene, NULL footprints or accum when
 * n > 0, n > INT32_MAX, samples_per_pixel < 1, bounce_depth < 0 (or > 0xFFFFFF), or bad options; nothing is written then.
 * n = 0 is a no-op returning RT_OK with zeroed stats.  stats is filled as a render fills it: samples, pixels (= n),
 * pixels_early, kernel_ms and total_ms always, the four counters under RT_RENDER_COUNTERS.
 * The device variant follows rt_render_device's contract: enqueued on `stream`, with stats == NULL it returns right after
 * the launch, scratch is stream-ordered, the caller's current device is left as it was.  options: as for a frame shard
 * (chunk_pixels is pixels per unit, passes 0/1/2 chooses fused or two-pass); a block of 512 or 768 threads runs as 1024.
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_render_footprints(const rt_scene *scene, int32_t device, size_t n, const double *footprints,
                         int32_t samples_per_pixel, int32_t bounce_depth, uint64_t seed, uint64_t stream_base,
                         uint32_t flags, int32_t *accum, uint8_t *rgb /* may be NULL */, rt_stats *stats);
int rt_render_footprints_device(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints,
                                int32_t samples_per_pixel, int32_t bounce_depth, uint64_t seed, uint64_t stream_base,
                                uint32_t flags, void *d_accum, void *d_rgb, void *stream,
                                const rt_render_options *options, rt_stats *stats);

/* ---- Pixel lists: a caller-chosen list of a FRAME's pixels, bit for bit -------------------------------------------------
 * pixels[i] is a GLOBAL PIXEL INDEX g = r*cols + c of the frame rt_render renders from (scene, camera, max_width_coord,
 * max_height_coord, seed): r the image row (0 = top), c the column, cols = 2*max_width_coord+1 (Scene.render's coordinate
 * mapping, Scene.fs:219,226) -- the index a whole-frame accum uses and the one the streams are keyed by.  Outputs are
 * COMPACT, in list order: accum[i*4 .. i*4+3] {Count, SumRed, SumGreen, SumBlue} and rgb[i*3 .. i*3+2] (may be NULL)
 * belong to entry i.
 *
 * Entry i IS pixel g of that frame, in every PixelStats word and every rgb byte: Scene.renderPixel (Scene.fs:157-194) with
 * the frame's streams (seed, g, sample), the frame's camera rays and the adaptive rule with camera->samples_per_pixel --
 * for any list order, any subset, any launch settings and both kernel variants (DESIGN.md "Pixel lists").  Duplicates are
 * allowed: each entry is rendered into its own slot, so equal entries give equal results.  A crop, a tile, the pixels a
 * partial pixel map lacks, a checkerboard or a split of a frame by cost are all lists.
 *
 * rt_render_pixels_extend* continue the n compact entries of a buffer a list render made, by rt_render_extend's contract
 * (below) word for word: samples_done >= 12, the target is camera->samples_per_pixel, Count == samples_done continues,
 * Count == 11 is final, any other Count makes the buffer MALFORMED and nothing is written; same list, same every other
 * argument as the call that made the buffer.
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for everything
 * rt_render rejects about scene, camera, geometry and options, a NULL pixels or accum with n > 0, n > INT32_MAX, a frame of
 * more than INT32_MAX pixels, and (extend) samples_done < 12 or a target below it.  n = 0 is a no-op returning RT_OK with
 * zeroed stats (and so is an extension with target == samples_done).
 * An entry outside [0, rows*cols) makes the LIST malformed (the check guards meaning, not memory: every store is indexed by
 * list position).  The host variants find it on the host: RT_ERR_INVALID_ARGUMENT before any device call.  The device variants
 * find it on the device, in front of the render, on the same stream: NO pixel is rendered, d_accum and d_rgb stay as they
 * were, and the call returns RT_ERR_INVALID_ARGUMENT when stats is given (it synchronises); with stats == NULL the untouched
 * buffers are the caller's evidence.
 *
 * stats as for a footprint list: pixels = n, samples, pixels_early, kernel_ms, total_ms, the four counters under
 * RT_RENDER_COUNTERS.  The device variants follow rt_render_device's contract: enqueued on `stream`, scratch is stream-ordered,
 * any number of calls in flight, with stats == NULL the call returns right after the launch, the caller's current device is
 * left as it was; the list must not change until the launch has finished.  options: as for a footprint list (a block of 512
 * or 768 threads runs as 1024; an extension ignores `passes`).
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_render_pixels(const rt_scene *scene, const rt_camera *camera,
                     int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                     int32_t device, size_t n, const int32_t *pixels, uint32_t flags,
                     int32_t *accum, uint8_t *rgb /* may be NULL */, rt_stats *stats);
int rt_render_pixels_device(const rt_scene *scene, const rt_camera *camera,
                            int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                            int32_t device, size_t n, const void *d_pixels, uint32_t flags,
                            void *d_accum, void *d_rgb, void *stream,
                            const rt_render_options *options, rt_stats *stats);
int rt_render_pixels_extend(const rt_scene *scene, const rt_camera *camera,
                            int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                            int32_t device, size_t n, const int32_t *pixels, uint32_t flags, int32_t samples_done,
                            int32_t *accum /* in, out */, uint8_t *rgb /* out, may be NULL */, rt_stats *stats);
int rt_render_pixels_extend_device(const rt_scene *scene, const rt_camera *camera,
                                   int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                                   int32_t device, size_t n, const void *d_pixels, uint32_t flags, int32_t samples_done,
                                   void *d_accum, void *d_rgb, void *stream,
                                   const rt_render_options *options, rt_stats *stats);

/* ---- a batch of views: Scene.render (Scene.fs:157-236) for n_views cameras over one scene, in ONE launch ----
 * A turntable, a fly-through, the training views of a learned model, one view under K seeds: K small frames of one scene, none of
 * which fills the device alone.  The batch is one launch: the scene is staged once per workgroup, pass B runs once over the
 * cost-ordered pixels of all views, and no frame's tail idles the machine before the next frame starts.
 *
 * cameras[v] and seeds[v] (seeds == NULL: every view uses `seed`) describe view v; every view is a frame of
 * rows = 2*max_height_coord+1 by cols = 2*max_width_coord+1 pixels.  accum is [n_views][rows][cols][4], rgb [n_views][rows][cols][3]
 * (may be NULL): view v's slice is a frame's buffer.
 *
 * View v IS rt_render(scene, &cameras[v], max_width_coord, max_height_coord, seeds ? seeds[v] : seed, device, 0, 1, rows, ...), in
 * every PixelStats word and every rgb byte -- for any launch settings, both kernel variants, fused or two-pass rendering (DESIGN.md
 * "Batches of views").  So rt_render_extend_device continues view v's slice with cameras[v] as it continues a frame.
 * `cameras` and `seeds` are HOST pointers in both variants and are fully read before the call returns.
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for a NULL scene, a
 * NULL cameras or accum with n_views > 0, n_views < 0, any camera or geometry rt_render rejects, cameras that do not all share
 * samples_per_pixel and bounce_depth (the sample counts of a pass are launch parameters of the whole batch),
 * n_views*rows*cols > INT32_MAX, and bad options.  n_views = 0 is a no-op returning RT_OK with zeroed stats.
 * A scene that holds a texture program (RT_TEXTURE_PROGRAM) is RT_ERR_UNSUPPORTED: the batch kernels are built for plain and
 * textured (Checkered, Image) scenes only.
 *
 * stats is the sum over the views of what rt_render reports for each: pixels = n_views*rows*cols, samples, pixels_early,
 * kernel_ms, total_ms, the four counters under RT_RENDER_COUNTERS.  The device variant follows rt_render_device's contract:
 * enqueued on `stream`, scratch is stream-ordered, any number of calls in flight, with stats == NULL the call returns right after
 * the launch, the caller's current device is left as it was.  options: as for a pixel list (a block of 512 or 768 threads runs as
 * 1024).
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_render_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                    int32_t max_width_coord, int32_t max_height_coord,
                    const uint64_t *seeds /* n_views, or NULL: every view uses `seed` */, uint64_t seed,
                    int32_t device, uint32_t flags,
                    int32_t *accum /* [n_views][rows][cols][4] */, uint8_t *rgb /* [n_views][rows][cols][3], may be NULL */,
                    rt_stats *stats);
int rt_render_views_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                           int32_t max_width_coord, int32_t max_height_coord,
                           const uint64_t *seeds, uint64_t seed,
                           int32_t device, uint32_t flags,
                           void *d_accum, void *d_rgb, void *stream,
                           const rt_render_options *options, rt_stats *stats);

/* ---- Camera hits: the object each pixel sample's camera ray strikes first ------------------------------------------------
 * A frame is (scene, camera, max_width_coord, max_height_coord, seed), as for rt_render.  For list entry i -- the GLOBAL PIXEL INDEX
 * g = r*cols + c of rt_render_pixels (pixels == NULL: entry i is pixel i, n <= rows*cols) -- and sample s in
 * [sample_first, sample_first + n_samples):
 *   rand = the stream keyed (seed, g, s); (r1, r2) = rand.GetTwo(); the ray is Scene.traceOnce's (Scene.fs:129-143) with
 *   row = max_height_coord - r - 1 and col = c - max_width_coord; the answer is Scene.hitObject scene ray (Scene.fs:62-91).
 * It is the very ray sample s of pixel g starts with in rt_render and rt_render_pixels: an object-id or depth buffer, a per-sample
 * coverage mask, "all pixels that show sphere 17" (the list rt_render_pixels and the targets rt_render_extend_map want next).
 *
 * Outputs are in list order, samples innermost: slot i*n_samples + (s - sample_first) holds entry i, sample s.  hit_index and strike
 * are rt_hit_objects': hit_index is an index into rt_scene_create's array, -1 ValueNone, -2 Ray.make' gave ValueNone; strike
 * (may be NULL) is Ray.walkAlong ray bestLength, NaN where hit_index < 0.  rays_out (may be NULL) is the ray itself, origin then
 * unit direction, all six NaN at -2: depth is |strike - origin|, and the rays can be fed to rt_trace_rays.  Duplicates are
 * allowed: every store is indexed by slot, never by an entry's value.  camera->samples_per_pixel and bounce_depth must pass
 * rt_render's checks and are not otherwise used.
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for everything
 * rt_render_pixels rejects about scene, camera, geometry and options, sample_first < 0, n_samples < 1,
 * sample_first + n_samples > 8000000, n * n_samples > INT32_MAX, a NULL hit_index with n > 0, and pixels == NULL with
 * n > rows*cols.  n = 0 is a no-op returning RT_OK with zeroed stats.  An entry outside [0, rows*cols) makes the LIST malformed, as
 * for rt_render_pixels: the host variant refuses it on the host; the device variant finds it on the device, in front of the launch
 * and on the same stream, writes NO output and returns RT_ERR_INVALID_ARGUMENT when stats is given.
 *
 * stats: pixels = n, samples = n*n_samples, kernel_ms, total_ms; under RT_RENDER_COUNTERS the counting variant runs and fills
 * rays (the slots whose ray was made), aabb_tests and prim_tests; reflections is 0.  The timed variant starts a camera ray from its
 * pixel's candidates exactly as a frame does, the counting variant walks from the root: results never depend on which.  The device
 * variant follows rt_render_device's contract: enqueued on `stream`, scratch is stream-ordered, any number of calls in flight, with
 * stats == NULL the call returns right after the launch, the caller's current device is left as it was; the list must not change
 * until the launch has finished.  options: chunk_pixels counts list entries per work unit; a block of 512 or 768 threads runs as
 * 1024; passes and park_lanes are checked and not used.
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_camera_hits(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                   uint64_t seed, int32_t device, size_t n, const int32_t *pixels /* NULL: entry i is pixel i, n <= rows*cols */,
                   int32_t sample_first, int32_t n_samples, uint32_t flags,
                   int32_t *hit_index /* n*n_samples */, double *strike /* n*n_samples*3, may be NULL */,
                   double *rays_out /* n*n_samples*6, may be NULL */, rt_stats *stats);
int rt_camera_hits_device(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                          uint64_t seed, int32_t device, size_t n, const void *d_pixels /* may be NULL */,
                          int32_t sample_first, int32_t n_samples, uint32_t flags,
                          void *d_hit_index, void *d_strike /* may be NULL */, void *d_rays_out /* may be NULL */,
                          void *stream, const rt_render_options *options, rt_stats *stats);

/* ---- Camera hits over a batch of views: the above for n_views cameras and ONE list, in ONE launch ---------------------------
 * The object-id buffers, strike points (depth) and camera rays of a turntable, a fly-through or the training views of a learned
 * model: what rt_render_views' K frames SEE.  Scene.hitObject (Scene.fs:62-91) of Scene.traceOnce's ray (Scene.fs:129-143), as above.
 *
 * cameras[v] and seeds[v] (seeds == NULL: every view uses `seed`) describe view v; every view is a frame of
 * rows = 2*max_height_coord+1 by cols = 2*max_width_coord+1 pixels.  The list (`pixels`, n entries; NULL: entry i is pixel i), the
 * sample range and the frame size are SHARED by the views.  Every output is [n_views][n][n_samples](...): slot
 * (v*n + i)*n_samples + (s - sample_first) holds view v, entry i, sample s.
 *
 * View v's slice of every output IS what rt_camera_hits(scene, &cameras[v], max_width_coord, max_height_coord,
 * seeds ? seeds[v] : seed, device, n, pixels, sample_first, n_samples, ...) writes, bit for bit -- NaN positions and the -1 / -2
 * codes included -- for any launch settings and both kernel variants: the stream is keyed (seed, pixel, sample) and nothing else.
 * The cameras need NOT share samples_per_pixel or bounce_depth (they are checked, as by rt_camera_hits, and not otherwise used), and
 * a scene that holds a texture program is taken: nothing is shaded.  `cameras` and `seeds` are HOST pointers in both variants and are
 * fully read before the call returns.
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for a NULL scene,
 * n_views < 0, a NULL cameras with n_views > 0, anything rt_camera_hits refuses (camera, geometry, sample range, n * n_samples,
 * a NULL hit_index with n > 0, pixels == NULL with n > rows*cols, options) -- reported for the first offending view --
 * and n_views * n * n_samples > INT32_MAX.  n_views = 0 or n = 0 is a no-op returning RT_OK with zeroed stats (with n_views = 0 only the
 * scene, n_views and the options are checked: there is no view to report for).  A list with an entry outside [0, rows*cols) is
 * malformed as for rt_camera_hits: the host variant refuses it on the host; the device variant checks the shared list ONCE on the
 * stream, in front of the launch, writes NO output in any view and returns RT_ERR_INVALID_ARGUMENT when stats is given.
 *
 * stats: pixels = n_views*n, samples = n_views*n*n_samples, reflections 0, kernel_ms, total_ms; under RT_RENDER_COUNTERS the counting
 * variant's rays, aabb_tests and prim_tests, summed over the views.  The device variant follows rt_camera_hits_device's contract
 * (stream, scratch, stats == NULL, current device, options: chunk_pixels counts list entries per work unit -- a unit never spans two
 * views, csrc/rt_views_plan.h -- and a block of 512 or 768 threads runs as 1024).
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_camera_hits_views(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                         int32_t max_width_coord, int32_t max_height_coord,
                         const uint64_t *seeds /* n_views, or NULL: every view uses `seed` */, uint64_t seed,
                         int32_t device, size_t n, const int32_t *pixels /* ONE list shared by all views; NULL: entry i is pixel i */,
                         int32_t sample_first, int32_t n_samples, uint32_t flags,
                         int32_t *hit_index /* [n_views][n][n_samples] */, double *strike /* ...[3], may be NULL */,
                         double *rays_out /* ...[6], may be NULL */, rt_stats *stats);
int rt_camera_hits_views_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                                int32_t max_width_coord, int32_t max_height_coord,
                                const uint64_t *seeds, uint64_t seed,
                                int32_t device, size_t n, const void *d_pixels /* may be NULL */,
                                int32_t sample_first, int32_t n_samples, uint32_t flags,
                                void *d_hit_index, void *d_strike /* may be NULL */, void *d_rays_out /* may be NULL */,
                                void *stream, const rt_render_options *options, rt_stats *stats);

/* ---- Path records: the vertices of each sample's path ---------------------------------------------------------------------
 * A SLOT is one path: follow Scene.traceRay maxCount scene &ray (Scene.fs:93-114) from {Ray = ray; Colour = White}.  Every loop
 * iteration in which hitObject answers ValueSome (object, strikePoint) is VERTEX j = 0, 1, ... of the path.  Per vertex:
 *   hit_index     the object's index in rt_scene_create's array (as rt_hit_objects')
 *   strike        Ray.walkAlong ray bestLength (Scene.fs:91)
 *   colour_after  object.Reflection (&ray, strikePoint) gave ValueNone: ray.Colour after the call; ValueSome c: c
 *   ray_after     ValueNone: ray.Ray after the call (origin, unit direction); ValueSome: six NaN
 * Per slot: n_vertices, the number of vertices the path has (NOT capped by what is stored); colour, traceRay's result; end:
 *   RT_PATH_MISS          hitObject gave ValueNone; the result is Black
 *   RT_PATH_STOPPED       Reflection gave ValueSome
 *   RT_PATH_BOUNCE_LIMIT  bounces > maxCount; the result is HotPink and n_vertices = maxCount + 1
 *   RT_PATH_NO_RAY        Ray.make' gave ValueNone: Black, 0 vertices, nothing drawn beyond what made the ray (as rt_trace_rays)
 * Only the first max_vertices (K) vertices of a slot are stored, at record slot*K + j; the unused records of a slot are written
 * too: hit_index -1, strike and ray_after NaN, colour_after 0.  Every element of every non-NULL output is written by every
 * successful call, and every store is indexed by slot, never by a list entry's value.  K == 0 ignores the per-record pointers.
 *
 * Camera paths (rt_camera_paths): the list, the frame, the sample range and the slot numbering i*n_samples + (s - sample_first) are
 * rt_camera_hits'.  The stream is (seed, g, s); GetTwo makes Scene.traceOnce's ray (Scene.fs:129-143) and the SAME generator then
 * feeds the path, maxCount = camera->bounce_depth: the very path sample s of pixel g follows in rt_render and rt_render_pixels.
 * first_ray (6 doubles per slot) is that camera ray, as rt_camera_hits' rays_out.  summary: RT_PATH_SUMMARY_WORDS int32 per list
 * ENTRY, reduced over the entry's n_samples slots (integer sums and one max, so no order can matter):
 *   [0] slots  [1] sum of n_vertices  [2] max n_vertices  [3..6] slots ending MISS, STOPPED, BOUNCE_LIMIT, NO_RAY
 *   [7] slots with >= 1 vertex  [8..10] sums of R, G, B of colour_after at vertex 0 over those (first-hit albedo)  [11] 0
 *   [12..15] {Count, SumRed, SumGreen, SumBlue} of colour over the slots: PixelStats over these samples -- for a pixel that took all
 *   spp samples and the range [0, spp) the render's accum words.  Duplicated list entries each get their own 16 words.
 * Ray paths (rt_trace_paths): slot i is ray i; rays, rng (given: read, then written back advanced; NULL: the stream keyed
 * (seed, stream_base + i, sample)) and bounce_depth are exactly rt_trace_rays', and colour and the returned states equal its.
 *
 * The contract is rt_camera_hits' for the camera variants and rt_trace_rays' for the ray variants (argument checks before any device
 * call and nothing written when one fails, n = 0 a no-op with zeroed stats, an entry outside the frame makes the list malformed --
 * found on the host by the host variant, on the device in front of the launch by the device variant --, stream-ordered scratch, any
 * number of calls in flight, stats == NULL returns after the launch, the caller's device is left as it was).  Refused as well: out
 * NULL or of another struct_size, every output NULL, max_vertices < 0, slots * max(K, 1) > INT32_MAX,
 * n_samples * (bounce_depth + 1) > INT32_MAX when summary is given, first_ray or summary given to a ray-path call.
 * flags: RT_RENDER_COUNTERS runs the counting variant and fills rays (hitObject calls), aabb_tests, prim_tests and reflections
 * (= the sum of n_vertices).  stats: pixels = n and samples = slots, always.  options: block_threads (512 and 768 run as 1024),
 * chunk_pixels (slots per run of the queue, default 64) and blocks_per_cu are honoured; the others are checked and not used.
 * Added symbols and one added struct only -- RT_ABI_VERSION stays 7. */
enum rt_path_end { RT_PATH_MISS = 0, RT_PATH_STOPPED = 1, RT_PATH_BOUNCE_LIMIT = 2, RT_PATH_NO_RAY = 3 };
#define RT_PATH_SUMMARY_WORDS 16
typedef struct rt_path_outputs { /* host pointers in the host variants, device pointers in the _device variants; any may be NULL */
    uint32_t struct_size;        /* sizeof(rt_path_outputs) */
    int32_t max_vertices;        /* K >= 0 */
    int32_t *n_vertices;         /* per slot: 1 */
    int32_t *end;                /* per slot: 1 (enum rt_path_end) */
    uint8_t *colour;             /* per slot: 3 */
    double *first_ray;           /* per slot: 6 (camera paths only) */
    int32_t *hit_index;          /* per record slot*K + j: 1 */
    double *strike;              /* per record: 3 */
    uint8_t *colour_after;       /* per record: 3 */
    double *ray_after;           /* per record: 6 */
    int32_t *summary;            /* per list entry: RT_PATH_SUMMARY_WORDS (camera paths only) */
} rt_path_outputs;
int rt_camera_paths(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                    uint64_t seed, int32_t device, size_t n, const int32_t *pixels /* NULL: entry i is pixel i, n <= rows*cols */,
                    int32_t sample_first, int32_t n_samples, uint32_t flags, const rt_path_outputs *out, rt_stats *stats);
int rt_camera_paths_device(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                           uint64_t seed, int32_t device, size_t n, const void *d_pixels /* may be NULL */,
                           int32_t sample_first, int32_t n_samples, uint32_t flags, const rt_path_outputs *out,
                           void *stream, const rt_render_options *options, rt_stats *stats);
int rt_trace_paths(const rt_scene *scene, int32_t device, size_t n, const double *rays, uint32_t *rng /* n*4, may be NULL */,
                   uint64_t seed, uint64_t stream_base, uint32_t sample, int32_t bounce_depth, uint32_t flags,
                   const rt_path_outputs *out, rt_stats *stats);
int rt_trace_paths_device(const rt_scene *scene, int32_t device, size_t n, const void *d_rays, void *d_rng /* may be NULL */,
                          uint64_t seed, uint64_t stream_base, uint32_t sample, int32_t bounce_depth, uint32_t flags,
                          const rt_path_outputs *out, void *stream, const rt_render_options *options, rt_stats *stats);
/* Diagnostic: the plan (csrc/rt_paths_plan.h) of the calling THREAD's last path launch: block, grid, chunk, lds_bytes,
 * lds_resident (1: the filter loop over the scene in LDS ran), counting, textured, slots.  All 0 before the first launch. */
int rt_dev_last_paths_plan(int64_t out[8]);

/* ---- Surface records at hits: normal, side, colour, tint and texture coordinates ---------------------------------------------
 * What the surface is like where a ray strikes: the values Hittable.Reflection (Hittable.fs:8-12) forms from the object, the strike
 * point and the incoming ray's origin, for any list of hits -- rt_hit_objects', rt_camera_hits', the vertices of path records.
 * A SLOT is (hit_index, strike, origin): hit_index indexes rt_scene_create's array as every hit query returns it, `rays` holds six
 * doubles per slot of which only the origin (the first three) is read.  Per slot, with obj = hittables[hit_index]:
 *   no surface   hit_index -1 or -2, or a component of strike or origin that is not finite (the reference throws or converts out of
 *                range there): normal and uv NaN, inside 0, colour and tint 0,0,0.
 *   spheres      (Sphere.fs:150-200)  n0 = Ray.make' strike (strike - centre) (Sphere.normal, Sphere.fs:65-66; ValueNone: normal is three
 *                NaN, the rest of the record stays defined); inside = (Float.compare |centre - origin|^2 radius^2 <> Greater) <>
 *                (Float.compare radius 0.0 = Less); normal = inside ? -1.0 * n0 : n0.  colour: LightSourceCap -- its Pixel when
 *                Float.compare strike.x (centre.x + (radius - radius / 4.0)) = Greater, else Black (Sphere.fs:190-200); every other style
 *                -- Texture.colourAt strike texture (the plain Pixel without a texture; programs included).
 *   planes       (InfinitePlane.fs:43-99)  normal as given, never flipped; inside 0; colour: Texture.colourAt for LightSource, the
 *                plane's Pixel otherwise.
 *   tint         the colour Reflection leaves a WHITE LightRay with: `colour` for LightSource / LightSourceCap (Pixel.combine White c = c),
 *                Pixel.darken albedo colour for every other style.
 *   uv           Sphere.planeMapInverse map_radius map_centre strike (Sphere.fs:55-61) where the style carries a parameterised texture whose
 *                root record is not RT_TEXTURE_COLOUR; NaN, NaN elsewhere.
 * normal, inside and colour are bit for bit what the render's reflection uses; tint is bit for bit colour_after of the first vertex of
 * rt_trace_paths for the same ray.  Every element of every non-NULL output is written by every successful call.
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for a NULL scene, a NULL
 * hit_index / strike / rays with n > 0, out NULL or of another struct_size, every output NULL, n > INT32_MAX, bad options.  n = 0 is a
 * no-op returning RT_OK with zeroed stats.  An index outside [-2, n_hittables) makes the LIST malformed, as an out-of-frame entry of a
 * pixel list does: the host variant refuses it on the host; the device variant finds it on the device, in front of the launch and on the
 * same stream, writes NO output and returns RT_ERR_INVALID_ARGUMENT when stats is given.
 * stats: samples = n, kernel_ms, total_ms; every other count 0.  RT_RENDER_COUNTERS is accepted and changes nothing.  The device
 * variant follows rt_camera_hits_device's contract (enqueued on `stream`, stream-ordered scratch, any number of calls in flight,
 * stats == NULL returns after the launch, the caller's current device is restored); options are checked and not used.
 *
 * rt_camera_surfaces: the arguments of rt_camera_hits up to flags; hit_index and strike (each may be NULL here) are bit for bit
 * rt_camera_hits'; the surface record of slot i*n_samples + (s - sample_first) is that of what the slot's camera ray strikes first
 * (every origin is camera->view_origin).  List semantics, refusals and a malformed list are rt_camera_hits'; stats are its own with
 * kernel_ms the sum of both kernels.  A scene that holds a texture program is taken.
 * Added symbols and one added struct only (rt_abi_sizeof(13)) -- no existing struct, field or symbol changed, so RT_ABI_VERSION stays 7. */
typedef struct rt_surface_outputs { /* every pointer may be NULL; host pointers for the host variants, device pointers for *_device */
    uint32_t struct_size;           /* sizeof(rt_surface_outputs) */
    void *normal;                   /* double [slots][3] */
    void *inside;                   /* uint8  [slots]    */
    void *colour;                   /* uint8  [slots][3] */
    void *tint;                     /* uint8  [slots][3] */
    void *uv;                       /* double [slots][2] */
} rt_surface_outputs;
int rt_surfaces(const rt_scene *scene, int32_t device, size_t n, const int32_t *hit_index, const double *strike /* n*3 */,
                const double *rays /* n*6, only the origins are read */, uint32_t flags, const rt_surface_outputs *out, rt_stats *stats);
int rt_surfaces_device(const rt_scene *scene, int32_t device, size_t n, const void *d_hit_index, const void *d_strike, const void *d_rays,
                       uint32_t flags, const rt_surface_outputs *out, void *stream, const rt_render_options *options, rt_stats *stats);
int rt_camera_surfaces(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                       uint64_t seed, int32_t device, size_t n, const int32_t *pixels /* NULL: entry i is pixel i, n <= rows*cols */,
                       int32_t sample_first, int32_t n_samples, uint32_t flags,
                       int32_t *hit_index /* n*n_samples, may be NULL */, double *strike /* n*n_samples*3, may be NULL */,
                       const rt_surface_outputs *out, rt_stats *stats);
int rt_camera_surfaces_device(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                              uint64_t seed, int32_t device, size_t n, const void *d_pixels /* may be NULL */,
                              int32_t sample_first, int32_t n_samples, uint32_t flags,
                              void *d_hit_index /* may be NULL */, void *d_strike /* may be NULL */,
                              const rt_surface_outputs *out, void *stream, const rt_render_options *options, rt_stats *stats);
/* Diagnostic: the plan (csrc/rt_surface_plan.h) of the calling THREAD's last surface launch: slots, tile slots, grid, block, 1 if the
 * program variant ran, 1 if the texture phase was enabled, textured slots evaluated (-1 when stats == NULL), 0.  All 0 before the first. */
int rt_dev_last_surface_plan(int64_t out[8]);

/* ---- Extending a rendered buffer to a higher sample count --------------------------------------------------------------
 * render at a, then extend a -> b  ==  render at b, for every PixelStats word and every rgb byte, for any 12 <= a <= b
 * (DESIGN.md "Extending a frame"): sample s of a pixel is the same ray tree whenever it is traced, the sums are integers, and
 * Scene.renderPixel's stopping rule (Scene.fs:172-188) reads only the first 11 samples at every spp >= 10.  A preview, a
 * time-budgeted render, a checkpoint or "more samples, please" therefore costs only the samples it adds.
 *
 * camera->samples_per_pixel (footprints: samples_per_pixel) is the TARGET b; samples_done is the sample count `accum` was
 * rendered or last extended with.  Every other argument means what it meant in the call that produced the buffer and must
 * be the same: scene, camera, geometry, seed, row shard, footprints, stream_base.  accum is read and written; rgb is output
 * only and may be NULL.
 *
 * Pixel classes: Count == samples_done -- the pixel is continued with samples samples_done .. b-1; Count == 11 -- it stopped
 * early, is final at every such spp, and its PixelStats are not touched; any other Count -- the buffer is not what the
 * arguments say (MALFORMED).  If the shard holds even one such pixel the call continues NO pixel: accum stays as it was, bit
 * for bit, rgb is not written, and the host variants return RT_ERR_INVALID_ARGUMENT; so does the device variant when stats is
 * given (it synchronises).  With stats == NULL the device variant cannot report it: the unchanged Counts are the caller's
 * evidence.  Otherwise rgb, when given, is written for EVERY pixel of the shard, final ones included, as PixelStats.mean of
 * the resulting sums.
 *
 * Argument checks come before any device call: RT_ERR_INVALID_ARGUMENT for samples_done < 12 (below, firstTrial differs and
 * Count cannot tell a stopped pixel from a finished one), a target below samples_done, a NULL accum with pixels to do, a
 * shard of 2^32 pixels or more, and everything the base call rejects; nothing is written then.  Target == samples_done and
 * empty shards (n_rows = 0, n = 0) are no-ops returning RT_OK with zeroed stats.
 *
 * stats describe this call alone: samples = the samples added, pixels = the shard's pixels, pixels_early = the final pixels
 * found, kernel_ms = list building plus pass B; under RT_RENDER_COUNTERS the four counters cover the samples this call traced,
 * so the counters of render(a) plus extend(a -> b) equal render(b)'s.
 *
 * The device variants follow rt_render_device's contract: enqueued on `stream`, scratch is stream-ordered, with
 * stats == NULL the call returns right after the launch, any number of calls may be in flight, the caller's current device
 * is left as it was.  options: as for the base call; `passes` is accepted and ignored -- an extension is pass B alone (a
 * list-building kernel over the stored Counts in place of pass A and the ordering), there is no fused form of it.
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_render_extend(const rt_scene *scene, const rt_camera *camera,
                     int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                     int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
                     uint32_t flags, int32_t samples_done, int32_t *accum /* in, out */, uint8_t *rgb /* out, may be NULL */,
                     rt_stats *stats);
int rt_render_extend_device(const rt_scene *scene, const rt_camera *camera,
                            int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                            int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
                            uint32_t flags, int32_t samples_done, void *d_accum, void *d_rgb, void *stream,
                            const rt_render_options *options, rt_stats *stats);
int rt_render_footprints_extend(const rt_scene *scene, int32_t device, size_t n, const double *footprints,
                                int32_t samples_per_pixel /* target */, int32_t bounce_depth, uint64_t seed, uint64_t stream_base,
                                uint32_t flags, int32_t samples_done, int32_t *accum /* in, out */, uint8_t *rgb /* out, may be NULL */,
                                rt_stats *stats);
int rt_render_footprints_extend_device(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints,
                                       int32_t samples_per_pixel /* target */, int32_t bounce_depth, uint64_t seed, uint64_t stream_base,
                                       uint32_t flags, int32_t samples_done, void *d_accum, void *d_rgb, void *stream,
                                       const rt_render_options *options, rt_stats *stats);

/* ---- Extending by map: every pixel to a sample count of its own --------------------------------------------------------------
 * The extension above has one target for the whole shard; here `targets` holds one int32 per pixel of the shard, numbered as
 * accum is laid out (i = local_row * cols + col; footprints: the list index).  The stored Count of a pixel is the whole state
 * needed to continue that pixel alone (DESIGN.md "Extending by map"), so there is no samples_done argument.  With c the
 * pixel's Count, t = targets[i] and cap = camera->samples_per_pixel (footprints: samples_per_pixel -- here only the upper
 * bound on every target):
 *   c == 11                       FINAL: the pixel stopped early; untouched whatever t is
 *   c >= 12 and c < t <= cap      CONTINUED with samples c .. t-1; Count becomes t
 *   c >= 12 and t <= c            LEFT as it is (0 and negative targets included)
 *   c < 11, or t > cap (c != 11)  MALFORMED
 * If the shard holds even one malformed pixel the call continues NO pixel: accum stays as it was, bit for bit, rgb is not
 * written, and the status is reported as for rt_render_extend (RT_ERR_INVALID_ARGUMENT from the host variants, and from the
 * device variants when stats is given; with stats == NULL the unchanged Counts are the caller's evidence).  Otherwise rgb,
 * when given, is written for EVERY pixel of the shard as PixelStats.mean.
 *
 * After any sequence of such calls on a buffer that began as a render at some spp >= 12, every pixel equals that pixel of a
 * direct render at spp = its Count (or is the early-stopped pixel every such render holds).  Every other argument as in the
 * call that made the buffer.
 *
 * Argument checks come before any device call, nothing is written when one fails: cap < 12, cap > 8000000, a NULL targets or
 * accum with pixels to do, a shard of 2^32 pixels or more, and everything the base call rejects.  Empty shards are no-ops
 * returning RT_OK with zeroed stats.
 *
 * stats describe this call alone: samples = the sum of t - c over the continued pixels, pixels = the shard's pixels,
 * pixels_early = the final pixels found; under RT_RENDER_COUNTERS the four counters cover the samples traced.
 *
 * The device variants (d_targets on `device`, like d_accum) follow rt_render_extend_device's contract: stream-ordered scratch,
 * any number of calls in flight, return right after the launch when stats == NULL, the caller's current device left as it was.
 * options->passes is accepted and ignored.  The map must not change until the launch has finished.
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_render_extend_map(const rt_scene *scene, const rt_camera *camera,
                         int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                         int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
                         uint32_t flags, const int32_t *targets, int32_t *accum /* in, out */, uint8_t *rgb /* out, may be NULL */,
                         rt_stats *stats);
int rt_render_extend_map_device(const rt_scene *scene, const rt_camera *camera,
                                int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                                int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows,
                                uint32_t flags, const void *d_targets, void *d_accum, void *d_rgb, void *stream,
                                const rt_render_options *options, rt_stats *stats);
int rt_render_footprints_extend_map(const rt_scene *scene, int32_t device, size_t n, const double *footprints,
                                    int32_t samples_per_pixel /* cap */, int32_t bounce_depth, uint64_t seed, uint64_t stream_base,
                                    uint32_t flags, const int32_t *targets, int32_t *accum /* in, out */, uint8_t *rgb /* out, may be NULL */,
                                    rt_stats *stats);
int rt_render_footprints_extend_map_device(const rt_scene *scene, int32_t device, size_t n, const void *d_footprints,
                                           int32_t samples_per_pixel /* cap */, int32_t bounce_depth, uint64_t seed, uint64_t stream_base,
                                           uint32_t flags, const void *d_targets, void *d_accum, void *d_rgb, void *stream,
                                           const rt_render_options *options, rt_stats *stats);

/* ---- Continuing a batch of views: Scene.render (Scene.fs:157-236) at a higher sample count, for n_views frames in ONE launch ----
 * rt_render_extend and rt_render_extend_map for the buffer of rt_render_views: a turntable previewed at 16 spp and refined to 100, or
 * refined view by view and region by region.  Continuing K views one rt_render_extend_device call each builds K lists, stages the
 * scene K times and idles through K tails; the batch call builds one list, orders it by view, and runs one pass B over all of it.
 * Measured on one MI355X (NOTES.md, round 34): 64 views of a 71x41 frame continued from 16 to 100 spp take 1.81 ms as ONE call and
 * 20.97 ms as 64 rt_render_extend_device calls back to back on one stream (a factor of 11.6); by a map with per-view targets from
 * {16, 40, 100} 1.41 ms against 13.93 ms (9.9).  ONE view of 2401x1601 continued from 100 to 500 spp costs 13 % more kernel time than
 * rt_render_extend_device: the batch form is for many small views.
 *
 * The contract is rt_render_extend's and rt_render_extend_map's, word for word, applied to batch pixel G = v*rows*cols + g (view v,
 * pixel g of its frame); cameras, seeds, geometry and buffers as rt_render_views takes them.
 *   rt_render_views_extend      samples_done >= 12; the target is the cameras' shared samples_per_pixel.  A pixel with
 *                               Count == samples_done is continued with samples samples_done .. target-1 of the stream keyed
 *                               (seed of view v, g, sample); Count == 11 is final; any other Count makes the buffer MALFORMED.
 *                               Afterwards view v is rt_render with cameras[v], seed v and the target count, in every PixelStats word
 *                               and every rgb byte.
 *   rt_render_views_extend_map  targets is [n_views][rows][cols] int32, one per batch pixel; the classes are those of "Extending by
 *                               map" above with cap = the cameras' shared samples_per_pixel.  Every view may have a budget of its own,
 *                               only noisy views or regions may be refined, views that stand at different Counts may be brought to a
 *                               common one.  Afterwards every pixel equals that pixel of a direct render of its view at spp = its
 *                               Count.
 * If ANY view holds even one malformed pixel the call continues NO pixel of ANY view: no byte of accum or rgb is written, and the
 * status is RT_ERR_INVALID_ARGUMENT from the host variants and from the device variants when stats is given; with stats == NULL the
 * untouched buffers are the caller's evidence.  Otherwise rgb, when given, is written for every pixel of every view.
 *
 * Buffers are interchangeable: a slice the batch call continued is a frame's buffer that rt_render_extend_device continues with
 * cameras[v]; K frames of rt_render_device laid out [K][rows][cols][4] are a batch's buffer that these calls continue.
 *
 * Argument checks come before any device call, nothing is written when one fails: everything rt_render_views rejects, with its
 * message (a scene that holds a texture program included: RT_ERR_UNSUPPORTED), then samples_done < 12 or a target below
 * samples_done (uniform), cap < 12 or a NULL targets with n_views > 0 (by map).  n_views = 0, and a target equal to samples_done,
 * are no-ops returning RT_OK with zeroed stats.  `cameras` and `seeds` are HOST pointers and are fully read before the call returns.
 *
 * stats describe this call alone, summed over the views: samples = the samples added, pixels = n_views*rows*cols, pixels_early =
 * the final pixels found, kernel_ms = list building, ordering and pass B; under RT_RENDER_COUNTERS the counters of render(a) plus
 * extend(a -> b) equal render(b)'s.  The device variants follow rt_render_views_device's contract: enqueued on `stream`,
 * stream-ordered scratch, any number of calls in flight, with stats == NULL the call returns right after the launch, the caller's
 * current device is left as it was; d_targets is on `device`, like d_accum, and must not change until the launch has finished.
 * options: as for rt_render_views; `passes` is accepted and ignored.
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
int rt_render_views_extend(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                           int32_t max_width_coord, int32_t max_height_coord,
                           const uint64_t *seeds /* n_views, or NULL: every view uses `seed` */, uint64_t seed,
                           int32_t device, uint32_t flags, int32_t samples_done,
                           int32_t *accum /* in, out: [n_views][rows][cols][4] */, uint8_t *rgb /* out, may be NULL */,
                           rt_stats *stats);
int rt_render_views_extend_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                                  int32_t max_width_coord, int32_t max_height_coord,
                                  const uint64_t *seeds, uint64_t seed,
                                  int32_t device, uint32_t flags, int32_t samples_done,
                                  void *d_accum, void *d_rgb, void *stream,
                                  const rt_render_options *options, rt_stats *stats);
int rt_render_views_extend_map(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                               int32_t max_width_coord, int32_t max_height_coord,
                               const uint64_t *seeds, uint64_t seed,
                               int32_t device, uint32_t flags, const int32_t *targets /* [n_views][rows][cols] */,
                               int32_t *accum /* in, out */, uint8_t *rgb /* out, may be NULL */,
                               rt_stats *stats);
int rt_render_views_extend_map_device(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                                      int32_t max_width_coord, int32_t max_height_coord,
                                      const uint64_t *seeds, uint64_t seed,
                                      int32_t device, uint32_t flags, const void *d_targets,
                                      void *d_accum, void *d_rgb, void *stream,
                                      const rt_render_options *options, rt_stats *stats);

/* ---- Output side (ImageOutput.fs:11-30,163-197) -------------------------------------------------- */
uint8_t rt_gamma_correct(uint8_t b); /* PixelOutput.correct (ImageOutput.fs:11-18) */
/* ImageOutput.writePpm gammaCorrect pixels file (ImageOutput.fs:163-197): P3, no trailing newline. */
int rt_write_ppm(const char *path, const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct);
/* Same bytes into a caller buffer; returns the length needed (excluding NUL) or a negative status. */
int64_t rt_format_ppm(const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct,
                      char *out, size_t out_capacity);

/* ImageOutput.resume's temp-file bytes (ImageOutput.fs:131-161): per pixel `<row>,<col>\n` in ASCII (0 is written as NO
 * digits, ImageOutput.fs:115-129) followed by the three raw colour bytes.  Returns the length, or a negative status. */
int64_t rt_format_pixel_map(const uint8_t *rgb, int32_t rows, int32_t cols, uint8_t *out, size_t out_capacity);
/* ImageOutput.readPixelMap (ImageOutput.fs:46-113): fills rgb_out for every pixel the data names and present_out[r*cols+c]=1
 * (may be NULL); a truncated tail is ignored as in the reference.  Returns the pixel count, or a negative status. */
int64_t rt_parse_pixel_map(const uint8_t *data, size_t n, int32_t rows, int32_t cols, uint8_t *rgb_out, uint8_t *present_out);

/* Png.write gammaCorrect pixels file (ImageOutput.fs:214-251; Program.fs:50 is its caller): the reference hands PixelOutput.toSkia
 * colours (ImageOutput.fs:32-39: R, G, B after PixelOutput.correct or as they are, alpha 255) to Skia's PNG encoder.  Those encoded
 * bytes cannot be reproduced; PNG is lossless, so the PIXELS are pinned -- any conforming decoder returns exactly those colours -- and
 * the container bytes are defined here (csrc/rt_png.h): colour type 2 (8-bit RGB, no alpha channel: a decoder reports the image as
 * opaque), every row Sub-filtered, ONE IDAT of run-length deflate blocks of rt_png_tile_bytes() filtered bytes each.
 * RT_ERR_INVALID_ARGUMENT as rt_write_ppm; RT_ERR_UNSUPPORTED for an image whose worst-case IDAT would not fit a 31-bit chunk length. */
int rt_write_png(const char *path, const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct);
/* Same bytes into a caller buffer; returns the length, or a negative status.  out == NULL: the length only.  A capacity below the
 * length: -RT_ERR_INVALID_ARGUMENT and nothing written.  Works without a GPU. */
int64_t rt_format_png(const uint8_t *rgb, int32_t rows, int32_t cols, int32_t gamma_correct, uint8_t *out, size_t out_capacity);
/* Filtered bytes per tile = per deflate block (RTO_PNG_TILE_BYTES). */
int32_t rt_png_tile_bytes(void);

/* ---- Output side, on the device: the same bytes from an image that is already there (DESIGN.md "Output on the device") ----
 * d_rgb is rows*cols*3 uint8 on `device` (rt_render_device's d_rgb, a torch tensor's data_ptr()); d_rgb and d_out may have any byte
 * alignment.  Everything is enqueued on `stream` (NULL = the null stream) with stream-ordered scratch: any number of calls may be
 * in flight, no call synchronises unless its contract says so, and the caller's current device is left as it was.
 * Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */

/* Upper bound on rt_format_ppm's length: strlen(header) + 12*rows*cols - 1 (every channel three digits; reached exactly by an image
 * whose every byte is >= 100 after gamma).  Pure host arithmetic; negative status on rows/cols <= 0 or more than INT32_MAX pixels. */
int64_t rt_ppm_max_bytes(int32_t rows, int32_t cols);
/* EXACT length of rt_format_pixel_map's output, in closed form (no image needed: lengths depend on (row, col) alone,
 * ImageOutput.fs:115-161).  Negative status as rt_ppm_max_bytes. */
int64_t rt_pixel_map_bytes(int32_t rows, int32_t cols);
/* Upper bound on rt_format_png's length, in closed form: the file of an image whose every tile is a stored block,
 * 68 + rows*(1+3*cols) + 5*ceil(rows*(1+3*cols) / rt_png_tile_bytes()); reached exactly by such an image.  Negative status as
 * rt_ppm_max_bytes, and -RT_ERR_UNSUPPORTED where rt_format_png says so. */
int64_t rt_png_max_bytes(int32_t rows, int32_t cols);

/* PixelOutput.correct (ImageOutput.fs:11-18) over n bytes on the device; d_out may equal d_in.  RT_ERR_INVALID_ARGUMENT for a NULL
 * pointer with n > 0; n = 0 is a no-op. */
int rt_gamma_correct_device(int32_t device, size_t n, const void *d_in, void *d_out, void *stream);

/* rt_format_ppm's bytes (ImageOutput.fs:163-197, PixelOutput.toPpm :20-30; no NUL) and rt_format_pixel_map's bytes
 * (ImageOutput.fs:115-161) from a device image into a device buffer.
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for a NULL d_rgb, rows or
 * cols <= 0, more than INT32_MAX pixels, or a non-NULL d_out with out_capacity == 0; then RT_ERR_NO_DEVICE without a device.
 * The needed length is always stored to d_length (an int64 on the device) when it is given; when `length` is non-NULL the call
 * synchronises the stream and stores it there too.  d_out == NULL: only the lengths are computed.
 * A capacity below the needed length is found ON THE DEVICE, in front of the writing kernel: NO byte of d_out is written, and the
 * call returns RT_ERR_INVALID_ARGUMENT when `length` is given; with length == NULL it returns RT_OK, and d_length > out_capacity and
 * the untouched buffer are the caller's evidence (the pattern of a malformed device pixel list).  Bytes at and beyond the needed
 * length are never written, whatever the capacity. */
int rt_format_ppm_device(int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct,
                         void *d_out /* may be NULL: length only */, size_t out_capacity,
                         void *d_length /* int64 on the device, may be NULL */, void *stream,
                         int64_t *length /* host; may be NULL */);
int rt_format_pixel_map_device(int32_t device, const void *d_rgb, int32_t rows, int32_t cols,
                               void *d_out, size_t out_capacity, void *d_length, void *stream, int64_t *length);

/* rt_format_png's bytes (Png.write, ImageOutput.fs:32-39,214-251) from a device image into a device buffer: exactly the contract of
 * rt_format_ppm_device above -- alignment, d_length, length, d_out == NULL, the capacity found on the device -- and RT_ERR_UNSUPPORTED
 * as rt_format_png, after the argument checks.  Four launches on `stream` (csrc/rt_png_kernels.h). */
int rt_format_png_device(int32_t device, const void *d_rgb, int32_t rows, int32_t cols, int32_t gamma_correct,
                         void *d_out /* may be NULL: length only */, size_t out_capacity,
                         void *d_length /* int64 on the device, may be NULL */, void *stream,
                         int64_t *length /* host; may be NULL */);

/* ImageOutput.writePpm (ImageOutput.fs:163-197) from a device image: format on the device, ONE device-to-host copy of exactly the
 * text, write.  Synchronises.  Arguments are checked (as above, and a NULL path), then the file is opened -- RT_ERR_IO before any
 * device work when that fails -- then the device runs; a short write is RT_ERR_IO, as in rt_write_ppm. */
int rt_write_ppm_device(const char *path, int32_t device, const void *d_rgb, int32_t rows, int32_t cols,
                        int32_t gamma_correct, void *stream);
/* Png.write (ImageOutput.fs:214-251) from a device image: rt_write_ppm_device with rt_format_png_device's bytes -- the same checks in the
 * same order, the file opened before any device work, a device buffer of rt_png_max_bytes, ONE device-to-host copy of exactly the file. */
int rt_write_png_device(const char *path, int32_t device, const void *d_rgb, int32_t rows, int32_t cols,
                        int32_t gamma_correct, void *stream);

/* Scene.render |> ImageOutput.writePpm (Scene.fs:196-236, ImageOutput.fs:163-197): the whole frame rendered, formatted and written;
 * its pixels never visit the host as rgb.  The file is byte for byte rt_format_ppm of rt_render's rgb for the same arguments.
 * Rejects what rt_render rejects about scene, camera, geometry and options (the same check list), and a NULL path; then opens the
 * file (RT_ERR_IO before any device work), renders on the null stream, formats, copies the text out and writes it.
 * stats (may be NULL) as rt_render fills them: kernel_ms = the render kernel; total_ms = the whole call, file included. */
int rt_render_ppm(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                  uint64_t seed, int32_t device, uint32_t flags, int32_t gamma_correct, const char *path,
                  const rt_render_options *options, rt_stats *stats);
/* Scene.render |> Png.write (Program.fs:47-50, ImageOutput.fs:214-251): rt_render_ppm with the PNG; the file is byte for byte
 * rt_format_png of rt_render's rgb for the same arguments. */
int rt_render_png(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                  uint64_t seed, int32_t device, uint32_t flags, int32_t gamma_correct, const char *path,
                  const rt_render_options *options, rt_stats *stats);

/* ---- PNG files of a batch of views (DESIGN.md "PNG files of a batch of views") ----------------------------------------------
 * rt_render_views leaves K frames in one device buffer; these calls turn them into K files without K encodes.  Image v is bytes
 * [v*rows*cols*3, (v+1)*rows*cols*3) of d_rgb, which is n_views*rows*cols*3 uint8 on `device` with any byte alignment (images
 * 1..K-1 start misaligned whenever rows*cols*3 is no multiple of 4).  The output is the K files behind one another with no padding:
 * offsets[v] is the first byte of file v, offsets[n_views] the total length, and bytes [offsets[v], offsets[v+1]) are exactly what
 * rt_format_png(image v, rows, cols, gamma_correct, ...) writes.  Nothing of one image reaches another's file.  The same FOUR launches
 * as one image whatever n_views is (csrc/rt_png_kernels.h): the per-tile kernels run one workgroup per tile of every image, one scan
 * places all tiles of all files, and one workgroup per image writes its head and tail.
 * Refused before any device call, nothing written: n_views < 0, a NULL d_rgb with n_views > 0, rows or cols <= 0, more than INT32_MAX
 * pixels in an image or in the batch, a non-NULL d_out with out_capacity == 0 (RT_ERR_INVALID_ARGUMENT); RT_ERR_UNSUPPORTED where
 * rt_format_png says so for one image.  n_views = 0 is RT_OK: no kernel runs, and 0 is stored to offsets[0] where offsets are asked for.
 * Added symbols only, so RT_ABI_VERSION stays 7. */

/* n_views * rt_png_max_bytes(rows, cols), in closed form.  Negative statuses as rt_png_max_bytes, and -RT_ERR_INVALID_ARGUMENT for
 * n_views < 0 or more than INT32_MAX pixels in the batch. */
int64_t rt_png_views_max_bytes(int32_t n_views, int32_t rows, int32_t cols);
/* rt_format_png_device's contract with the offsets in the place of its length: everything is enqueued on `stream` with stream-ordered
 * scratch and nothing synchronises unless `offsets` is given; the caller's current device is left as it was.  d_out == NULL computes
 * the offsets only.  A capacity below offsets[n_views] is found ON THE DEVICE in front of the writing kernels: no byte of d_out is
 * written, d_offsets still receives the needed values, and the call returns RT_ERR_INVALID_ARGUMENT when `offsets` is given and RT_OK
 * otherwise.  Bytes at and beyond the total are never written. */
int rt_format_png_views_device(int32_t device, const void *d_rgb, int32_t n_views, int32_t rows, int32_t cols,
                               int32_t gamma_correct, void *d_out /* may be NULL: offsets only */, size_t out_capacity,
                               void *d_offsets /* int64[n_views+1] on the device, may be NULL */, void *stream,
                               int64_t *offsets /* host, n_views+1; may be NULL */);
/* The K files written: a device buffer of rt_png_views_max_bytes, the encode, ONE device-to-host copy of exactly offsets[n_views]
 * bytes, then paths[v] for v = 0..K-1, one file open at a time (K may pass the descriptor limit).  Synchronises.  A NULL paths or
 * paths[v] is RT_ERR_INVALID_ARGUMENT before any device work.  The first file that cannot be opened or is written short gives
 * RT_ERR_IO naming that path; the files written before it stay. */
int rt_write_png_views_device(const char *const *paths, int32_t device, const void *d_rgb, int32_t n_views, int32_t rows,
                              int32_t cols, int32_t gamma_correct, void *stream);
/* rt_render_views_device into buffers of the call's own, then the encode, the one copy and the K files: the pixels never visit the
 * host as rgb.  File v is byte for byte rt_format_png of view v of rt_render_views for the same arguments.  Rejects what
 * rt_render_views rejects (the same check list; a scene that holds a texture program is RT_ERR_UNSUPPORTED), then a NULL paths or
 * paths[v].  stats (may be NULL) as rt_render_views fills them, total_ms covering the whole call, files included. */
int rt_render_views_png(const rt_scene *scene, const rt_camera *cameras, int32_t n_views,
                        int32_t max_width_coord, int32_t max_height_coord,
                        const uint64_t *seeds /* n_views, or NULL: every view uses `seed` */, uint64_t seed,
                        int32_t device, uint32_t flags, int32_t gamma_correct, const char *const *paths,
                        const rt_render_options *options, rt_stats *stats);

/* ---- Resuming from a pixel map, on the device (DESIGN.md "Resuming from a pixel map") ------------------
 * Program.fs:39-50 spills the frame as a pixel map (ImageOutput.toPpm), reads it back (ImageOutput.readPixelMap, ImageOutput.fs:46-113),
 * insists that it is complete (ImageOutput.assertComplete, ImageOutput.fs:199-200) and writes the PNG.  These calls are the read-back
 * from bytes that are on the device, and the completion of a partial map by rendering only what it lacks.  The device output stage's
 * contract holds: any byte alignment of d_data, d_rgb and d_present; everything enqueued on `stream` with stream-ordered scratch, so any
 * number of calls may be in flight; the caller's current device left as it was; argument checks before any device call, then
 * RT_ERR_NO_DEVICE.  Added symbols only, so RT_ABI_VERSION stays 7. */

/* The shapes of the parse kernels (csrc/rt_pixel_map.h): bytes per thread, bytes per workgroup, tiles per trip of the scanning workgroup. */
int32_t rt_pixel_map_chunk_bytes(void);
int32_t rt_pixel_map_tile_bytes(void);
int32_t rt_pixel_map_scan_tiles(void);

/* ImageOutput.readPixelMap (ImageOutput.fs:46-113; Program.fs:47) from n_bytes of map on the device, as a scan (csrc/rt_pixel_map.h).
 * Exactly the records rt_parse_pixel_map handles: a record counts iff its third colour byte exists, a truncated tail is ignored, a
 * terminator is any non-digit, an empty digit run is 0, leading zeros of any length are allowed.
 * d_rgb (rows*cols*3) is written for the pixels the data names and every other byte of it is left alone; d_present (rows*cols) is
 * written in full, 0 or 1.  A pixel named more than once keeps its LAST record in file order, whatever the scheduling.  The count is the
 * number of complete records, duplicates included; it goes to d_count (an int64 on the device) when given, and to `count` when given,
 * which synchronises the stream.
 * A malformed map -- a complete record whose row or column is outside the image, or whose digit run exceeds INT32_MAX -- is found ON THE
 * DEVICE, in front of the storing kernels: NOTHING of d_rgb or d_present is written, and the call returns RT_ERR_INVALID_ARGUMENT when
 * `count` is given; with count == NULL it returns RT_OK, and d_count == -RT_ERR_INVALID_ARGUMENT and the untouched buffers are the
 * caller's evidence (the pattern of a malformed device pixel list).  rt_parse_pixel_map differs: by the time it fails it has stored the
 * records in front of the bad one.
 * RT_ERR_INVALID_ARGUMENT for a NULL d_data with n_bytes > 0, a NULL d_rgb or d_present, rows or cols <= 0, more than INT32_MAX pixels;
 * then RT_ERR_UNSUPPORTED for n_bytes > INT32_MAX.  n_bytes == 0 clears d_present and counts 0. */
int rt_parse_pixel_map_device(int32_t device, const void *d_data, size_t n_bytes, int32_t rows, int32_t cols, void *d_rgb, void *d_present,
                              void *d_count /* int64 on the device, may be NULL */, void *stream,
                              int64_t *count /* host; may be NULL */);

/* What ImageOutput.assertComplete (ImageOutput.fs:199-200; Program.fs:49) would throw on: the global pixel indices r*cols + c of the zero
 * bytes of d_present (rows*cols), ascending, as int32 -- the list rt_render_pixels_device takes.  A compaction by scan, no atomic append.
 * The length always goes to d_n (int64 on the device) when given, and to `n` when given, which synchronises.  d_pixels == NULL: the
 * length only.  The capacity (in entries) follows rt_format_ppm_device's rule: one that is too small is found on the device, no entry is
 * written, RT_ERR_INVALID_ARGUMENT when `n` is given, RT_OK and d_n > capacity otherwise. */
int rt_missing_pixels_device(int32_t device, const void *d_present, int32_t rows, int32_t cols, void *d_pixels /* int32, may be NULL */,
                             size_t capacity, void *d_n /* int64 on the device, may be NULL */, void *stream, int64_t *n /* host; may be NULL */);

/* frame[d_pixels[i]] = d_rgb_list[i], three bytes each, for i < n: a rendered pixel list (rt_render_pixels_device's d_rgb) put into a
 * frame of rows*cols*3 bytes -- what makes the map of Program.fs:47 the complete one Program.fs:49 asks for.  An entry outside the frame
 * is found on the device in front of the storing kernel and then NOTHING is written; the call does not synchronise and returns RT_OK, the
 * untouched frame being the caller's evidence.  Of duplicate entries the LAST in list order wins.  n == 0 is a no-op. */
int rt_scatter_pixels_device(int32_t device, size_t n, const void *d_pixels, const void *d_rgb_list, int32_t rows, int32_t cols,
                             void *d_rgb_frame, void *stream);

/* Program.fs:45-49 for an interrupted frame: the map's bytes (host) uploaded and parsed, the pixels it lacks listed, rendered with
 * rt_render_pixels_device and scattered into the frame, which is copied to rgb_out (rows*cols*3, rows = 2*max_height_coord+1).
 * Synchronises.  Rejects what rt_render rejects about scene, camera, geometry and options (the same check list), NULL data with
 * n_bytes > 0, a NULL rgb_out, RT_ERR_UNSUPPORTED for n_bytes > INT32_MAX; a malformed map is RT_ERR_INVALID_ARGUMENT before anything is
 * rendered, and rgb_out is then untouched.
 * For a map whose records come from rt_render's frame with the same scene, camera, geometry and seed -- in any order, any subset,
 * duplicated or truncated -- rgb_out is that frame's rgb byte for byte.  For any other map every named pixel keeps the map's bytes and
 * every other pixel is the frame's.  stats (may be NULL) as rt_render_pixels fills them: pixels = the number rendered, total_ms = the
 * whole call; a complete map renders nothing and leaves every other field zero. */
int rt_resume_pixel_map(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                        uint64_t seed, int32_t device, uint32_t flags, const uint8_t *data, size_t n_bytes, uint8_t *rgb_out,
                        const rt_render_options *options, rt_stats *stats);

/* Program.fs:45-50 with the missing pixels rendered where ImageOutput.assertComplete would throw: the spill at map_path read,
 * resumed on the device as rt_resume_pixel_map does, formatted there (rt_format_png_device / rt_format_ppm_device: the frame never visits
 * the host as rgb) and written to out_path.  The file is byte for byte rt_format_png / rt_format_ppm of rt_resume_pixel_map's rgb_out.
 * The order of checks is rt_render_png's: the arguments, then both files (map_path read whole, out_path opened: RT_ERR_IO before any
 * device work; the two may name one file), then the device. */
int rt_resume_png(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                  uint64_t seed, int32_t device, uint32_t flags, const char *map_path, int32_t gamma_correct, const char *out_path,
                  const rt_render_options *options, rt_stats *stats);
int rt_resume_ppm(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                  uint64_t seed, int32_t device, uint32_t flags, const char *map_path, int32_t gamma_correct, const char *out_path,
                  const rt_render_options *options, rt_stats *stats);

/* ---- Render jobs: live progress, a stop request, a resumable partial frame (DESIGN.md "Render jobs") ----
 * Scene.render ticks its progress bar once per finished row (Scene.fs:196-236, the tick at :232) and ImageOutput.resume spills finished
 * pixels eagerly (ImageOutput.fs:131-161), so a reference run can be watched, interrupted and picked up again.  A render job is the
 * producer half of that on the device: rt_render_device_ex's render of one shard, launched and left running, whose progress the host can
 * read, which the host can ask to stop, and which then leaves a PARTIAL frame -- every pixel either the frame's own, bit for bit, or
 * absent and zero -- together with the presence map that rt_render_job_finish, rt_missing_pixels_device and the pixel-map formatter below
 * take.  The kernels are stoppable variants of the frame passes under symbols of their own (render_job_kernel); they POLL a word of
 * pinned host memory once per work reservation and never wait on the host.  Added symbols and structs only: RT_ABI_VERSION stays 7. */
typedef struct rt_render_job rt_render_job;
typedef struct rt_job_progress {
    uint32_t struct_size;  /* set to sizeof(rt_job_progress) by the caller */
    int32_t state;         /* 0 running, 1 stop requested, 2 finished */
    int64_t pixels_total;  /* n_rows * cols */
    int64_t pixels_final;  /* pixels that have every sample the frame gives them; never decreases, never exceeds pixels_total */
} rt_job_progress;
typedef struct rt_job_result {
    uint32_t struct_size;  /* set to sizeof(rt_job_result) by the caller */
    int32_t complete;      /* 1: every pixel is present */
    int32_t stop_requested;
    int64_t pixels_total, n_present;
} rt_job_result;

/* Scene.render (Scene.fs:196-236) of one shard as a job whose spill ImageOutput.resume (ImageOutput.fs:131-161) would have left.
 * Argument checks are rt_render_device_ex's, from the same check list, then a NULL d_present or `out`, a frame of more than INT32_MAX
 * pixels (rt_render_job_finish lists pixels as int32) and RT_RENDER_COUNTERS (RT_ERR_UNSUPPORTED: there is no counting variant) -- all
 * before any device call, and nothing is written when one fails.  The launch plan is rt_render_device_ex's for the same arguments
 * (blocks of 512 or 768 threads run at 1024).  Everything -- pass A, the ordering, pass B, the finishing kernels -- is enqueued on
 * `stream` up front and the call returns right after the launches.  The scene, the camera's values (copied), d_accum (n_rows*cols*16),
 * d_rgb (n_rows*cols*3, may be NULL) and d_present (n_rows*cols bytes) must outlive the job. */
int rt_render_job_start(const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord, uint64_t seed,
                        int32_t device, int32_t row_first, int32_t row_stride, int32_t n_rows, uint32_t flags, void *d_accum,
                        void *d_rgb /* may be NULL */, void *d_present /* n_rows*cols bytes */, void *stream,
                        const rt_render_options *options, rt_render_job **out);
/* The tick of Scene.fs:232 (the progress bar of Scene.fs:196-236), read instead of called; the count is of the pixels an eager spill
 * (ImageOutput.fs:131-161) would hold: no device call, never blocks.
 * pixels_final never decreases across calls on one job; after rt_render_job_wait it equals n_present. */
int rt_render_job_progress(const rt_render_job *job, rt_job_progress *progress);
/* Asks the job's kernels to reserve no more work (the interrupt of a Scene.fs:196-236 run whose ImageOutput.fs:131-161 spill survives):
 * one store to the polled word.  Idempotent; from any thread, also while another is in rt_render_job_wait.  Work already reserved is
 * finished: at most one unit (fused, pass A) or two ranges (pass B) per wave. */
int rt_render_job_stop(rt_render_job *job);
/* Synchronises the job's stream and reports what is there (Scene.fs:196-236 up to the interrupt; ImageOutput.fs:131-161's spill):
 * d_present written in full, 0 or 1; every present pixel's PixelStats and colour rt_render_device's, bit for bit; every absent
 * pixel's zero.  stats (may be NULL): pixels = n_present, samples = every sample traced (those of discarded pixels included),
 * kernel_ms, total_ms; the other fields zero.  May be called again: the same answer. */
int rt_render_job_wait(rt_render_job *job, rt_job_result *result, rt_stats *stats);
/* Picks the frame up again (Program.fs's resume of ImageOutput.fs:131-161's spill; the pixels Scene.fs:196-236 had not reached): after
 * rt_render_job_wait (else RT_ERR_INVALID_ARGUMENT) lists the absent pixels, renders them as a pixel list on `stream`, scatters
 * PixelStats and colour and sets every present byte.  Synchronises.  Afterwards d_accum and d_rgb are rt_render_device's byte for byte,
 * whenever and wherever the stop landed.  A complete job renders nothing.  stats (may be NULL) as rt_render_pixels fills them. */
int rt_render_job_finish(rt_render_job *job, void *stream, rt_stats *stats);
/* Waits for the job's stream if nobody has, then frees the job (Scene.fs:196-236's run is over; ImageOutput.fs:131-161's buffers are the
 * caller's).  NULL is a no-op. */
void rt_render_job_destroy(rt_render_job *job);
/* Test hooks (Scene.fs:196-236 stopped at a chosen unit; ImageOutput.fs:131-161's spill made deterministic).  A budget for the NEXT job
 * this thread starts: exactly units [0, limit_a) of the fused kernel / pass A and exactly list entries [0, limit_b) of pass B are
 * rendered; -1 = no limit.  Consumed by that job. */
int rt_dev_set_job_limits(int64_t limit_a, int64_t limit_b);
/* The last job this thread waited for: passes, chunk (pixels per unit of the fused kernel / pass A), units_a, n_list, done_a, done_b,
 * block, textured (Scene.fs:196-236's schedule and ImageOutput.fs:131-161's prefix; csrc/rt_job_plan.h defines the present set from these). */
int rt_dev_last_job_plan(int64_t out[8]);

/* ImageOutput.resume's records (ImageOutput.fs:131-161, the record at :145-155; the spill a Scene.fs:196-236 run leaves when it is
 * interrupted) for the PRESENT pixels only, in row-major order: rt_format_pixel_map restricted to present[r*cols + c] != 0.  With every
 * byte of `present` set the output is rt_format_pixel_map's.  Returns the length; writes when out is given and out_capacity holds it. */
int64_t rt_format_pixel_map_present(const uint8_t *rgb, const uint8_t *present, int32_t rows, int32_t cols, uint8_t *out, size_t out_capacity);
/* ... on the device (ImageOutput.fs:131-161 over a Scene.fs:196-236 partial frame): lengths, scan and write with the output stage's scan
 * kernels, byte for byte the host formatter's.  rt_format_ppm_device's capacity rule: a buffer that is too small is found on the
 * device, no byte is written, RT_ERR_INVALID_ARGUMENT when `bytes` is given, RT_OK and d_bytes > out_capacity otherwise. */
int rt_format_pixel_map_present_device(int32_t device, const void *d_rgb, const void *d_present, int32_t rows, int32_t cols, void *d_out,
                                       size_t out_capacity, void *d_bytes /* int64 on the device, may be NULL */, void *stream,
                                       int64_t *bytes /* host; may be NULL */);

/* ---- Runtime ------------------------------------------------------------------------------------- */
int rt_device_count(void);         /* 0 when no HIP device is visible (never an error) */
const char *rt_last_error(void);   /* thread-local message of the last failing call */
int rt_abi_version(void);
/* sizeof of the ABI structs as compiled: 0 rt_hittable, 1 rt_texture, 2 rt_camera, 3 rt_scene_info, 4 rt_stats,
 * 5 rt_render_options, 6 rt_scene_options, 7 rt_tune_info, 9 rt_path_outputs, 13 rt_surface_outputs (bindings check their mirrors). */
size_t rt_abi_sizeof(int which);
/* Byte offset of field number `field` (declaration order, from 0) of struct `which` (numbering of rt_abi_sizeof), or
 * (size_t)-1 past the last field: a binding in another language asserts its own layout against these at start-up
 * (the F# StructLayout(Sequential) mirrors; ray-tracing-fsharp_amd/_lib.py: the ctypes ones). */
size_t rt_abi_offsetof(int which, int field);
/* Tunables of the render kernel: threads per workgroup (256, 512, 768 or 1024) and pixels per wave work unit (<= 64).
 * 0 keeps the default.  Process-wide DEFAULTS for calls that pass no rt_render_options; meant for bench sweeps. */
int rt_set_launch_config(int32_t block_threads, int32_t chunk_pixels, int32_t blocks_per_cu);
/* Lane-scheduling thresholds of the render kernel (DESIGN.md "Kernel"): a stage yields once `yield_lanes` lanes wait for
 * another stage; idle lanes are refilled once `refill_lanes` are idle.  0 keeps the default.  Results never depend on them. */
int rt_set_schedule(int32_t yield_lanes, int32_t refill_lanes);
/* Which binary tree over the Leaf boxes the device walks, for scenes created AFTERWARDS.  RT_WALK_TREE_SAH (default): a
 * surface-area-heuristic build, ~14 % fewer box tests per ray on the reference's scenes; RT_WALK_TREE_REFERENCE:
 * BoundingBoxTree.make's own tree (BoundingBoxTree.fs:9-43) with Array.sortBy taken as a STABLE sort, i.e. the oracle's
 * tree: the box-test count then equals the oracle's.  (.NET's Array.sortBy is an unstable introsort and every small sphere
 * of the final scene ties on Min.y, so the real reference's tree -- and its count -- may differ from both.)  The hit a ray
 * returns -- hence every pixel -- is the same bit for bit under every such tree (rt_scene.h "the tree the device WALKS");
 * only the aabb_tests statistic differs. */
int rt_set_walk_tree(int32_t kind);
/* 1: always the fused kernel; 2: always two passes (phase 1 + decision, cost-ordered phase 2); 0: choose by shard size.
 * Results never depend on it. */
int rt_set_passes(int32_t passes);
/* Capacity of a wave's pool of parked paths: a path whose hit is neither an untextured light source nor an untextured
 * Lambert sphere is set aside (88 bytes of state, in global memory) and shaded later together with others of its kind
 * (DESIGN.md "Kernel").  0 = default (64), -1 = never park (such paths are shaded in their lane).  Results never depend on it. */
int rt_set_park(int32_t park_lanes);
/* Diagnostic: wave-level stage executions of the calling THREAD's last render that asked for stats with
 * RT_RENDER_COUNTERS set: {refill stages, node-loop trips, leaf stages, shade stages, lanes refilled, lanes shaded, sum of
 * wave lifetimes and first-start-to-last-end span (both in 100 MHz ticks), waves launched, general-reflection stages, lanes in them,
 * lanes parked, shader-clock cycles summed over the waves inside the refill / general-reflection / walk / shade stages}. */
int rt_last_stage_stats(uint64_t out[16]);
/* Diagnostic: the launch plan (csrc/rt_launch_plan.h) of the calling THREAD's last launch -- a render shard, rt_scene_tune's probe
 * a ray list, a footprint list, a pixel list or a camera-hit list; of rt_render_frame, its last device's -- as the library gathered its inputs and executed its outputs.  Read-only
 * host bookkeeping: no device work, nothing launched depends on it.  Words, under the names tests/c/launch_plan_table.cpp reads
 * and prints:
 *   [0]      1 once this thread has planned a launch (all words are 0 before)
 *   [1..21]  inputs: kind (0 frame shard, 1 traceRays list, 2 hitObject list, 3 footprint list: n pixels,
 *            4 pixel list: n pixels, 5 camera hits: n list entries, spp = n_samples, 6 batch of views: n views of n_rows rows each, run by
 *            the render_views kernels at the frame passes' mode numbers, 7 camera hits over a batch of views: kind 5's words, n the
 *            shared list's entries, planned over n_views * n * n_samples rays and run by the camera_hits_views kernels at mode 14)
 *            lds_total lds32_total n_nodes n_obj has_tex
 *            s_block s_chunk s_bpc s_yield s_refill s_passes s_park (the resolved settings, 0 = "the plan decides") count log
 *            n_rows max_w spp n cu_count per_cu (what the occupancy query answered, before blocks_per_cu)
 *   [22..34] q_lds q_count q_block q_mode q_tex q_lds_bytes two_pass pairs list sort pool waves error
 *   [35..48] the fused or ray-list kernel (F_), [49..62] pass A (A_), [63..76] pass B (B_), each: mode grid lds_bytes chunk park
 *            park_l park_l_lds lds_node_bytes lds_node_thr yield leaf_wait refill k total_waves.  F_ is what ran unless two_pass;
 *            A_ and B_ are filled only with two_pass and no error.
 *   [77]     first_sample: 0 for a fresh render; for an extension (rt_render_extend*, rt_render_footprints_extend*) its samples_done;
 *            for camera hits (kind 5, mode 14, planned as a ray list of n * n_samples rays with units of F_chunk entries) sample_first.
 *            An extension reports kind 0, 3 or 4 (rt_render_pixels_extend*), two_pass 1, pairs and sort 0, every A_ word 0 (no pass A is launched) and pass B as
 *            the same job gets it with passes = 2.
 *   [78]     1 for an extension by map (rt_render_extend_map*, rt_render_footprints_extend_map*), else 0.  Such a launch reports
 *            first_sample 12 and spp = the cap (it is planned as the extension 12 -> cap) and pass B's mode as 9 (frame) or 10
 *            (footprints), its lds_bytes and chunk following from the map variant's larger per-wave scratch.
 *   [79]     n_views of camera hits over a batch of views (kind 7), else 0.
 * A call that fails before its plan is complete (bad arguments, no kernel built for the launch, occupancy 0) leaves the previous
 * launch's report in place: read it after a call that returned RT_OK.
 * An added diagnostic symbol only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7. */
#define RT_LAUNCH_PLAN_WORDS 80
int rt_dev_last_launch_plan(int64_t out[RT_LAUNCH_PLAN_WORDS]);

/*
 * ---- Device unit hooks ---------------------------------------------------------------------------
 * Run ONE device function of the path over n inputs on the GPU, so that the reference's unit tests
 * (the .fs files under RayTracing.Test) can be replayed against the very code the render kernel inlines.
 * All pointers are HOST pointers; the hooks copy in, launch, copy out.
 */
/* FloatProducer (Float.fs:14-76): from state[4] produce n doubles with Get(). */
int rt_dev_float_producer(int32_t device, const uint32_t state[4], int32_t n, double *out);
/* Stream seeding (DESIGN.md "Seeding"): state for (seed, pixel, sample). */
int rt_dev_stream_state(int32_t device, uint64_t seed, int32_t n, const uint64_t *pixel, const uint32_t *sample,
                        uint32_t *state_out /* n*4 */);
/* BoundingBox.inverseDirections + hits (BoundingBox.fs:25-94). rays: n*6 (origin, unit dir); boxes: n*6 (min xyz, max xyz). */
int rt_dev_bbox_hits(int32_t device, int32_t n, const double *rays, const double *boxes, int32_t *hit_out);
/* The timed kernel's node loop does not run BoundingBox.hits on the boxes ABOVE the leaves: it runs a conservative
 * single-precision filter F with hits(box) => F(box) (csrc/rt_device.h, "the node loop of the timed variant"), and the leaf pass
 * then makes the Leaf's own BoundingBox.hits exactly -- the set of spheres tested is the reference's (Scene.fs:39-60).  This hook
 * runs both on n (ray, box) pairs: out[i] bit 0 = the exact test, bit 1 = F in the loop's own instruction forms, bit 2 = F as
 * compiled C++.  Boxes are rounded outward to single precision as the scene image does; bmax (>= 0) enlarges the margin's scale
 * beyond the batch's largest |coordinate| (the scene image uses the largest |coordinate| of its tree). */
int rt_dev_bbox_filter(int32_t device, int32_t n, const double *rays, const double *boxes, double bmax, int32_t *out);
/* The timed kernel walks the tree ONCE per pixel for all of the pixel's camera rays (Scene.traceOnce, Scene.fs:129-144): with the
 * pyramid from the eye through the pixel's patch of the viewport it collects the Leaves any of those rays can reach (at most four;
 * csrc/rt_device.h, pixel_candidates), and a camera ray then starts with those Leaves queued for their exact tests instead of
 * walking.  This hook returns that set for n pixels given as (row, col) pairs in the reference's coordinates (row = maxH - r - 1,
 * col = c - maxW, Scene.fs:219,226): leaves_out[i*4 .. i*4+3] = hittable indices (input order of rt_scene_create), -1 padded;
 * leaves_out[i*4] = -2 when the pixel's camera rays walk the tree as all other rays do (more than four Leaves in reach, more than
 * two for a scene of 16384 objects or more, or a degenerate pyramid).  Any scene: one that does not fit the LDS is read through
 * the timed kernel's global-memory view, with the queue words of its layout (16-bit entries below 16384 objects, full-width ones
 * from there on). */
int rt_dev_pixel_candidates(int32_t device, const rt_scene *scene, const rt_camera *camera, int32_t max_width_coord, int32_t max_height_coord,
                            int32_t n, const int32_t *row_col, int32_t *leaves_out);
/* Sphere.firstIntersection (Sphere.fs:349-386). spheres: n*4 (centre xyz, radius). t_out = NaN when ValueNone. */
int rt_dev_sphere_first_intersection(int32_t device, int32_t n, const double *rays, const double *spheres, double *t_out);
/* InfinitePlane.intersection (InfinitePlane.fs:125-136). planes: n*6 (point, unit normal). */
int rt_dev_plane_intersection(int32_t device, int32_t n, const double *rays, const double *planes, double *t_out);
/* Pixel.combine / Pixel.darken (Pixel.fs:136-151). a,b: n*3 bytes; albedo: n. */
int rt_dev_pixel_combine(int32_t device, int32_t n, const uint8_t *a, const uint8_t *b, uint8_t *out);
int rt_dev_pixel_darken(int32_t device, int32_t n, const uint8_t *p, const double *albedo, uint8_t *out);
/* Hittable.Reflection (Hittable.fs:8-12 -> Sphere.fs:150-300 | InfinitePlane.fs:43-99) for hittable `index` of the
 * scene (index into the array given to rt_scene_create).  Per item: ray_in n*6, colour_in n*3, strike n*3,
 * rng_state n*4 (in/out).  Outputs: absorbed[n] (1 = ValueSome colour), colour_out n*3, ray_out n*6. */
int rt_dev_reflection(int32_t device, const rt_scene *scene, int32_t n, const int32_t *index,
                      const double *ray_in, const uint8_t *colour_in, const double *strike,
                      uint32_t *rng_state, int32_t *absorbed, uint8_t *colour_out, double *ray_out);
/* Scene.hitObject (Scene.fs:62-91): hit_index = index into the rt_scene_create array or -1; strike n*3; counters optional (n*2: aabb, prim). */
int rt_dev_hit_object(int32_t device, const rt_scene *scene, int32_t n, const double *rays,
                      int32_t *hit_index, double *strike, uint32_t *counters);
/* The same through the render kernel's timed route: scene staged into LDS, the hand-written node loop with its per-lane queue of
 * pending leaf tests, leaf passes between its runs, the unbounded objects last (RT_ERR_UNSUPPORTED when the scene does not fit the LDS). */
int rt_dev_hit_object_lds(int32_t device, const rt_scene *scene, int32_t n, const double *rays, int32_t *hit_index, double *strike);
/* Scene.traceRay (Scene.fs:93-114) from White for given rays and RNG states. colour_out n*3. */
int rt_dev_trace_ray(int32_t device, const rt_scene *scene, int32_t bounce_depth, int32_t n, const double *rays,
                     uint32_t *rng_state, uint8_t *colour_out);
/* Texture lookup incl. Sphere.planeMapInverse (Sphere.fs:55-61, Texture.fs:50-67): uv_out n*2, colour_out n*3. */
int rt_dev_texture_colour_at(int32_t device, const rt_scene *scene, int32_t texture, int32_t n, const double *points,
                             double *uv_out, uint8_t *colour_out);
/* IEEE-754 conformance probes of the device arithmetic the path relies on: op 0: 1.0/x, 1: sqrt(x), 2: rint(x),
 * 3: x/y, 4: pow5(x) = Math.Pow(x, 5.0) (Sphere.fs:290), 5: the path's sqrt for operands > 1e-8, 6: its 1.0/sqrt(x) for
 * operands >= 1e-8 (both must equal the correctly rounded results), 7: Math.Acos(x), 8: Math.Sin(x), 9: Math.Atan2(x, y) as the
 * texture maps use them (Sphere.fs:59-60, Texture.fs:58): the correctly rounded values (csrc/rt_trig.h).
 * a,b: n doubles (b may be NULL for unary ops). */
int rt_dev_arith(int32_t device, int32_t op, int32_t n, const double *a, const double *b, double *out);

/* ---- BoundingBoxTree.make's tree on the device (BoundingBoxTree.fs:9-43; csrc/rt_tree_plan.h, csrc/rt_tree_kernels.h; DESIGN.md "The
 * reference tree on the device").  Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7.
 *
 * The tree's shape is a function of the number of boxes alone: a node over c boxes has children over c/2 + 1 and c - c/2 - 1 boxes
 * (BoundingBoxTree.fs:28-29), two boxes make two Leaves without sorting, so the tree has 2n - 1 nodes, and in pre-order skip[me] =
 * me + 2c - 1.  rt_tree_nodes: 2n - 1, 0 for n == 0.  rt_tree_depth: the nodes on the longest path from the root (BoundingBoxTree.fs:9-43).
 * rt_tree_lds_boxes: the largest segment the device build finishes in one workgroup's LDS (a whole build of at most that many boxes
 * is one launch behind the NaN check). */
int64_t rt_tree_nodes(size_t n);
int32_t rt_tree_depth(size_t n);
int32_t rt_tree_lds_boxes(void);
/* BoundingBoxTree.make (BoundingBoxTree.fs:9-43) over the caller's boxes, Array.sortBy defined stable (DESIGN.md "Tree shape").
 * boxes: n*6 doubles (minx,maxx,miny,maxy,minz,maxz), the form of rt_scene_get_tree.  Outputs, any may be NULL:
 * skip, prim (input index of a Leaf's box, -1 for a Branch): rt_tree_nodes(n) int32 each; node_boxes: rt_tree_nodes(n)*6 doubles;
 * order: n int32, the depth-first leaf order (the rank table of rt_scene_create).
 *
 * rt_tree_make_host is the host builder of rt_scene_create on these boxes and touches no device: the yardstick for inputs a sphere
 * cannot express (signed zeros, infinities, arbitrary inverted boxes).  rt_tree_make stages the boxes, runs rt_tree_make_device on the
 * null stream and copies back.  rt_tree_make_device builds on `stream` (NULL = the null stream) from and into device memory, with
 * stream-ordered scratch (any number of builds may be in flight), and returns after the stream has finished the build.  All three give
 * the same four arrays, the boxes bit for bit (the sign of a zero in a Branch box included: BoundingBox.mergeTwo keeps the later
 * operand of a tied minimum and the earlier one of a tied maximum, BoundingBox.fs:96-108).
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for NULL boxes with n > 0,
 * a device pointer that is not 8-byte (boxes, node_boxes) or 4-byte (skip, prim, order) aligned; then RT_ERR_UNSUPPORTED for
 * n > 4,500,000 (the scene's own limit).  n == 0 is a no-op RT_OK.  A NaN coordinate has no order: RT_ERR_INVALID_ARGUMENT, found on
 * the host by rt_tree_make_host and on the device by the other two -- in front of the build, on the same stream, with no output written.
 * RT_ERR_NO_DEVICE without a GPU (not rt_tree_make_host).  The caller's current device is left as it was. */
int rt_tree_make_host(size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes, int32_t *order);
int rt_tree_make(int32_t device, size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes, int32_t *order);
int rt_tree_make_device(int32_t device, size_t n, const void *d_boxes, void *d_skip, void *d_prim, void *d_node_boxes,
                        void *d_order, void *stream);
/* rt_scene_create_ex with BoundingBoxTree.make's tree (BoundingBoxTree.fs:9-43), and with it the ranks, taken from the device build on
 * `device`; everything after the tree -- object table, walk tree, device image -- is the same host code, and the scene is the same scene:
 * rt_scene_get_info, _get_tree, _get_walk_tree, _get_filter_tree and every render are identical.  With fewer than 3 bounded spheres, or a
 * NaN box coordinate, the host builder is used (the device is still entered: RT_ERR_NO_DEVICE without a GPU, before anything else).
 * Measured on one MI355X against the host builder on 16 CPUs (same section): the crossover is at about 1e4 spheres -- the tree
 * takes 1.2 ms instead of 0.25 ms at 485 spheres, 4.5 ms on both routes at 1e4, 7 instead of 43 ms at 1e5 and 25 ms instead of 1.1-1.3 s at
 * 1e6, where creating the scene goes from 2.96 s to 1.98 s (the surface-area build, still on the host, is 1.56 s of that). */
int rt_scene_create_gpu_tree(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                             const rt_scene_options *options, int32_t device, rt_scene **out);

/* ---- The tree the device walks, built on the device (csrc/rt_walk_plan.h, csrc/rt_walk_kernels.h; DESIGN.md "The walk tree on the
 * device").  Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7.
 *
 * The surface-area build of rt_scene_create (RT_WALK_TREE_SAH, the arms without probe rays) over the caller's boxes: a node over n boxes
 * holds their union; in pre-order node `me` has its left child at me + 1 over k boxes, its right child at me + 2k over n - k, and
 * skip[me] = me + 2n - 1.  k is chosen by cost (csrc/rt_walk_plan.h: a full sweep up to 4096 boxes, 32 centroid bins above, halving from
 * depth 48 on), so the shape depends on the boxes; there are always rt_tree_nodes(n) nodes.
 * boxes: n*6 doubles (minx,maxx,miny,maxy,minz,maxz).  Outputs, any may be NULL: skip, prim (input index of a Leaf's box, -1 for a
 * Branch): rt_tree_nodes(n) int32 each; node_boxes: rt_tree_nodes(n)*6 doubles.
 *
 * rt_walk_tree_make_host is the host builder of rt_scene_create on these boxes and touches no device: the yardstick.
 * rt_walk_tree_make stages the boxes, builds on the null stream and copies back.  rt_walk_tree_make_device builds on `stream` (NULL = the
 * null stream) from and into device memory with stream-ordered scratch (any number of builds may be in flight) and returns after the
 * stream has finished the build; it waits for the stream once per level of nodes above 4096 boxes.  All three give the same skip and
 * prim, and boxes that are equal as numbers: a Branch box of the device build has +0.0 for either zero, where the host builder's sign
 * depends on the order its std::nth_element leaves (no cost, comparison, split or render depends on it).  The two device routes agree
 * byte for byte, and so do two builds of one input.
 *
 * Argument checks come before any device call, nothing is written when one fails: RT_ERR_INVALID_ARGUMENT for NULL boxes with n > 0 or a
 * device pointer that is not 8-byte (boxes, node_boxes) or 4-byte (skip, prim) aligned; then RT_ERR_UNSUPPORTED for n > 4,500,000.
 * n == 0 is a no-op RT_OK.  A coordinate that is not finite: RT_ERR_INVALID_ARGUMENT (a scene never builds this tree over such boxes),
 * found on the host by rt_walk_tree_make_host and on the device by the other two -- in front of the build, on the same stream, with no
 * output written.  RT_ERR_NO_DEVICE without a GPU (not rt_walk_tree_make_host).  The caller's current device is left as it was. */
int rt_walk_tree_make_host(size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes);
int rt_walk_tree_make(int32_t device, size_t n, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes);
int rt_walk_tree_make_device(int32_t device, size_t n, const void *d_boxes, void *d_skip, void *d_prim, void *d_node_boxes, void *stream);
/* rt_scene_create_gpu_tree with the walk tree taken from the device build as well: both trees come from `device`, everything else is the
 * same host code, and the scene is the same scene -- rt_scene_get_info, _get_tree, _get_walk_tree (boxes equal as numbers),
 * _get_filter_tree and every render are identical, before and after rt_scene_tune*.  The host builders are used exactly where they are
 * otherwise: RT_WALK_TREE_REFERENCE (no surface-area tree at all), fewer than 3 bounded spheres, a box coordinate that is not finite.
 * Measured on one MI355X (DESIGN.md "The walk tree on the device"): the walk tree takes 17.7 ms instead of 1.83 s at 1e6 boxes, 9.2 instead of
 * 160 ms at 1e5, 6.8 instead of 13.4 ms at 1e4 and 1.32 instead of 0.43 ms at 485; creating a scene of 1e6 spheres goes from 1.98 s
 * (rt_scene_create_gpu_tree) to 0.51 s.  The crossover is at about 8000 spheres: below it rt_scene_create(_ex) is the faster route. */
int rt_scene_create_gpu_trees(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                              const rt_scene_options *options, int32_t device, rt_scene **out);

/* ---- Scene.make from hittables in device memory (Scene.fs:15-28; csrc/rt_scene_plan.h, csrc/rt_scene_kernels.h; DESIGN.md "Scene.make on
 * the device").  Added symbols only -- no struct, field or existing symbol changed, so RT_ABI_VERSION stays 7.
 *
 * d_hittables: n_hittables rt_hittable records in `device`'s memory, 8-byte aligned; they are read, not kept (the scene holds a copy of its
 * own).  textures: a HOST array, as for rt_scene_create (at most 254 records, copied the same way).  The build runs on `stream` (NULL = the
 * null stream) with stream-ordered scratch, so any number of builds may be in flight, and the call returns after the stream has finished
 * it.  The scene is the scene rt_scene_create_gpu_trees returns for the same records: every rt_scene_get_*, every render, the rt_hit_objects
 * family (indices into d_hittables), rt_scene_tune* and rt_scene_destroy behave identically.
 *
 * On the device, on `stream`: the check of every hittable; Array.partition with order kept on both sides (a scan of the bounded flags);
 * Sphere.make's boxes; both trees, by the builds of rt_tree_make_device and rt_walk_tree_make_device from and into device memory with no
 * staging; the ranks (the reference tree's depth-first leaf order, which that build gives as `order`) and the object table; the leaf boxes
 * in rank order as the walk build's input; the whole image node | geo | meta | node32 | mat, its node32 section in the stable order by
 * depth (a difference array over the pre-order ranges of the Branches, a scan, and a radix sort on the depth alone); bmax and the inputs
 * of leaf_box_implied.  Read back: the counts, the error word, the NaN / not-finite flags, bmax, the largest radius and the radius flag,
 * the largest depth -- O(1) bytes -- and the walk build's per-level counters.  The device's copy of the scene (image, object table,
 * texture records, texels) is installed directly: nothing proportional to the scene goes to the host in this call or in renders on `device`.
 *
 * Fetched lazily, once, under the scene's lock: the host's copy of the hittables, both trees, the leaf boxes, the object table and the
 * image.  What needs it fetches it: rt_scene_get_tree, _get_walk_tree, _get_filter_tree, rt_scene_tune* (where they rebuild the tree), the
 * first use of the scene on ANOTHER device, and the rt_dev_* hooks that translate hittable indices.  rt_scene_get_info does not.
 *
 * Where the host code still runs: the texture records (O(textures)); the empty scene; and a NaN box coordinate, which has no order --
 * found on the device, after which the records are downloaded and the scene is rt_scene_create_gpu_trees' own (slow for many records, but
 * the same scene; it has its host copy from the start).  With fewer than 3 bounded spheres the tree is trivial and is written directly on
 * the device (so a scene of planes and unbounded spheres alone never passes through the host either).  Boxes that are not finite but
 * ordered walk the reference tree, as on every route, and are still encoded on the device.
 *
 * Refusals.  Argument checks come before any device call: RT_ERR_INVALID_ARGUMENT for NULL d_hittables with n_hittables > 0, NULL textures
 * with n_textures > 0, d_hittables not 8-byte aligned, NULL out, an options->walk_tree that is not a creation option.  RT_ERR_NO_DEVICE
 * without a GPU.  Then the textures' own refusals, and for the records the status and rt_last_error() text of rt_scene_create_ex: with
 * several bad hittables the smallest index is reported, with the first failing check of that hittable (one minimum over index * 8 +
 * reason); then RT_ERR_UNSUPPORTED for more than 4,500,000 bounded spheres or 16,000,000 objects.  *out is written on success only. */
int rt_scene_create_device(int32_t device, const void *d_hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                           const rt_scene_options *options, void *stream, rt_scene **out);

/* ---- Test hooks of the device-made scene ---- */
/* The image bytes as `device` holds them (for a scene made on the host: the host's image once that device has its copy) and the
 * thirteen words of the kernel's SceneOffsets (node, geo, meta, node32, mat, total, lds_total, lds32_total, n_nodes, n_bounded,
 * n_unbounded, the bits of bmax, box_implied; the rest 0).  *bytes: the image's size; out may be NULL to ask for it, offsets may be NULL. */
int rt_dev_scene_image(const rt_scene *scene, int32_t device, void *out, size_t cap, size_t *bytes, uint32_t offsets[16]);
/* The device encoder alone (the depth, the order by depth and the records) on the scene's own walk tree, object table and hittables, staged
 * up: the bytes encode_image gives, also for the n-ary tree of a tuned scene.  out may be NULL to ask for *bytes. */
int rt_dev_encode_image(int32_t device, const rt_scene *host_made, void *out, size_t cap, size_t *bytes);
/* The same with the order by depth sorted in passes of digit_bits bits (1 .. 8; the product's are 8 wide, so only a tree of 256 levels or
 * more takes a second pass there): with narrow digits a tree of a few dozen levels runs the later passes -- the same bytes. */
int rt_dev_encode_image_radix(int32_t device, const rt_scene *host_made, int32_t digit_bits, void *out, size_t cap, size_t *bytes);
/* 1 when the host holds its copy of the scene's arrays (always, for a scene made on the host), 0 while they are still on the device.
 * (Scenes whose texels were placed on a device -- "Image textures from device memory" below -- report 0 until those are fetched too.) */
int rt_dev_scene_has_host_mirror(const rt_scene *scene);

/* ---- LoadImage.fromResource (RayTracing.App/LoadImage.fs:9-18): a baseline JPEG to the bitmap ParameterisedTexture.ofImage takes ----
 * The reference hands the file to SKBitmap.Decode, which is libjpeg-turbo; its decode of a baseline file is integer arithmetic
 * throughout (Huffman, jpeg_idct_islow, "fancy" upsampling, the fixed-point YCbCr tables), and csrc/rt_jpeg.h restates it bit for bit.
 * The bitmap: `height` rows, top first, of `width` pixels as R, G, B bytes -- rt_texture.texels' layout.  EXIF orientation is ignored.
 *
 * Accepted: SOF0, 8-bit samples, 1 component or 3 (YCbCr) in ONE interleaved scan, 8-bit quantisation tables, sampling 4:4:4, 4:2:2
 * (2x1) and 4:2:0 (2x2), with or without restart markers.  RT_ERR_UNSUPPORTED: progressive and every other SOFn, arithmetic coding,
 * 12-bit samples, 4 components, multiple scans, other sampling factors, 16-bit quantisers, a 3-component file whose Adobe marker names
 * a transform other than 1, more than 2^28 entropy-coded bytes (2^31 - 1 with the restart markers).  RT_ERR_INVALID_ARGUMENT, with rt_last_error() naming what and where:
 * NULL arguments, no SOI, a segment that runs past the end, a table or component referenced before it is defined, a zero dimension,
 * more than INT32_MAX pixels, a capacity below width * height * 3; and for the entropy-coded data: a code that is not in its table, a
 * coefficient index past 63, or a number of blocks -- in front of any restart marker, or in all -- other than the frame and the restart
 * interval call for (a stream that ends early is one), or restart markers that do not number one between every two intervals.  No byte at or behind data + n is read, and on any error nothing is written.
 *
 * Added symbols and two added structs only -- no existing struct, field or symbol changed, so RT_ABI_VERSION stays 7. */
#define RT_JPEG_GREY 0
#define RT_JPEG_444 1
#define RT_JPEG_422 2
#define RT_JPEG_420 3
typedef struct rt_jpeg_info {
    uint32_t struct_size;     /* sizeof(rt_jpeg_info), set by the caller */
    int32_t width, height;
    int32_t components;       /* 1 or 3 */
    int32_t sampling;         /* RT_JPEG_GREY .. RT_JPEG_420 */
    int32_t restart_interval; /* MCUs; 0: none */
    int64_t entropy_bytes;    /* the scan's entropy-coded bytes as they are in the file (stuffing and restart markers included) */
} rt_jpeg_info;
typedef struct rt_jpeg_stats {
    uint32_t struct_size;       /* sizeof(rt_jpeg_stats), set by the caller */
    int32_t subsequence_bytes;  /* clean-stream bytes per thread of the synchronising rounds */
    int64_t subsequences, rounds, decodes, blocks, boundaries;
    double total_ms;            /* wall time of the call */
} rt_jpeg_stats;
/* The header alone (the scan's entropy-coded bytes are measured, not decoded).  Works without a GPU. */
int rt_jpeg_get_info(const uint8_t *data, size_t n, rt_jpeg_info *out);
/* The decode on the host, sequentially.  Works without a GPU and with no device visible. */
int rt_decode_jpeg(const uint8_t *data, size_t n, uint8_t *rgb, size_t capacity);
/* The decode on `device` into d_rgb (device memory of `capacity` bytes, any alignment); `data` is HOST memory, where files come from.
 * The header is parsed on the host -- its refusals come before any device call -- and the tables and the entropy-coded bytes go up;
 * the rest is kernels on `stream` (csrc/rt_jpeg_kernels.h): the byte stream is cleaned, decoded in subsequences from guessed states
 * that are synchronised in rounds (the host reads one word per round between batches of launches; no workgroup waits for another),
 * placed, and turned into samples and colours.  Scratch is stream-ordered; any number of decodes may be in flight.  Errors of the
 * entropy-coded data are found on the device, in front of the one kernel that writes d_rgb: nothing of d_rgb is written.  With
 * stats == NULL the call returns RT_OK after its last launch with nothing promised about such a file; with stats it synchronises and
 * returns what rt_decode_jpeg returns for the same bytes, text included.  RT_ERR_NO_DEVICE without a GPU (not rt_decode_jpeg). */
int rt_decode_jpeg_device(int32_t device, const uint8_t *data, size_t n, void *d_rgb, size_t capacity, void *stream, rt_jpeg_stats *stats);
/* Test hooks.  rt_decode_jpeg_device on the null stream with subsequences of subsequence_bytes (at least 4: a symbol is at most 31 bits,
 * so every 32-bit run holds a symbol start; 0: the default); it synchronises and returns the status.  The plan of this thread's last
 * device decode: subsequence bytes, subsequences, rounds, subsequence decodes run, blocks, boundaries, 0, 0. */
int rt_dev_decode_jpeg(int32_t device, const uint8_t *data, size_t n, int32_t subsequence_bytes, void *d_rgb, size_t capacity);
int rt_dev_last_jpeg_plan(int64_t out[8]);

/* ---- Image textures from device memory (Texture.fs:34; csrc/rt_texture_plan.h, csrc/rt_texture_kernels.h; DESIGN.md "Textures from device
 * memory").  Added symbols and one added struct only -- no existing struct, field or symbol changed, so RT_ABI_VERSION stays 7.
 *
 * rt_texture.texels is a host pointer.  A bitmap that is already in device memory -- rt_decode_jpeg_device's output, a frame a torch program
 * made -- would have to come down, have its rows reversed (ParameterisedTexture.ofImage: img.[y] is the bitmap's row height - 1 - y) and go
 * up again inside scene creation.  These calls take, per texture record, where its texels come from; the reversal and the placement into
 * the scene's texel blob (images in record order, each zero-padded to 16 bytes) are one kernel launch for all device-sourced images of a
 * table, on the caller's stream.
 *
 * The create calls.  sources: n_textures entries, or NULL = every record RT_TEXELS_RECORD, which IS the existing call
 * (rt_scene_create_gpu_trees / rt_scene_create_device).  For a source that is not RT_TEXELS_RECORD the record's rt_texture.texels is
 * ignored and may be NULL.  RECORD images are uploaded into their ranges, DEVICE images are placed by the kernel, JPEG images are decoded
 * by rt_decode_jpeg_device's kernels on `stream` into stream-ordered scratch and placed by the same launch.  The device's copy of the scene
 * is installed directly, and the calls return after the stream has finished the build.  The scene is the scene the existing call returns
 * for the same records with the same texels on the host: every rt_scene_get_*, every render, rt_scene_tune* and rt_scene_destroy behave
 * identically; rt_scene_get_info().texel_bytes is right without any fetch.
 *
 * The host's copy of the texels is empty until something needs it -- the first use of the scene on ANOTHER device -- and is then fetched
 * once under the scene's lock, together with (and in the manner of) the lazy copy of a device-made scene's hittables: whatever fetches
 * that copy (rt_scene_get_tree, rt_scene_tune* where it rebuilds, ...) fetches the texels too.  rt_scene_create_textures has its host
 * arrays from the start; only its texels are lazy.  rt_dev_scene_has_host_mirror reports 0 while ANY part of the host's copy is still on
 * a device, so 0 for a scene of either call that has an image (and for any scene after rt_scene_set_texels_device), 1 once fetched; a
 * scene of these calls without an image reports what the existing call's scene reports.
 *
 * Refusals.  Before any device call, RT_ERR_INVALID_ARGUMENT: the existing call's own argument checks; a struct_size that is not
 * sizeof(rt_texels_source); an unknown kind or flag bit; a source that is not RECORD on a record that is not RT_TEXTURE_IMAGE; DEVICE or
 * JPEG with NULL data; DEVICE with bytes < width * height * 3.  RT_ERR_NO_DEVICE without a GPU.  Then the JPEG sources' headers, parsed on
 * the host: rt_decode_jpeg's status and text prefixed "texture i: ", and RT_ERR_INVALID_ARGUMENT for a file whose width or height is not
 * the record's.  Then the textures' own refusals and the hittables', unchanged in status and text; RT_ERR_UNSUPPORTED for a texel blob of
 * more than UINT32_MAX - 15 bytes (texel offsets are 32 bits wide).  A damaged entropy-coded stream is found by the decoder on the device:
 * the call waits for the stream, fails with rt_decode_jpeg's status and text, frees everything and leaves *out unwritten. */
enum rt_texels_kind { RT_TEXELS_RECORD = 0,  /* rt_texture.texels, a host pointer, as today */
                      RT_TEXELS_DEVICE = 1,  /* data: a bitmap in `device`'s memory, height*width*3 bytes, any alignment */
                      RT_TEXELS_JPEG   = 2 };/* data: a baseline JPEG in HOST memory, `bytes` long; decoded on `device` */
#define RT_TEXELS_TOP_FIRST 1u /* rows as a decoder leaves them: ofImage's reversal (Texture.fs:34) is applied on the device.
                                  Without it the rows are already img.[y], rt_texture.texels' layout.  JPEG: always top first. */
typedef struct rt_texels_source { uint32_t struct_size, kind, flags, reserved; const void *data; size_t bytes; } rt_texels_source;

/* Scene.make with host hittables (as rt_scene_create_gpu_trees) / device hittables (as rt_scene_create_device). */
int rt_scene_create_textures(const rt_hittable *hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                             const rt_texels_source *sources, const rt_scene_options *options, int32_t device, void *stream, rt_scene **out);
int rt_scene_create_device_textures(int32_t device, const void *d_hittables, size_t n_hittables, const rt_texture *textures, size_t n_textures,
                                    const rt_texels_source *sources, const rt_scene_options *options, void *stream, rt_scene **out);
/* ofImage alone: d_bitmap (top first) -> d_texels (rows reversed), capacity >= width*height*3, both of any alignment; exactly
 * width*height*3 bytes are written.  Enqueued on `stream`; the call does not wait.  Overlapping buffers (in place) are refused. */
int rt_of_image_device(int32_t device, const void *d_bitmap, int32_t width, int32_t height, void *d_texels, size_t capacity, void *stream);
/* Replace the texels of IMAGE record `texture` (same width and height) from a bitmap in device memory (bytes >= width*height*3; flags:
 * RT_TEXELS_TOP_FIRST or 0).  The copy is enqueued on `stream` into the scene's blob on `device` (that device's copy of the scene is made
 * first if there is none) and the call does not wait: launches enqueued on `stream` afterwards see the new texels, ordering against other
 * streams is the caller's, and a render in flight on another stream reads a mixture of old and new texels -- never a fault, the range is
 * fixed.  d_rgb must stay valid until the stream has passed the copy.  The host's copy of the texels is dropped and fetched again when
 * wanted.  RT_ERR_INVALID_ARGUMENT for a wrong index, a record that is not an image, short bytes, an unknown flag; RT_ERR_UNSUPPORTED for
 * a scene that has a copy on another device.  On any refusal the scene is unchanged. */
int rt_scene_set_texels_device(rt_scene *scene, int32_t texture, int32_t device, const void *d_rgb, size_t bytes, uint32_t flags, void *stream);
/* Test hooks.  The texel blob as `device` holds it (out may be NULL to ask for *bytes) and every record's texel_off (n_textures words,
 * UINT32_MAX: not an image; may be NULL).  The plan of this thread's last rt_scene_create_*textures call with sources: textures, images,
 * device-sourced, jpeg-sourced, blob bytes; then, counted on from that call through rt_scene_set_texels_device and the lazy fetch on
 * this thread: of_image_kernel launches, texel bytes copied host->device, texel bytes copied device->host. */
int rt_dev_scene_texels(const rt_scene *scene, int32_t device, void *out, size_t cap, size_t *bytes, uint32_t *texel_off);
int rt_dev_last_texture_plan(int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* RTFS_AMD_H */
