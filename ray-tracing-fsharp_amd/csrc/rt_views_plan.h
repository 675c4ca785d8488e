// rt_views_plan.h -- the WORK UNITS of a batch of views (rt_render_views; DESIGN.md "Batches of views"), defined once.  A batch is
// n_views frames of pixels_per_view = rows * cols pixels each over one scene, rendered by one launch.  The camera and the seed key of a
// wave's current work stay wave-uniform (scalar pointers, as a frame's one camera is), so no piece of work spans two views:
//   the fused kernel / pass A   unit u is view u / units_per_view; its first local pixel is (u % units_per_view) * chunk and it has
//                               min(chunk, pixels_per_view - first) pixels -- the last unit of a view is short;
//   pass B                      the live list holds BATCH pixels, ordered by view (inside a view by decreasing cost); a reservation
//                               [first, first + n) of list entries is handed out as ranges clipped at the end of the view of its first entry.
// Batch pixel G = view * pixels_per_view + g owns accum[G] and rgb[G]; its stream is pixel_key(seed_key[view], g), the key a frame uses,
// so view v is the frame of camera v and seed v whatever the units are.
// Plain C++ over plain integers, so that tests/c/views_plan_table.cpp drives on a CPU the very functions the kernels inline (in the
// style of rt_extend_map.h and rt_job_plan.h).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTVIEWS_HD __host__ __device__ __forceinline__
#else
#define RTVIEWS_HD static inline
#endif

namespace rtviews {

// n_views * pixels_per_view <= INT32_MAX (the entry points refuse more), so every unit and every batch pixel fits 32 bits
struct Plan {
    uint32_t pixels_per_view; // rows * cols of one view
    uint32_t chunk;           // pixels per unit of the fused kernel / of pass A, >= 1
    uint32_t n_views;
};
struct Unit { uint32_t view, first, npx; }; // pixels [first, first + npx) of `view`, local to it

RTVIEWS_HD uint32_t units_per_view(const Plan &pl) { return (pl.pixels_per_view + pl.chunk - 1u) / pl.chunk; }
RTVIEWS_HD uint64_t units_of(const Plan &pl) { return (uint64_t) pl.n_views * (uint64_t) units_per_view(pl); }

// Unit u < units_of(pl).  upv: units_per_view(pl), which the kernel holds as a launch parameter
RTVIEWS_HD Unit unit_of(const Plan &pl, uint32_t upv, uint32_t u) {
    Unit r;
    r.view = u / upv;
    r.first = (u - r.view * upv) * pl.chunk;
    const uint32_t left = pl.pixels_per_view - r.first;
    r.npx = left < pl.chunk ? left : pl.chunk;
    return r;
}

RTVIEWS_HD uint64_t batch_pixel(const Plan &pl, uint32_t view, uint32_t g) { return (uint64_t) view * (uint64_t) pl.pixels_per_view + (uint64_t) g; }
RTVIEWS_HD uint32_t view_of(uint32_t pixels_per_view, uint32_t batch_px) { return batch_px / pixels_per_view; }

// Camera hits over a batch (rt_camera_hits_views): the entries of the ONE list stand where a view's pixels do (pixels_per_view = n), each
// with n_samples output slots; the slot of the first item of a unit that starts at entry `first` of `view`.
// n_views * n * n_samples <= INT32_MAX (the entry points refuse more), so every slot fits 32 bits
RTVIEWS_HD uint32_t first_slot(const Plan &pl, uint32_t view, uint32_t first, uint32_t n_samples) { return (view * pl.pixels_per_view + first) * n_samples; }

// Pass B: how many of the list entries [first, first + n) a range may take when the view of entry `first` ends at list index view_end
// (> first: the list is ordered by view and entry `first` is one of that view's)
RTVIEWS_HD uint32_t range_in_view(uint64_t first, uint32_t n, uint64_t view_end) {
    const uint64_t left = view_end - first;
    return left < (uint64_t) n ? (uint32_t) left : n;
}

// The ordering of pass B's list: key = view * buckets + (buckets - 1 - cost bucket), ascending -- by view, then by decreasing cost.
// `buckets` cost buckets per view: RTD_COST_BUCKETS, or 1 (by view alone) for a batch of so many views that the table of keys would
// outgrow the list it orders.  No result depends on the order inside a view: it decides which wave traces what when.
RTVIEWS_HD uint32_t sort_buckets(uint32_t n_views, uint32_t cost_buckets) { return n_views <= 4096u ? cost_buckets : 1u; }
RTVIEWS_HD uint32_t sort_key(uint32_t view, uint32_t buckets, uint32_t cost_bucket) {
    return view * buckets + (buckets == 1u ? 0u : buckets - 1u - cost_bucket);
}

} // namespace rtviews
