// rt_job_plan.h -- the PRESENT SET of a render job (rt_render_job_*; DESIGN.md "Render jobs"), defined once.  A job is the whole-frame
// render of a shard whose waves may stop RESERVING work (a stop request, or the test hook's budget): every pass hands out its work
// from one atomic counter and a wave finishes what it reserved, so what has been rendered is a prefix of the unit order --
//   the fused kernel / pass A   units [0, done_a) of `chunk` consecutive local pixels each (the last one ragged);
//   pass B                      entries [0, done_b) of the cost-ordered live list, whose entries are local pixel indices.
// A pixel is PRESENT iff every sample the whole-frame render gives it has been added:
//   fused       its unit is below done_a;
//   two passes  its unit is below done_a AND it is not a live-list entry at an index >= done_b
//               (a pixel that pass A stopped early is on no list and is final; one that continues is final once pass B flushed it).
// done_a / done_b are the final values of the counters, clamped to their totals (an exhausted queue is overshot by one reservation per
// wave) and to the budget (a reservation at or beyond the limit gets nothing but still moves the counter).
// Plain C++ over plain integers, so that tests/c/job_plan_table.cpp drives on a CPU the very functions the finishing kernels inline
// (in the style of rt_extend_map.h and rt_png.h).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTJOB_HD __host__ __device__ __forceinline__
#else
#define RTJOB_HD static inline
#endif

namespace rtjob {

// The job's plan as the present set needs it (rt_dev_last_job_plan reports the same words)
struct Plan {
    int32_t passes;    // 1: the fused kernel; 2: pass A, the ordering, pass B
    uint32_t chunk;    // local pixels per unit of the fused kernel / of pass A
    uint64_t n_local;  // the shard's pixels: n_rows * cols
};
// The shard: local pixel lp is column lp % cols of image row row_first + (lp / cols) * row_stride
struct Shard { int32_t cols, row_first, row_stride, n_rows; };

RTJOB_HD uint64_t units_of(const Plan &pl) { return pl.chunk ? (pl.n_local + (uint64_t) pl.chunk - 1u) / (uint64_t) pl.chunk : 0u; }

// A counter's final value as a count of finished work: clamped to the total, and to the budget (limit < 0: none)
RTJOB_HD uint64_t clamp_done(uint64_t counter, uint64_t total, int64_t limit) {
    uint64_t d = counter < total ? counter : total;
    if (limit >= 0 && (uint64_t) limit < d) d = (uint64_t) limit;
    return d;
}

// What a reservation [first, first + want) of a queue of `total` items gets under a budget: nothing at or beyond the limit (or the
// total), clipped to it when it straddles.  limit < 0: no budget.
RTJOB_HD uint64_t clip_reservation(uint64_t first, uint64_t want, uint64_t total, int64_t limit) {
    uint64_t end = total;
    if (limit >= 0 && (uint64_t) limit < end) end = (uint64_t) limit;
    if (first >= end) return 0u;
    return end - first < want ? end - first : want;
}

// The prefix of the fused kernel / pass A: is local pixel lp in a unit below done_a?
RTJOB_HD bool unit_done(const Plan &pl, uint64_t lp, uint64_t done_a) { return lp / (uint64_t) pl.chunk < done_a; }
// The live list's suffix: is the entry at `index` one that pass B has NOT rendered?
RTJOB_HD bool entry_pending(uint64_t index, uint64_t done_b) { return index >= done_b; }

// The image's pixel index (row-major over the whole frame) of the shard's local pixel lp
RTJOB_HD uint64_t global_pixel(const Shard &s, uint64_t lp) {
    const uint64_t lr = lp / (uint64_t) s.cols, c = lp - lr * (uint64_t) s.cols;
    return ((uint64_t) s.row_first + lr * (uint64_t) s.row_stride) * (uint64_t) s.cols + c;
}

// The whole set, as the finishing kernels write it: present[lp] = 0 or 1 for every local pixel; returns the number present.
// queue_a / queue_b: the counters' final values as read; limit_a / limit_b: the budget (-1: none); list: the live list, n_list entries.
template <class List> static inline uint64_t present_set(const Plan &pl, uint64_t queue_a, uint64_t queue_b, int64_t limit_a, int64_t limit_b, List list,
                                                         uint64_t n_list, uint8_t *present) {
    const uint64_t done_a = clamp_done(queue_a, units_of(pl), limit_a);
    for (uint64_t lp = 0; lp < pl.n_local; ++lp) present[lp] = unit_done(pl, lp, done_a) ? 1u : 0u;
    if (pl.passes == 2) {
        const uint64_t done_b = clamp_done(queue_b, n_list, limit_b);
        for (uint64_t i = 0; i < n_list; ++i)
            if (entry_pending(i, done_b)) present[(uint64_t) list[i]] = 0u;
    }
    uint64_t n = 0;
    for (uint64_t lp = 0; lp < pl.n_local; ++lp) n += present[lp];
    return n;
}

} // namespace rtjob
