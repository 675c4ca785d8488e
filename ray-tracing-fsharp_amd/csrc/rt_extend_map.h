// rt_extend_map.h -- the item -> (pixel, offset) lookup of pass B's per-pixel ranges (rt_render_extend_map; DESIGN.md "Extending by
// map").  A wave's range holds npx <= 64 pixels; pixel j adds n2[j] samples, so the range's items are numbered
//   start[j] = n2[0] + ... + n2[j-1]   (exclusive prefix sums, start[0] = 0),   total = start[npx-1] + n2[npx-1]
// and item i belongs to the LAST pixel j with start[j] <= i, as that pixel's offset i - start[j].  "Last" makes a pixel with
// nothing to add (n2[j] = 0: start[j] == start[j+1]) own no item.  Plain C++ over plain integers, so that tests/c/extend_map_lookup_table.cpp
// drives on a CPU, exhaustively, the very function the kernel inlines (in the style of rt_launch_plan.h).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTM_HD __host__ __device__ __forceinline__
#else
#define RTM_HD static inline
#endif

namespace rtm {

#define RTM_MAX_PIXELS 64u /* pixels of a range: the lanes of a wave */

// Exclusive prefix sums of n2[0 .. npx) into start[0 .. npx); returns the total (64 pixels x 8e6 samples is below 2^32).
template <class In, class Out> RTM_HD uint32_t map_starts(In n2, uint32_t npx, Out start) {
    uint32_t run = 0u;
    for (uint32_t j = 0u; j < npx; ++j) { start[j] = run; run += (uint32_t) n2[j]; }
    return run;
}

// The pixel of item `item` < total: the last j < npx with start[j] <= item.  A search by halving steps over the 64 possible
// positions: six steps, each at most one read of `start` (none past npx), no division.  `Starts` is anything indexable -- on the
// device a pointer into the wave's LDS scratch.
template <class Starts> RTM_HD uint32_t map_find_pixel(Starts start, uint32_t npx, uint32_t item) {
    uint32_t j = 0u; // start[0] = 0 <= item
    for (uint32_t step = RTM_MAX_PIXELS / 2u; step != 0u; step >>= 1) {
        const uint32_t c = j + step;
        if (c < npx && (uint32_t) start[c] <= item) j = c;
    }
    return j;
}

} // namespace rtm
