// rt_jpeg_kernels.h -- the decode of rt_jpeg.h on the device.  The format, the subsequence step, the IDCT, the upsampling and the colour
// conversion are rt_jpeg.h's; the scan of words is rt_scene_kernels.h's.  DESIGN.md "JPEG on the device".
//
// Launches on the caller's stream, and NO workgroup ever waits for another:
//   clean_flags_kernel      per raw entropy-coded byte: is it kept, is it a restart marker's FF           (then two scans of words)
//   clean_scatter_kernel    kept bytes to their clean positions, the markers' clean bit positions to the sorted bounds
//   sync_kernel             one ROUND: one thread per subsequence runs rtj::sync_round; ran[round] counts the threads that decoded.
//                           The host launches rounds in small batches and reads the batch's counts; a round that decoded nothing
//                           ends the loop, and so does round number `subsequences`
//   place_kernel            (after the scan of the block counts) the step again from the now true start states: coefficients as
//                           int16 at block * 64 + k, every store behind a check of the block index, and the validity rule -- the
//                           blocks in front of every bound, the total -- into Head::flags
//   dc_gather_kernel        the DC differences by component                                              (then one inclusive scan)
//   idct_kernel             one lane per block: dequantise, jpeg_idct_islow, samples into the component's plane
//   colour_kernel           one thread per pixel: upsample, YCbCr -> RGB, store.  The ONLY kernel that writes d_rgb, and it writes
//                           nothing when Head::flags is set
// The coefficient and plane buffers are scratch, sized from the header; what a damaged stream makes of them is never shown.
#pragma once

#include "rt_jpeg.h"
#include "rt_scene_kernels.h"

#include <hip/hip_runtime.h>

#define RTJK_BLOCK 256
#define RTJK_SYNC_BLOCK 64  /* one wave: a subsequence decode is long and divergent, small groups spread over the CUs */
#define RTJK_ROUND_BATCH 4  /* rounds launched between two reads of their counts */

namespace rtjk {

struct Head {
    uint32_t flags; // rtj::BAD_*: nothing is written to d_rgb
    uint32_t pad[7];
};
static_assert(sizeof(Head) == 32, "the round counts follow the head");

__global__ __launch_bounds__(RTJK_BLOCK) void clean_flags_kernel(const uint8_t *raw, uint32_t n, uint32_t *keep, uint32_t *rst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keep[i] = rtj::is_kept(raw, n, i) ? 1u : 0u;
    rst[i] = rtj::is_bound(raw, n, i) ? 1u : 0u;
}
// keep_at / rst_at: the exclusive scans of the flags
__global__ __launch_bounds__(RTJK_BLOCK) void clean_scatter_kernel(const uint8_t *raw, uint32_t n, const uint32_t *keep_at, const uint32_t *rst_at, uint8_t *clean,
                                                                   uint32_t n_clean, uint32_t *bounds, uint32_t nb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (rtj::is_bound(raw, n, i)) {
        if (rst_at[i] < nb) bounds[rst_at[i]] = keep_at[i] * 8u;
    } else if (rtj::is_kept(raw, n, i) && keep_at[i] < n_clean) {
        clean[keep_at[i]] = raw[i];
    }
}

__device__ inline void stage_tables(rtj::Tables *lds, const rtj::Tables *t) {
    static_assert(sizeof(rtj::Tables) % 4u == 0u, "copied as words");
    for (uint32_t w = threadIdx.x; w < sizeof(rtj::Tables) / 4u; w += blockDim.x) ((uint32_t *) lds)[w] = ((const uint32_t *) t)[w];
    __syncthreads();
}

__global__ __launch_bounds__(RTJK_SYNC_BLOCK) void sync_kernel(const rtj::Frame f, const rtj::Tables *tables, const uint8_t *clean, uint32_t nbits, const uint32_t *bounds,
                                                                uint32_t nb, uint32_t S, uint32_t ns, uint32_t round, rtj::State *start, const rtj::State *end_prev,
                                                                rtj::State *end_cur, uint32_t *count, uint32_t *ran) {
    __shared__ rtj::Tables t;
    stage_tables(&t, tables);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool did = i < ns && rtj::sync_round(f, t, clean, nbits, bounds, nb, S, i, round, start, end_prev, end_cur, count);
    const unsigned long long all = __ballot(did);
    if ((threadIdx.x & 63u) == 0u && all) atomicAdd(&ran[round], (uint32_t) __popcll(all));
}

// first: the exclusive scan of count; first[ns] .. is not there: sums_total points at the scan's sum of all
__global__ __launch_bounds__(RTJK_SYNC_BLOCK) void place_kernel(const rtj::Frame f, const rtj::Tables *tables, const uint8_t *clean, uint32_t nbits, const uint32_t *bounds,
                                                                 uint32_t nb, uint32_t S, uint32_t ns, const rtj::State *start, const uint32_t *first,
                                                                 const uint32_t *sums_total, int16_t *coefs, Head *head) {
    __shared__ rtj::Tables t;
    stage_tables(&t, tables);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    rtj::PlaceSink sink{&f, coefs, first[i], 0u};
    rtj::State s = start[i];
    (void) rtj::step(f, t, clean, nbits, bounds, nb, s, rtj::sub_end(i, S, nbits), sink);
    if (i == 0u && *sums_total != f.total) sink.flags |= (uint32_t) rtj::BAD_COUNT;
    if (sink.flags) atomicOr(&head->flags, sink.flags);
}

__global__ __launch_bounds__(RTJK_BLOCK) void dc_gather_kernel(const rtj::Frame f, const int16_t *coefs, uint32_t *dcarr, const Head *head) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= f.total || head->flags) return;
    uint32_t c, gi, seg, brow, bcol;
    rtj::block_place(f, g, c, gi, seg, brow, bcol);
    dcarr[gi] = (uint32_t) (int32_t) coefs[(size_t) g * 64u]; // (gi < total: a permutation of the blocks)
}

__global__ __launch_bounds__(RTJK_BLOCK) void idct_kernel(const rtj::Frame f, const int16_t *coefs, const uint32_t *dcsum, uint8_t *planes, const Head *head) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= f.total || head->flags) return;
    rtj::block_samples(f, coefs, dcsum, g, planes);
}

__global__ __launch_bounds__(RTJK_BLOCK) void colour_kernel(const rtj::Frame f, const uint8_t *planes, uint8_t *rgb, const Head *head) {
    if (head->flags) return; // the same word for every thread of every workgroup
    const uint32_t px = blockIdx.x * blockDim.x + threadIdx.x;
    if (px >= f.W * f.H) return;
    const uint32_t y = px / f.W, x = px - y * f.W;
    uint8_t c[3];
    rtj::pixel_rgb(f, planes, x, y, c);
    rgb[(size_t) px * 3u] = c[0]; rgb[(size_t) px * 3u + 1u] = c[1]; rgb[(size_t) px * 3u + 2u] = c[2];
}

} // namespace rtjk
