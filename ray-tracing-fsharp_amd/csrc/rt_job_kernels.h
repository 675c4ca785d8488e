// rt_job_kernels.h -- the partial spill of a render job on the device: ImageOutput.resume's records (ImageOutput.fs:131-161; the record
// at :145-155) for the PRESENT pixels only, in row-major order -- what an interrupted reference run leaves behind.  The host formatter
// rth::format_pixel_map_present (rt_scene.h) is what every byte is held to.  rt_output.h's three steps, with a pixel's length 0 where its
// presence byte is 0:
//   present_sums_kernel     one workgroup per tile of RTO_TILE_PIXELS pixels: the tile's byte count
//   rto::format_scan_kernel the output stage's own scan: tile offsets, the total, and "does the caller's buffer hold it" on the device
//   present_scatter_kernel  one workgroup per tile: the lengths again, a scan inside the tile, every thread stores its own records
// d_rgb, d_present and d_out may have any byte alignment: every access is a byte.
#pragma once

#include "rt_output.h"

namespace rtjob {

// This thread's RTO_THREAD_PIXELS consecutive pixels: len[k] (0 behind the image's end and for an absent pixel), (g, r, c) of the first
__device__ inline uint32_t present_lengths(const unsigned char *present, uint32_t npx, uint32_t cols, uint32_t len[RTO_THREAD_PIXELS], uint32_t &g0, uint32_t &r0,
                                           uint32_t &c0) {
    g0 = blockIdx.x * (uint32_t) RTO_TILE_PIXELS + threadIdx.x * (uint32_t) RTO_THREAD_PIXELS;
    r0 = g0 / cols; c0 = g0 - r0 * cols;
    uint32_t r = r0, c = c0, sum = 0;
    for (uint32_t k = 0; k < (uint32_t) RTO_THREAD_PIXELS; ++k) {
        const uint32_t g = g0 + k;
        len[k] = (g < npx && present[g] != 0u) ? rto::ascii_int_len(r) + rto::ascii_int_len(c) + 5u : 0u; // ',' '\n' R G B
        sum += len[k];
        if (++c == cols) { c = 0; ++r; }
    }
    return sum;
}

__global__ __launch_bounds__(RTO_BLOCK) void present_sums_kernel(const unsigned char *present, uint32_t npx, uint32_t cols, unsigned long long *tiles) {
    __shared__ uint32_t wave_tot[RTO_BLOCK / 64];
    uint32_t len[RTO_THREAD_PIXELS], g0, r0, c0, total;
    const uint32_t mine = present_lengths(present, npx, cols, len, g0, r0, c0);
    (void) rto::block_exclusive_scan<uint32_t, RTO_BLOCK>(mine, wave_tot, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(RTO_BLOCK) void present_scatter_kernel(const unsigned char *rgb, const unsigned char *present, uint32_t npx, uint32_t cols,
                                                                    const unsigned long long *tiles, const rto::FormatScratch *head, unsigned char *out) {
    __shared__ uint32_t wave_tot[RTO_BLOCK / 64];
    if (!head->go) return; // the same word for every thread of every workgroup
    uint32_t len[RTO_THREAD_PIXELS], g0, r0, c0, total;
    const uint32_t mine = present_lengths(present, npx, cols, len, g0, r0, c0);
    const uint32_t at0 = rto::block_exclusive_scan<uint32_t, RTO_BLOCK>(mine, wave_tot, total);
    unsigned char *dst = out + tiles[blockIdx.x] + at0; // (head->go: the whole output fits, so every byte below is inside the buffer)
    uint32_t r = r0, c = c0;
    for (uint32_t k = 0; k < (uint32_t) RTO_THREAD_PIXELS; ++k) {
        if (len[k] != 0u) {
            const unsigned char *p = rgb + (size_t) (g0 + k) * 3u;
            uint32_t n = rto::put_ascii_int(dst, r);
            dst[n++] = ',';
            n += rto::put_ascii_int(dst + n, c);
            dst[n++] = '\n';
            dst[n++] = p[0]; dst[n++] = p[1]; dst[n++] = p[2];
            dst += n;
        }
        if (++c == cols) { c = 0; ++r; }
    }
}

} // namespace rtjob
