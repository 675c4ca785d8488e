// rt_texture_kernels.h -- ParameterisedTexture.ofImage (Texture.fs:34) on the device: bitmaps in device memory into a scene's texel blob.
// The rules (layout, which source byte lands where, which image a blob byte belongs to) are rt_texture_plan.h's; this is one kernel around
// rtt::place_unit.  One workgroup-independent pass: no workgroup waits for another, nothing is reduced.
#pragma once
#include "rt_texture_plan.h"

#include <hip/hip_runtime.h>

#define RTXK_BLOCK 256

namespace rtxk {

// One lane per 16-byte unit of the blob, units [unit0, unit0 + n_units).  The table: `table` (device memory, n entries, staged in LDS once
// per workgroup) or, when table is NULL, the single entry `one` passed by value (rt_scene_set_texels_device, rt_of_image_device: nothing to
// upload, so the launch needs no host memory to outlive it).
// ALIGNED: `blob` is 16-byte aligned and every image's padded range is the kernel's to write -- one 16-byte store per lane, padding as 0.
// Otherwise (rt_of_image_device: a caller's buffer of any alignment, width * height * 3 bytes of it) byte stores of the texels alone.
template <bool ALIGNED>
__global__ __launch_bounds__(RTXK_BLOCK) void of_image_kernel(const rtt::ImageEntry *table, uint32_t n, const rtt::ImageEntry one, uint8_t *blob, uint64_t unit0,
                                                               uint64_t n_units) {
    __shared__ rtt::ImageEntry entries[RTX_MAX_IMAGES];
    __shared__ uint64_t offsets[RTX_MAX_IMAGES];
    if (table) {
        for (uint32_t i = threadIdx.x; i < n; i += RTXK_BLOCK) { const rtt::ImageEntry e = table[i]; entries[i] = e; offsets[i] = e.off; }
    } else {
        n = 1u;
        if (threadIdx.x == 0) { entries[0] = one; offsets[0] = one.off; }
    }
    __syncthreads();
    const uint64_t id = (uint64_t) blockIdx.x * RTXK_BLOCK + threadIdx.x;
    if (id >= n_units) return;
    const uint64_t at = (unit0 + id) * RTX_UNIT;
    uint8_t out[RTX_UNIT];
    uint32_t valid = 0u;
    if (!rtt::place_unit(offsets, entries, n, at, out, &valid)) return;
    if (ALIGNED) {
        uint4 v;
        v.x = (uint32_t) out[0] | ((uint32_t) out[1] << 8) | ((uint32_t) out[2] << 16) | ((uint32_t) out[3] << 24);
        v.y = (uint32_t) out[4] | ((uint32_t) out[5] << 8) | ((uint32_t) out[6] << 16) | ((uint32_t) out[7] << 24);
        v.z = (uint32_t) out[8] | ((uint32_t) out[9] << 8) | ((uint32_t) out[10] << 16) | ((uint32_t) out[11] << 24);
        v.w = (uint32_t) out[12] | ((uint32_t) out[13] << 8) | ((uint32_t) out[14] << 16) | ((uint32_t) out[15] << 24);
        *(uint4 *) (blob + at) = v;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < RTX_UNIT; ++k) if (k < valid) blob[at + k] = out[k];
    }
}

} // namespace rtxk
