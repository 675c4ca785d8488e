// rt_surface_plan.h -- the plan of the surface-record kernel (rt_surface_kernels.h; rt_surfaces, rt_camera_surfaces): tile and grid
// arithmetic and the three predicates the kernel decides a slot by, in ONE place over plain integers.  Plain C++17 shared by host
// and device (no scene, no device state), so tests/test_surface_plan_cpp.py runs it on a CPU (tests/c/surface_plan_table.cpp);
// rtfs_amd.hip launches what it lists and rt_dev_last_surface_plan reports it.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RTSF_HD __host__ __device__ inline
#else
#define RTSF_HD inline
#endif

namespace rtsf {

#define RTSF_BLOCK 256          /* threads of a workgroup */
#define RTSF_TILE 1024          /* slots a workgroup takes at a time: the capacity of its LDS list of textured slots (uint16 entries) */
#define RTSF_BLOCKS_PER_CU 8    /* the grid's cap: as many blocks as keep every CU busy, the tiles beyond are grid-strided */
static_assert(RTSF_TILE % RTSF_BLOCK == 0 && RTSF_TILE <= 65536, "a tile is whole rounds of the block, and a list entry is 16 bits");

struct SurfacePlan {
    uint64_t slots = 0;
    uint32_t tile = RTSF_TILE;
    uint32_t block = RTSF_BLOCK;
    uint64_t tiles = 0;
    uint64_t grid = 0;      // 0: nothing to launch
    bool prog = false;      // surface_kernel<true>: the scene holds a texture program
    bool tex_phase = false; // the per-tile list is built and phase 2 runs: colour, tint or uv was asked for AND the scene has texture records
};

// want_tex_outputs: colour, tint or uv is asked for.  scene_tex / scene_prog: the scene has texture records / one of them is a program.
static inline SurfacePlan plan(uint64_t slots, int cu_count, bool scene_tex, bool scene_prog, bool want_tex_outputs) {
    SurfacePlan pl;
    pl.slots = slots;
    pl.tiles = (slots + (uint64_t) RTSF_TILE - 1u) / (uint64_t) RTSF_TILE;
    const uint64_t fit = (uint64_t) (cu_count > 0 ? cu_count : 1) * (uint64_t) RTSF_BLOCKS_PER_CU;
    pl.grid = pl.tiles < fit ? pl.tiles : fit;
    pl.prog = scene_tex && scene_prog;
    pl.tex_phase = scene_tex && want_tex_outputs;
    return pl;
}

// A slot without a surface: hitObject's -1 (ValueNone) and -2 (Ray.make' gave ValueNone), and a strike or an origin with a component
// that is not finite (the reference throws or converts out of range there).  `finite`: all six components are.
// An index outside [-2, n_hittables) makes the LIST malformed (list_entry_ok); the kernel still never indexes with one.
RTSF_HD bool list_entry_ok(int32_t hit_index, int32_t n_hittables) { return hit_index >= -2 && hit_index < n_hittables; }
RTSF_HD bool no_surface(int32_t hit_index, int32_t n_hittables, bool finite) {
    return hit_index < 0 || hit_index >= n_hittables || !finite;
}

// The texture a slot's colour comes from, as an index into the scene's records, or -1: rt_device.h's textured() over the meta words
// {kind | style << 2 | flipped << 5, rgb | (texture + 1) << 24}.  Styles that carry a Texture: every SphereStyle but LightSourceCap
// (Sphere.fs:10-37) and the plane LightSource (InfinitePlane.fs:5).
RTSF_HD int texture_of(int32_t meta_x, int32_t meta_y) {
    const int texId = (int) (((uint32_t) meta_y) >> 24) - 1;
    const bool isPlane = (meta_x & 3) == 2;
    const int style = (meta_x >> 2) & 7;
    return (texId >= 0 && (isPlane ? style == 0 : style != 1)) ? texId : -1;
}
// Does the slot go through phase 2 (Texture.colourAt on a parameterised texture)?  root_kind: the kind of record texture_of() names
// (0 COLOUR: ParameterisedTexture.toTexture's Colour case is the record's own Pixel, no map is evaluated and uv stays NaN).
RTSF_HD bool needs_texture_phase(int32_t meta_x, int32_t meta_y, uint32_t root_kind) { return texture_of(meta_x, meta_y) >= 0 && root_kind != 0u; }
// uv is filled exactly for those slots
RTSF_HD bool uv_filled(int32_t meta_x, int32_t meta_y, uint32_t root_kind) { return needs_texture_phase(meta_x, meta_y, root_kind); }
// Hittable.Reflection returns the incoming colour combined with the surface's, NOT darkened: sphere LightSource and LightSourceCap,
// plane LightSource (Sphere.fs:185-200, InfinitePlane.fs:52-56)
RTSF_HD bool emitter(int32_t meta_x) {
    const bool isPlane = (meta_x & 3) == 2;
    const int style = (meta_x >> 2) & 7;
    return isPlane ? style == 0 : style <= 1;
}

} // namespace rtsf
