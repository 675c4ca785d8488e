// rt_surface_kernels.h -- surface records at hits (DESIGN.md "Surface records"; rt_surfaces, rt_camera_surfaces): for a list of
// (hit_index, strike, incoming ray's origin) the normal, the inside flag, the surface colour, the colour a White ray leaves with and
// the texture coordinates -- the values Hittable.Reflection forms (reflection<LDS, TEX>, rt_device.h) and the render throws away.
//
// One kernel, separate from render_kernel, with its own parameter block.  It reads the scene through SceneView<false>'s global
// image: a slot reads ONE object record once, so staging the scene would cost more than it saves.
//
// Shape: a workgroup of RTSF_BLOCK threads takes tiles of RTSF_TILE slots, grid-striding over them.
//   phase 1  thread t handles slots base + t + 256 k: normal and inside for every slot, colour / tint / uv for the slots whose colour
//            is a plain Pixel; a slot whose colour is Texture.colourAt on a parameterised texture is appended to the tile's LDS list
//            (ballot + mbcnt rank, one LDS atomic per wave).
//   phase 2  after a barrier the list is consumed 256 entries at a time, i.e. by FULL waves whatever lanes the textured hits fell on:
//            strike and object are read again (L2-hot), texture_colour_at_inline<PROG> runs with nothing else live.
// The texture evaluation is hundreds of double-double instructions, everything else a few dozen FP64 operations: run at the lane
// occupancy the hits happen to have, a frame with a textured globe in one corner would pay the evaluation per WAVE that touches it.
#pragma once
#include "rt_device.h"
#include "rt_surface_plan.h"

namespace rtd {

struct SurfaceParams {
    const unsigned char *scene_image;
    SceneOffsets off;
    const TexRec *tex;
    const uint8_t *texels;
    const int32_t *orig_to_obj;  // index into rt_scene_create's array -> object-table index (the inverse of DeviceScene::obj_to_orig)
    int32_t n_hittables;
    uint32_t tex_phase;          // rtsf::SurfacePlan::tex_phase
    const int32_t *hit_index;    // [slots]
    const double *strike;        // [slots][3]
    const double *origin_base;   // the origin of slot i: origin_base + (i / slots_per_origin) * origin_stride doubles
    uint32_t slots_per_origin, origin_stride;
    uint64_t slots;
    double *normal;              // [slots][3] or null
    uint8_t *inside;             // [slots] or null
    uint8_t *colour;             // [slots][3] or null
    uint8_t *tint;               // [slots][3] or null
    double *uv;                  // [slots][2] or null
    const unsigned int *bad;     // nonzero: the list is malformed (surface_list_check_kernel, or the camera launch's seal): nothing is written
    unsigned long long *textured;// the slots phase 2 evaluated, summed over the tiles; or null
};

// orig_to_obj[obj_to_orig[j]] = j: obj_to_orig is a permutation of [0, n)
__global__ void __launch_bounds__(256) surface_inverse_map_kernel(const int32_t *obj_to_orig, int32_t n, int32_t *orig_to_obj) {
    const int j = (int) (blockIdx.x * 256u + threadIdx.x);
    if (j >= n) return;
    const int32_t o = obj_to_orig[j];
    if (o >= 0 && o < n) orig_to_obj[o] = j;
}

// Is every entry an index rt_scene_create's array has, or -1 / -2?  pixel_list_check_kernel's shape (rt_render_kernel.h): one 4-byte
// load per lane, a ballot, one atomicAdd per wave that saw a bad entry.  The check guards MEANING, not memory: the kernel below never
// indexes with an entry outside the array.
__global__ void __launch_bounds__(256) surface_list_check_kernel(const int32_t *list, unsigned long long n, int32_t n_hittables, unsigned int *bad) {
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long) gridDim.x * 256ull;
    const unsigned long long trips = (n + stride - 1ull) / stride; // uniform over the grid: every lane of a wave makes every ballot
    unsigned long long nBad = 0ull;
    for (unsigned long long t = 0; t < trips; ++t) {
        const unsigned long long i = t * stride + (unsigned long long) blockIdx.x * 256ull + threadIdx.x;
        int32_t g = 0;
        if (i < n) g = list[i];
        nBad += (unsigned long long) __popcll(__builtin_amdgcn_ballot_w64(i < n && !rtsf::list_entry_ok(g, n_hittables)));
    }
    if (lane == 0 && nBad != 0ull) atomicAdd(bad, (unsigned int) nBad); // (n < 2^31: the sum cannot wrap to 0)
}

RTD_INLINE uint32_t surface_lane_rank(unsigned long long mask) { // number of set bits of `mask` below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
}
RTD_INLINE void surface_store_rgb(uint8_t *out, uint64_t slot, uint32_t c) {
    if (!out) return;
    out[slot * 3 + 0] = (uint8_t) c;
    out[slot * 3 + 1] = (uint8_t) (c >> 8);
    out[slot * 3 + 2] = (uint8_t) (c >> 16);
}
// the colour Hittable.Reflection leaves a White LightRay with: Pixel.combine White c = c; every style that goes on darkens it
RTD_INLINE uint32_t surface_tint(const SceneView<false> &sc, int obj, i2 m, double sphereAlbedo, uint32_t colour) {
    if (rtsf::emitter(m.x)) return colour;
    const bool isPlane = (m.x & 3) == (int) RTD_KIND_PLANE;
    return pix_darken(isPlane ? sc.mat[obj * 4 + 0] : sphereAlbedo, colour);
}

template <bool PROG>
__global__ void __launch_bounds__(RTSF_BLOCK) surface_kernel(const SurfaceParams p) {
    __shared__ uint16_t list[RTSF_TILE]; // the tile's slots that want phase 2, as offsets from the tile's base
    __shared__ uint32_t listCount;
    if (p.bad && *p.bad != 0u) return; // (uniform over the grid)

    SceneView<false> sc;
    sc.node = p.scene_image + p.off.node;
    sc.geo = (const d2 *) (p.scene_image + p.off.geo);
    sc.meta = (const i2 *) (p.scene_image + p.off.meta);
    sc.mat = (const double *) (p.scene_image + p.off.mat);
    sc.n_nodes = p.off.n_nodes; sc.n_bounded = p.off.n_bounded; sc.n_unbounded = p.off.n_unbounded;
    sc.first = 0; sc.end = 0; sc.lds_lim = 0; sc.lds_thr = 65; sc.narrow = 0;
    sc.tex = p.tex; sc.texels = p.texels;

    const uint32_t t = threadIdx.x;
    const uint32_t lane = t & 63u;
    const double qnan = __builtin_nan("");
    const uint64_t tiles = (p.slots + (uint64_t) RTSF_TILE - 1u) / (uint64_t) RTSF_TILE;
    const bool wantTex = p.tex_phase != 0u;
    if (t == 0) listCount = 0u;
    __syncthreads();

    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (uniform over the block: every thread meets every barrier)
        const uint64_t base = tile * (uint64_t) RTSF_TILE;
        // ---- phase 1 ----
#pragma unroll 1
        for (uint32_t k = 0; k < (uint32_t) (RTSF_TILE / RTSF_BLOCK); ++k) {
            const uint32_t local = t + (uint32_t) RTSF_BLOCK * k;
            const uint64_t i = base + local;
            bool later = false;
            if (i < p.slots) {
                const int32_t hit = p.hit_index[i];
                const V3 strike = mk(p.strike[i * 3 + 0], p.strike[i * 3 + 1], p.strike[i * 3 + 2]);
                const double *op = p.origin_base + (uint64_t) (p.slots_per_origin == 1u ? (uint32_t) i : (uint32_t) i / p.slots_per_origin) * p.origin_stride;
                const V3 o = mk(op[0], op[1], op[2]);
                const bool finite = __builtin_isfinite(strike.x) && __builtin_isfinite(strike.y) && __builtin_isfinite(strike.z) &&
                                    __builtin_isfinite(o.x) && __builtin_isfinite(o.y) && __builtin_isfinite(o.z);
                V3 n = mk(qnan, qnan, qnan);
                bool inside = false;
                uint32_t colour = RTD_BLACK, tint = RTD_BLACK;
                if (!rtsf::no_surface(hit, p.n_hittables, finite)) {
                    const int obj = p.orig_to_obj[hit];
                    const i2 m = sc.meta[obj];
                    const d2 g0 = sc.geo[obj * 3 + 0], g1 = sc.geo[obj * 3 + 1], g2 = sc.geo[obj * 3 + 2];
                    const bool isPlane = (m.x & 3) == (int) RTD_KIND_PLANE;
                    const int style = (m.x >> 2) & 7;
                    colour = (uint32_t) m.y & 0x00FFFFFFu;
                    if (isPlane) n = mk(g1.y, g2.x, g2.y); // as given, never flipped (InfinitePlane.fs:43-99)
                    else {                                 // Sphere.fs:150-200, statement for statement reflection's
                        const V3 c = mk(g0.x, g0.y, g1.x);
                        const double r2 = g1.y, radius = g2.y;
                        const bool flipped = (m.x >> 5) & 1;
                        V3 n0;
                        const bool have = unitise(vsub(strike, c), n0); // Sphere.normal (Sphere.fs:65-66); ValueNone: the reference throws, NaN here
                        const V3 co = vsub(c, o);
                        const int cmp = fcmp(dot(co, co), r2);
                        inside = (cmp != CMP_GT) != flipped;
                        if (have) n = inside ? vscale(-1.0, n0) : n0;
                        if (style == 1) { // LightSourceCap (Sphere.fs:190-200)
                            const double lower = c.x + (radius - (radius / 4.0));
                            if (fcmp(strike.x, lower) != CMP_GT) colour = RTD_BLACK;
                        }
                    }
                    const int texId = wantTex ? rtsf::texture_of(m.x, m.y) : -1;
                    if (texId >= 0) {
                        const TexRec *root = sc.tex + texId;
                        if (root->kind == 0u) colour = root->rgb; // ParameterisedTexture.toTexture's Colour case (Texture.fs:71)
                        else later = true;
                    }
                    if (!later) tint = surface_tint(sc, obj, m, g2.x, colour);
                }
                if (p.normal) { p.normal[i * 3 + 0] = n.x; p.normal[i * 3 + 1] = n.y; p.normal[i * 3 + 2] = n.z; }
                if (p.inside) p.inside[i] = inside ? 1u : 0u;
                if (!later) {
                    surface_store_rgb(p.colour, i, colour);
                    surface_store_rgb(p.tint, i, tint);
                    if (p.uv) { p.uv[i * 2 + 0] = qnan; p.uv[i * 2 + 1] = qnan; }
                }
            }
            if (wantTex) { // (outside the bounds test: every lane of the wave makes the ballot)
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(later);
                if (mask != 0ull) {
                    uint32_t at = 0u;
                    if (lane == 0u) at = atomicAdd(&listCount, (uint32_t) __popcll(mask));
                    at = (uint32_t) __builtin_amdgcn_readfirstlane((int) at);
                    if (later) list[at + surface_lane_rank(mask)] = (uint16_t) local; // at + rank < RTSF_TILE: a tile appends each of its slots at most once
                }
            }
        }
        __syncthreads();
        // ---- phase 2 ----
        const uint32_t nList = wantTex ? listCount : 0u;
#pragma unroll 1
        for (uint32_t j = t; j < nList; j += (uint32_t) RTSF_BLOCK) {
            const uint64_t i = base + (uint64_t) list[j];
            const int obj = p.orig_to_obj[p.hit_index[i]];
            const i2 m = sc.meta[obj];
            const V3 strike = mk(p.strike[i * 3 + 0], p.strike[i * 3 + 1], p.strike[i * 3 + 2]);
            double uv[2] = {qnan, qnan};
            const uint32_t colour = texture_colour_at_inline<PROG>(sc.tex, sc.texels, rtsf::texture_of(m.x, m.y), strike, uv);
            surface_store_rgb(p.colour, i, colour);
            if (p.tint) surface_store_rgb(p.tint, i, surface_tint(sc, obj, m, sc.geo[obj * 3 + 2].x, colour));
            if (p.uv) { p.uv[i * 2 + 0] = uv[0]; p.uv[i * 2 + 1] = uv[1]; }
        }
        __syncthreads(); // the list is read; the next tile may fill it
        if (t == 0) {
            if (p.textured && nList != 0u) atomicAdd(p.textured, (unsigned long long) nList);
            listCount = 0u;
        }
        __syncthreads();
    }
}

} // namespace rtd
