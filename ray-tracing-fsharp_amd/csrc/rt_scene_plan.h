// rt_scene_plan.h -- what Scene.make (Scene.fs:15-28) computes PER ITEM, in one place: the check of a hittable, Sphere.make's box, the
// outward rounding of a box coordinate, the node / node32 / geo / meta / mat records of the device image (layout: rt_device.h), the section
// offsets and the box_implied predicate.  Plain C++ for host and device (no HIP calls), in the manner of rt_tree_plan.h and rt_walk_plan.h:
// build_scene and encode_image (rt_scene.h), the kernels of rt_scene_kernels.h and tests/c/scene_plan_table.cpp all include this one
// definition.  Nothing here may be contracted (-ffp-contract=off holds for host and device).
#pragma once
#include "../../include/rtfs_amd.h"
#include "rt_launch_consts.h"
#include "rt_tree_plan.h"

#ifndef RTD_NODE_BYTES
#define RTD_NODE_BYTES 112
#endif
// (the same values as rt_device.h, which needs the HIP headers; rtfs_amd.hip holds the two sets to each other)
#define RTS_LEAF 0x40000000
#define RTS_PEND_MARK 0x4000u
#define RTS_PEND_WIDE 0x80000000u
#define RTS_KIND_SPHERE 0u
#define RTS_KIND_PLANE 2u
#define RTS_MAX_BOUNDED 4500000u  /* (2n-1) * 112 B < 2^30: walk offsets are int32 byte offsets with bit 30 reserved (RTS_LEAF) */
#define RTS_MAX_OBJECTS 16000000u

namespace rts {

// ---- the check of one hittable: 0, or the first failing check in build_scene's order.  index * 8 + reason is the error word of the
// device route: its minimum over all hittables names the smallest bad index with that hittable's first failing check. ----
enum Reason { OK = 0, BAD_KIND = 1, BAD_STYLE = 2, TEXTURE_RANGE = 3, CARRIES_PIXEL = 4 };
RTT_HD static inline int check_hittable(const rt_hittable &o, int64_t n_textures) {
    if (o.kind > RT_HITTABLE_INFINITE_PLANE) return BAD_KIND;
    const bool plane = o.kind == RT_HITTABLE_INFINITE_PLANE;
    if (plane ? o.style > RT_PLANE_FUZZED_REFLECTION : o.style > RT_SPHERE_GLASS) return BAD_STYLE;
    if ((int64_t) o.texture >= n_textures) return TEXTURE_RANGE;
    if (o.texture >= 0) {
        const bool carries = plane ? o.style == RT_PLANE_LIGHT_SOURCE : o.style != RT_SPHERE_LIGHT_SOURCE_CAP;
        if (!carries) return CARRIES_PIXEL;
    }
    return OK;
}
static inline const char *reason_text(int reason) { // after "hittable <index>: "
    switch (reason) {
    case BAD_KIND: return "bad kind";
    case BAD_STYLE: return "bad style";
    case TEXTURE_RANGE: return "texture index out of range";
    case CARRIES_PIXEL: return "this style carries a Pixel, not a Texture";
    default: return "";
    }
}
// Array.partition (snd >> ValueOption.isSome): only Hittable.Sphere has a box
RTT_HD static inline bool is_bounded(const rt_hittable &o) { return o.kind == RT_HITTABLE_SPHERE; }
static inline const char *too_large_text() { return "scene too large for 32-bit walk offsets (4,500,000 bounded spheres)"; }
RTT_HD static inline bool too_large(uint64_t n_bounded, uint64_t n_objects) { return n_bounded > RTS_MAX_BOUNDED || n_objects > RTS_MAX_OBJECTS; }

// ---- Sphere.make's box (Sphere.fs:333-336): centre + (-r,-r,-r) .. centre + (r,r,r); inverted when r < 0 ----
RTT_HD static inline rtt::Box sphere_box(const rt_hittable &o) {
    rtt::Box b;
    for (int a = 0; a < 3; ++a) { b.mn[a] = o.point[a] + (-o.radius); b.mx[a] = o.point[a] + o.radius; }
    return b;
}
RTT_HD static inline bool is_nan(double v) { return v != v; }
RTT_HD static inline bool is_finite(double v) { return v - v == 0.0; }

// ---- outward rounding of a box coordinate to single precision (the node32 records): the largest float <= v / the smallest float >= v.
// +-inf and NaN pass through.  The neighbour is taken on the bits (what nextafterf gives for these operands). ----
RTT_HD static inline float f32_next(float f, bool up) { // f is not NaN, and not the infinity in the direction asked for
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof(u));
    if ((u << 1) == 0u) u = up ? 0x00000001u : 0x80000001u;   // either zero: the smallest subnormal on that side
    else if (((u >> 31) != 0u) == up) u -= 1u;                // towards zero
    else u += 1u;                                             // away from zero
    __builtin_memcpy(&f, &u, sizeof(u));
    return f;
}
RTT_HD static inline float f32_down(double v) {
    float f = (float) v; // round to nearest
    if ((double) f > v) f = f32_next(f, false);
    return f;
}
RTT_HD static inline float f32_up(double v) {
    float f = (float) v;
    if ((double) f < v) f = f32_next(f, true);
    return f;
}
RTT_HD static inline float abs32(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof(u));
    u &= 0x7FFFFFFFu;
    __builtin_memcpy(&f, &u, sizeof(u));
    return f;
}

// ---- section offsets of the image node | geo | meta | node32 | mat from (nn, nobj).  The same words as rtd::SceneOffsets' first
// eleven; bmax and box_implied are known only after the records. ----
struct Offsets {
    uint32_t node, geo, meta, node32, mat, total, lds_total, lds32_total;
    int32_t n_nodes, n_bounded, n_unbounded;
    uint64_t image_bytes; // what is allocated: `total`, 16 for an empty scene
};
RTT_HD static inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t) 15u; }
RTT_HD static inline Offsets offsets(uint64_t nn, uint64_t nb, uint64_t nu) {
    const uint64_t nobj = nb + nu;
    Offsets off;
    uint64_t cur = 0;
    off.node = (uint32_t) cur; cur = align16(cur + nn * RTD_NODE_BYTES);
    off.geo = (uint32_t) cur;  cur = align16(cur + nobj * 48u);
    off.meta = (uint32_t) cur; cur = align16(cur + nobj * 8u);
    off.lds_total = (uint32_t) cur; // [0, lds_total): what the counting variant stages
    off.node32 = (uint32_t) cur; cur = align16(cur + nn * RTD_NODE32_BYTES);
    off.lds32_total = (uint32_t) cur - off.geo; // [geo, node32 end): what the timed variant stages
    off.mat = (uint32_t) cur;  cur = align16(cur + nobj * 32u);
    off.total = (uint32_t) cur;
    off.n_nodes = (int32_t) nn; off.n_bounded = (int32_t) nb; off.n_unbounded = (int32_t) nu;
    off.image_bytes = cur == 0 ? 16 : cur;
    if (cur == 0) off.total = 16;
    if (off.lds_total == 0) off.lds_total = 16;
    if (off.lds32_total == 0) off.lds32_total = 16;
    return off;
}

// ---- the 112-byte node record and the 64-byte node32 record of pre-order node i from (box, skip, prim, place, nobj).
// place_i / place_next / place_skip: the node32 positions of i, i + 1 and skip (breadth first, pre-order within a level; place[nn] = nn).
// node: twelve doubles {mn, mx, mx, mn} per axis, then on_hit, on_miss, prim, 0.  node32: twelve floats the same way, rounded outward, then
// the links in the queue form of the timed node loop: a Leaf's on_hit is its on_miss, the third word its queue entry (16 bits wide for
// scenes below 16384 objects), the fourth the shift that pushes it. ----
struct NodeRec { double box[12]; int32_t link[4]; };
struct Node32Rec { float box[12]; int32_t link[4]; };
RTT_HD static inline NodeRec node_record(const rtt::Box &b, uint32_t i, int32_t skip, int32_t prim) {
    NodeRec r;
    for (int a = 0; a < 3; ++a) { r.box[a * 4] = b.mn[a]; r.box[a * 4 + 1] = b.mx[a]; r.box[a * 4 + 2] = b.mx[a]; r.box[a * 4 + 3] = b.mn[a]; }
    r.link[0] = prim >= 0 ? (int32_t) (RTS_LEAF | (i * RTD_NODE_BYTES)) : (int32_t) ((i + 1u) * RTD_NODE_BYTES); // on_hit
    r.link[1] = skip * RTD_NODE_BYTES; // byte offset of the record to visit on a miss
    r.link[2] = prim;                  // object index of a Leaf, -1 for a Branch
    r.link[3] = 0;
    return r;
}
RTT_HD static inline Node32Rec node32_record(const rtt::Box &b, int32_t prim, uint32_t place_next, uint32_t place_skip, uint64_t nobj) {
    Node32Rec r;
    for (int a = 0; a < 3; ++a) {
        const float lo = f32_down(b.mn[a]), hi = f32_up(b.mx[a]);
        r.box[a * 4] = lo; r.box[a * 4 + 1] = hi; r.box[a * 4 + 2] = hi; r.box[a * 4 + 3] = lo;
    }
    const bool leaf = prim >= 0;
    const int32_t onMiss32 = (int32_t) (place_skip * RTD_NODE32_BYTES);
    r.link[0] = leaf ? onMiss32 : (int32_t) (place_next * RTD_NODE32_BYTES);
    r.link[1] = onMiss32;
    r.link[2] = !leaf ? 0 : (nobj < 16384u ? (int32_t) (RTS_PEND_MARK | (uint32_t) prim) : (int32_t) (RTS_PEND_WIDE | (uint32_t) prim));
    r.link[3] = leaf ? 16 : 0;
    return r;
}
// what a node32 record adds to bmax: the largest |coordinate| above `bmax` (a NaN compares false and leaves it alone)
RTT_HD static inline float bmax_with(float bmax, const Node32Rec &r) {
    for (int a = 0; a < 3; ++a) {
        const float lo = abs32(r.box[a * 4]), hi = abs32(r.box[a * 4 + 1]);
        if (lo > bmax) bmax = lo;
        if (hi > bmax) bmax = hi;
    }
    return bmax;
}

// ---- geo (six doubles), meta (two words) and mat (four doubles) of one object ----
struct ObjectRec { double geo[6]; int32_t meta[2]; double mat[4]; };
RTT_HD static inline uint32_t pack_rgb(const uint8_t rgb[3]) { return (uint32_t) rgb[0] | ((uint32_t) rgb[1] << 8) | ((uint32_t) rgb[2] << 16); }
// flipped = Float.compare this.Radius 0.0 = Less (Sphere.fs:321), Float.compare's tolerance being 1e-8
RTT_HD static inline bool flipped(double radius) {
    const double d = radius - 0.0;
    return !((d < 0.0 ? -d : d) < 0.00000001) && (radius < 0.0);
}
RTT_HD static inline ObjectRec object_record(const rt_hittable &o) {
    ObjectRec r;
    uint32_t m0;
    double *g = r.geo, *m = r.mat;
    if (o.kind == RT_HITTABLE_INFINITE_PLANE) {
        g[0] = o.point[0]; g[1] = o.point[1]; g[2] = o.point[2];
        g[3] = o.normal[0]; g[4] = o.normal[1]; g[5] = o.normal[2];
        m0 = RTS_KIND_PLANE | (o.style << 2);
        m[0] = o.albedo; m[1] = o.fuzz; m[2] = 0.0; m[3] = 0.0;
    } else {
        g[0] = o.point[0]; g[1] = o.point[1]; g[2] = o.point[2];
        g[3] = o.radius * o.radius; // RadiusSquared (Sphere.fs:326)
        g[4] = o.albedo; g[5] = o.radius; // the radius itself: LightSourceCap (Sphere.fs:191) and the leaf pass' exact box (leaf_test_object_exact)
        m0 = RTS_KIND_SPHERE | (o.style << 2) | (flipped(o.radius) ? 32u : 0u);
        const bool usesIor = o.style == RT_SPHERE_DIELECTRIC || o.style == RT_SPHERE_GLASS;
        m[0] = 0.0; m[1] = usesIor ? o.ior : o.fuzz; m[2] = o.prob; m[3] = 0.0;
        if (usesIor) {
            // Per-material values the reference recomputes at every hit from the same inputs with the same IEEE operations: `1.0 / ior`
            // (Sphere.fs:117, 283-284) and Schlick's `param * param`, param = (1.0 - sr) / (1.0 + sr), for sr = ior (outside) and
            // sr = 1.0 / ior (inside) (Sphere.fs:288-289).
            const double ior = o.ior;
            const double inv = 1.0 / ior;
            if (o.style == RT_SPHERE_DIELECTRIC) m[3] = inv;
            else {
                const double po = (1.0 - ior) / (1.0 + ior), pi = (1.0 - inv) / (1.0 + inv);
                m[0] = pi * pi;  // Schlick's term inside the glass
                m[2] = inv;      // Glass carries no refraction probability
                m[3] = po * po;
            }
        }
    }
    r.meta[0] = (int32_t) m0;
    r.meta[1] = (int32_t) (pack_rgb(o.rgb) | ((uint32_t) (o.texture + 1) << 24));
    return r;
}

// ---- the hypotheses of leaf_test_object_exact's claim (rt_device.h): the exact leaf-box test is then implied by a sphere hit.
// radii_ok: every bounded radius r has r > 0 && r <= 100; rmax: the largest radius above 0 (0 when there is none). ----
RTT_HD static inline bool radius_ok(double r) { return r > 0.0 && r <= 100.0; }
RTT_HD static inline int32_t box_implied(float bmax, bool radii_ok, double rmax) {
    const bool ok = (bmax - bmax == 0.0f) && bmax <= 1000.0f && radii_ok;
    return (ok && rmax * (double) bmax <= 500.0) ? 1 : 0;
}

} // namespace rts
