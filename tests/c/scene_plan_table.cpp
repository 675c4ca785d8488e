// csrc/rt_scene_plan.h alone, as a host program: the per-item rules of Scene.make against hand-checked values.
//   g++ -std=c++17 -ffp-contract=off -o scene_plan_table tests/c/scene_plan_table.cpp && ./scene_plan_table
#include "../../ray-tracing-fsharp_amd/csrc/rt_scene_plan.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

static int failures = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; }            \
    } while (0)

static rt_hittable sphere(uint32_t style, double x, double y, double z, double r) {
    rt_hittable o{};
    o.kind = RT_HITTABLE_SPHERE; o.style = style;
    o.point[0] = x; o.point[1] = y; o.point[2] = z;
    o.radius = r; o.albedo = 0.75; o.fuzz = 0.25; o.ior = 1.5; o.prob = 0.5;
    o.rgb[0] = 1; o.rgb[1] = 2; o.rgb[2] = 3;
    o.texture = -1;
    return o;
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static void checks() {
    rt_hittable o = sphere(RT_SPHERE_GLASS, 0, 0, 0, 1);
    CHECK(rts::check_hittable(o, 0) == rts::OK);
    o.kind = 3;                                 CHECK(rts::check_hittable(o, 0) == rts::BAD_KIND);
    o.style = 99; o.texture = 7;                CHECK(rts::check_hittable(o, 0) == rts::BAD_KIND); // the first failing check
    o.kind = RT_HITTABLE_SPHERE;                CHECK(rts::check_hittable(o, 0) == rts::BAD_STYLE);
    o.style = RT_SPHERE_GLASS;                  CHECK(rts::check_hittable(o, 7) == rts::TEXTURE_RANGE);
    CHECK(rts::check_hittable(o, 8) == rts::OK);
    o.style = RT_SPHERE_LIGHT_SOURCE_CAP;       CHECK(rts::check_hittable(o, 8) == rts::CARRIES_PIXEL);
    o.kind = RT_HITTABLE_INFINITE_PLANE; o.style = RT_PLANE_FUZZED_REFLECTION + 1; CHECK(rts::check_hittable(o, 8) == rts::BAD_STYLE);
    o.style = RT_PLANE_LIGHT_SOURCE;            CHECK(rts::check_hittable(o, 8) == rts::OK);
    o.style = RT_PLANE_PURE_REFLECTION;         CHECK(rts::check_hittable(o, 8) == rts::CARRIES_PIXEL);
    o.texture = -1;                             CHECK(rts::check_hittable(o, 0) == rts::OK);
    o.kind = RT_HITTABLE_UNBOUNDED_SPHERE; o.style = RT_SPHERE_GLASS; CHECK(rts::check_hittable(o, 0) == rts::OK && !rts::is_bounded(o));
    CHECK(std::strcmp(rts::reason_text(rts::TEXTURE_RANGE), "texture index out of range") == 0);
    CHECK(!rts::too_large(4500000, 16000000) && rts::too_large(4500001, 4500001) && rts::too_large(0, 16000001));
    std::printf("checks ok\n");
}

static void boxes() {
    const rtt::Box b = rts::sphere_box(sphere(0, 1.0, -2.0, 0.5, 0.25));
    CHECK(b.mn[0] == 0.75 && b.mx[0] == 1.25 && b.mn[1] == -2.25 && b.mx[1] == -1.75 && b.mn[2] == 0.25 && b.mx[2] == 0.75);
    const rtt::Box inv = rts::sphere_box(sphere(0, 0.0, 0.0, 0.0, -1.0)); // inverted
    CHECK(inv.mn[0] == 1.0 && inv.mx[0] == -1.0);
    const rtt::Box z = rts::sphere_box(sphere(0, 0.0, 0.0, 0.0, 0.0)); // 0.0 + (-0.0) = +0.0
    CHECK(z.mn[0] == 0.0 && !std::signbit(z.mn[0]));
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(rts::is_nan(rts::sphere_box(sphere(0, inf, 0, 0, inf)).mn[0]) && !rts::is_finite(inf) && rts::is_finite(1e308) && !rts::is_finite(std::nan("")));
    std::printf("boxes ok\n");
}

static void rounding() {
    CHECK(rts::f32_down(0.5) == 0.5f && rts::f32_up(0.5) == 0.5f);
    CHECK(rts::f32_down(0.1) == std::nextafterf(0.1f, -1.0f) && rts::f32_up(0.1) == 0.1f);   // (float) 0.1 > 0.1
    CHECK(rts::f32_down(-0.1) == -0.1f && rts::f32_up(-0.1) == std::nextafterf(-0.1f, 1.0f));
    CHECK(bits(rts::f32_down(-1e-60)) == 0x80000001u && bits(rts::f32_up(1e-60)) == 0x00000001u); // past either zero: the smallest subnormal
    CHECK(bits(rts::f32_up(-1e-60)) == 0x80000000u && bits(rts::f32_down(1e-60)) == 0u);
    CHECK(rts::f32_down(1e300) == std::numeric_limits<float>::max() && std::isinf(rts::f32_up(1e300)));
    CHECK(std::isinf(rts::f32_down(-1e300)) && rts::f32_up(-1e300) == -std::numeric_limits<float>::max());
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(rts::f32_down(inf) == (float) inf && rts::f32_up(-inf) == (float) -inf && std::isnan(rts::f32_down(std::nan(""))));
    for (double v : {1.0 + 1e-12, -3.75 - 1e-9, 123456.789, 1e-40, -1e-40, 16777217.0}) { // against nextafterf, which the host code used
        float d = (float) v, u = (float) v;
        if ((double) d > v) d = std::nextafterf(d, -HUGE_VALF);
        if ((double) u < v) u = std::nextafterf(u, HUGE_VALF);
        CHECK(bits(rts::f32_down(v)) == bits(d) && bits(rts::f32_up(v)) == bits(u) && (double) d <= v && v <= (double) u);
    }
    std::printf("rounding ok\n");
}

static void offsets() {
    const rts::Offsets e = rts::offsets(0, 0, 0);
    CHECK(e.total == 16 && e.image_bytes == 16 && e.lds_total == 16 && e.lds32_total == 16 && e.node == 0 && e.mat == 0);
    const rts::Offsets o = rts::offsets(5, 3, 2); // 5 nodes, 5 objects
    CHECK(o.node == 0 && o.geo == 560 && o.meta == 800 && o.lds_total == 848 && o.node32 == 848 && o.mat == 1168 && o.total == 1328);
    CHECK(o.lds32_total == 1168 - 560 && o.n_nodes == 5 && o.n_bounded == 3 && o.n_unbounded == 2 && o.image_bytes == 1328);
    const rts::Offsets p = rts::offsets(0, 0, 3); // planes only: 144 | 24 -> 32 | 96
    CHECK(p.geo == 0 && p.meta == 144 && p.node32 == 176 && p.mat == 176 && p.total == 272);
    std::printf("offsets ok\n");
}

static void records() {
    const rtt::Box b{{-1.0, 0.1, 2.0}, {1.0, 0.3, 4.0}};
    const rts::NodeRec leaf = rts::node_record(b, 3, 4, 7), branch = rts::node_record(b, 0, 9, -1);
    CHECK(sizeof(leaf) == 112 && leaf.box[0] == -1.0 && leaf.box[1] == 1.0 && leaf.box[2] == 1.0 && leaf.box[3] == -1.0 && leaf.box[4] == 0.1 && leaf.box[9] == 4.0);
    CHECK(leaf.link[0] == (0x40000000 | 336) && leaf.link[1] == 448 && leaf.link[2] == 7 && leaf.link[3] == 0);
    CHECK(branch.link[0] == 112 && branch.link[1] == 1008 && branch.link[2] == -1);
    const rts::Node32Rec l32 = rts::node32_record(b, 7, 5, 6, 100), b32 = rts::node32_record(b, -1, 5, 6, 100), wide = rts::node32_record(b, 7, 5, 6, 16384);
    CHECK(sizeof(l32) == 64 && l32.box[0] == -1.0f && l32.box[4] == rts::f32_down(0.1) && l32.box[5] == rts::f32_up(0.3) && l32.box[6] == l32.box[5] && l32.box[7] == l32.box[4]);
    CHECK(l32.link[0] == 384 && l32.link[1] == 384 && l32.link[2] == (0x4000 | 7) && l32.link[3] == 16);
    CHECK(b32.link[0] == 320 && b32.link[1] == 384 && b32.link[2] == 0 && b32.link[3] == 0);
    CHECK((uint32_t) wide.link[2] == (0x80000000u | 7u) && rts::node32_record(b, 7, 5, 6, 16383).link[2] == (0x4000 | 7));
    CHECK(rts::bmax_with(1e-30f, l32) == 4.0f && rts::bmax_with(5.0f, l32) == 5.0f);
    const rtt::Box nb{{std::nan(""), 0, 0}, {2.0, 0, 0}};
    CHECK(rts::bmax_with(1e-30f, rts::node32_record(nb, -1, 0, 0, 1)) == 2.0f); // a NaN coordinate leaves bmax alone
    std::printf("nodes ok\n");

    CHECK(!rts::flipped(1.0) && rts::flipped(-1.0) && !rts::flipped(0.0) && !rts::flipped(-0.0) && !rts::flipped(-9e-9) && rts::flipped(-2e-8) && !rts::flipped(std::nan("")));
    rts::ObjectRec g = rts::object_record(sphere(RT_SPHERE_GLASS, 1, 2, 3, -2.0));
    const double inv = 1.0 / 1.5, po = (1.0 - 1.5) / (1.0 + 1.5), pi = (1.0 - inv) / (1.0 + inv);
    CHECK(g.geo[0] == 1 && g.geo[3] == 4.0 && g.geo[4] == 0.75 && g.geo[5] == -2.0);
    CHECK(g.meta[0] == (int32_t) (0u | (6u << 2) | 32u) && g.meta[1] == (int32_t) (1u | (2u << 8) | (3u << 16)));
    CHECK(g.mat[0] == pi * pi && g.mat[1] == 1.5 && g.mat[2] == inv && g.mat[3] == po * po);
    rts::ObjectRec d = rts::object_record(sphere(RT_SPHERE_DIELECTRIC, 0, 0, 0, 1.0));
    CHECK(d.mat[0] == 0.0 && d.mat[1] == 1.5 && d.mat[2] == 0.5 && d.mat[3] == inv && d.meta[0] == (int32_t) (5u << 2));
    rt_hittable f = sphere(RT_SPHERE_FUZZED_REFLECTION, 0, 0, 0, 1.0);
    f.texture = 4;
    rts::ObjectRec fr = rts::object_record(f);
    CHECK(fr.mat[1] == 0.25 && fr.mat[3] == 0.0 && fr.meta[1] == (int32_t) (1u | (2u << 8) | (3u << 16) | (5u << 24)));
    rt_hittable p{};
    p.kind = RT_HITTABLE_INFINITE_PLANE; p.style = RT_PLANE_FUZZED_REFLECTION; p.point[1] = -1; p.normal[1] = 1; p.albedo = 0.5; p.fuzz = 0.125; p.texture = -1;
    rts::ObjectRec pr = rts::object_record(p);
    CHECK(pr.geo[1] == -1 && pr.geo[4] == 1 && pr.meta[0] == (int32_t) (2u | (3u << 2)) && pr.mat[0] == 0.5 && pr.mat[1] == 0.125 && pr.mat[2] == 0 && pr.mat[3] == 0);
    std::printf("objects ok\n");

    CHECK(rts::radius_ok(100.0) && !rts::radius_ok(std::nextafter(100.0, 200.0)) && !rts::radius_ok(0.0) && !rts::radius_ok(-1.0) && !rts::radius_ok(std::nan("")));
    CHECK(rts::box_implied(1000.0f, true, 0.5) == 1 && rts::box_implied(std::nextafterf(1000.0f, 2000.0f), true, 0.5) == 0);
    CHECK(rts::box_implied(10.0f, true, 50.0) == 1 && rts::box_implied(10.0f, true, std::nextafter(50.0, 60.0)) == 0);
    CHECK(rts::box_implied(10.0f, false, 1.0) == 0 && rts::box_implied(std::numeric_limits<float>::infinity(), true, 0.0) == 0 && rts::box_implied(1e-30f, true, 0.0) == 1);
    std::printf("implied ok\n");
}

int main() {
    checks();
    boxes();
    rounding();
    offsets();
    records();
    return failures ? 1 : 0;
}
