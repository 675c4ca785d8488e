/* Plain-C consumer of rt_surfaces / rt_camera_surfaces (include/rtfs_amd.h): argument checks without a GPU; with one, ONE small frame's
 * normals and colours through rt_camera_surfaces, printed for tests/test_gpu_surfaces.py to hold against the composer (doubles as
 * their bit patterns).
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/surfaces_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
#include "rtfs_amd.h"

#include <inttypes.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

#define MAX_W 6
#define MAX_H 4
#define COLS (2 * MAX_W + 1)
#define ROWS (2 * MAX_H + 1)
#define SLOTS (ROWS * COLS)

static uint64_t bits(double d) {
    uint64_t u;
    memcpy(&u, &d, sizeof(u));
    return u;
}

int main(void) {
    /* camera_hits_smoke.c's scene: a Lambert sphere, a glass sphere, a fuzzed floor, a light dome */
    rt_hittable h[4];
    memset(h, 0, sizeof(h));
    h[0].kind = RT_HITTABLE_SPHERE; h[0].style = RT_SPHERE_LAMBERT_REFLECTION; h[0].point[2] = 3.0; h[0].radius = 1.0;
    h[0].albedo = 0.8; h[0].ior = 1.0; h[0].rgb[0] = 200; h[0].rgb[1] = 100; h[0].rgb[2] = 50; h[0].texture = -1;
    h[1].kind = RT_HITTABLE_SPHERE; h[1].style = RT_SPHERE_GLASS; h[1].point[0] = 1.5; h[1].point[2] = 4.0; h[1].radius = 0.7;
    h[1].albedo = 1.0; h[1].ior = 1.5; h[1].rgb[0] = h[1].rgb[1] = h[1].rgb[2] = 255; h[1].texture = -1;
    h[2].kind = RT_HITTABLE_INFINITE_PLANE; h[2].style = RT_PLANE_FUZZED_REFLECTION; h[2].point[1] = -1.0; h[2].normal[1] = 1.0;
    h[2].albedo = 0.9; h[2].fuzz = 0.2; h[2].ior = 1.0; h[2].rgb[0] = 180; h[2].rgb[1] = 200; h[2].rgb[2] = 220; h[2].texture = -1;
    h[3].kind = RT_HITTABLE_UNBOUNDED_SPHERE; h[3].style = RT_SPHERE_LIGHT_SOURCE; h[3].radius = 100.0;
    h[3].albedo = 1.0; h[3].ior = 1.0; h[3].rgb[0] = 230; h[3].rgb[1] = 230; h[3].rgb[2] = 255; h[3].texture = -1;
    rt_scene *scene = NULL;
    CHECK(rt_scene_create(h, 4, NULL, 0, &scene) == RT_OK);

    const double origin[3] = {0.0, 0.5, -2.0}, view[3] = {0.0, 0.0, 1.0}, up[3] = {0.0, 1.0, 0.0};
    rt_camera cam;
    CHECK(rt_camera_make_basic(24, 1.0, (double) COLS / (double) ROWS, origin, view, up, &cam) == RT_OK);
    cam.bounce_depth = 10;

    static int32_t hit[SLOTS];
    static double strike[SLOTS * 3], rays[SLOTS * 6], normal[SLOTS * 3];
    static uint8_t inside[SLOTS], colour[SLOTS * 3], tint[SLOTS * 3];
    rt_surface_outputs out, none, wrong;
    memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(out);
    out.normal = normal; out.inside = inside; out.colour = colour; out.tint = tint;
    memset(&none, 0, sizeof(none));
    none.struct_size = sizeof(none);
    wrong = out;
    wrong.struct_size = sizeof(out) - 8;
    rt_render_options bad;
    memset(&bad, 0, sizeof(bad));
    bad.struct_size = sizeof(bad);
    bad.block_threads = 100;
    rt_stats st;

    /* argument checks come first: nothing is written, no device is needed */
    memset(hit, 0, sizeof(hit));
    memset(strike, 0x55, sizeof(strike));
    memset(rays, 0x55, sizeof(rays));
    memset(normal, 0x55, sizeof(normal));
    memset(inside, 0x55, sizeof(inside));
    memset(colour, 0x55, sizeof(colour));
    memset(tint, 0x55, sizeof(tint));
    CHECK(rt_abi_sizeof(13) == sizeof(rt_surface_outputs) && rt_abi_offsetof(13, 5) == offsetof(rt_surface_outputs, uv) && rt_abi_offsetof(13, 6) == (size_t) -1);
    CHECK(rt_surfaces(NULL, 0, 8, hit, strike, rays, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, 8, NULL, strike, rays, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, 8, hit, NULL, rays, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, 8, hit, strike, NULL, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, 8, hit, strike, rays, 0, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, 8, hit, strike, rays, 0, &none, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, 8, hit, strike, rays, 0, &wrong, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces(scene, 0, (size_t) INT32_MAX + 1u, hit, strike, rays, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_surfaces_device(scene, 0, 8, hit, strike, rays, 0, &out, NULL, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    hit[5] = 4; /* an index the scene does not have: the host variant finds it before any device call */
    CHECK(rt_surfaces(scene, 0, 8, hit, strike, rays, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    hit[5] = -3;
    CHECK(rt_surfaces(scene, 0, 8, hit, strike, rays, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    hit[5] = 0;
    CHECK(rt_camera_surfaces(NULL, &cam, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 1, 0, hit, strike, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_surfaces(scene, NULL, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 1, 0, hit, strike, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_surfaces(scene, &cam, MAX_W, MAX_H, 5, 0, SLOTS + 1, NULL, 0, 1, 0, hit, strike, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_surfaces(scene, &cam, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 0, 0, hit, strike, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_surfaces(scene, &cam, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 1, 0, hit, strike, &none, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_surfaces(scene, &cam, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 1, 0, hit, strike, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_surfaces_device(scene, &cam, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 1, 0, hit, strike, &out, NULL, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(hit[0] == 0 && bits(strike[0]) == 0x5555555555555555ull && bits(normal[0]) == 0x5555555555555555ull && bits(normal[SLOTS * 3 - 1]) == 0x5555555555555555ull);
    CHECK(inside[0] == 0x55 && colour[SLOTS * 3 - 1] == 0x55 && tint[0] == 0x55);
    /* an empty list is a no-op with zeroed stats */
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_surfaces(scene, 0, 0, NULL, NULL, NULL, 0, &out, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.rays == 0 && st.kernel_ms == 0.0);
    CHECK(rt_camera_surfaces_device(scene, &cam, MAX_W, MAX_H, 5, 0, 0, NULL, 0, 1, 0, NULL, NULL, &out, NULL, NULL, NULL) == RT_OK);
    printf("surfaces: argument checks ok\n");

    /* the one frame */
    const int rc = rt_camera_surfaces(scene, &cam, MAX_W, MAX_H, 5, 0, SLOTS, NULL, 0, 1, 0, hit, strike, &out, &st);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        CHECK(bits(normal[0]) == 0x5555555555555555ull && colour[0] == 0x55);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    CHECK(st.pixels == SLOTS && st.samples == SLOTS && st.reflections == 0);
    for (int i = 0; i < SLOTS; ++i) {
        printf("slot %d %d", i, hit[i]);
        for (int k = 0; k < 3; ++k) printf(" %016" PRIx64, bits(strike[i * 3 + k]));
        for (int k = 0; k < 3; ++k) printf(" %016" PRIx64, bits(normal[i * 3 + k]));
        printf(" %d %d %d %d %d %d %d\n", inside[i], colour[i * 3], colour[i * 3 + 1], colour[i * 3 + 2], tint[i * 3], tint[i * 3 + 1], tint[i * 3 + 2]);
    }
    /* the same records from the hits themselves: every camera ray starts at the camera's origin */
    static double normal2[SLOTS * 3];
    static uint8_t colour2[SLOTS * 3];
    for (int i = 0; i < SLOTS; ++i)
        for (int k = 0; k < 6; ++k) rays[i * 6 + k] = k < 3 ? cam.view_origin[k] : 0.0;
    rt_surface_outputs two;
    memset(&two, 0, sizeof(two));
    two.struct_size = sizeof(two);
    two.normal = normal2; two.colour = colour2;
    CHECK(rt_surfaces(scene, 0, SLOTS, hit, strike, rays, 0, &two, &st) == RT_OK);
    CHECK(st.samples == SLOTS && memcmp(normal, normal2, sizeof(normal)) == 0 && memcmp(colour, colour2, sizeof(colour)) == 0);
    printf("surfaces: %d slots answered on the GPU\n", SLOTS);
    rt_scene_destroy(scene);
    return 0;
}
