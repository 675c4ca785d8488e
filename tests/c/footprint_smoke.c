/* Plain-C consumer of the footprint entry points of include/rtfs_amd.h (rt_render_footprints and its device variant): argument
 * checks without a GPU; with one, eight pixels of a fixed scene, printed for tests/test_gpu_footprints.py to hold against the
 * oracle's composition.
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/footprint_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

#define N_PX 8

int main(void) {
    /* ray_query_smoke.c's scene: a Lambert sphere, a glass sphere, a fuzzed floor, a light dome */
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

    /* a strip of eight pixels seen from (0, 0.5, -2): origin, base, du, dv; the last one is degenerate (base = du = dv = 0) */
    double fp[N_PX * 12];
    for (int i = 0; i < N_PX; ++i) {
        const double one[12] = {0.0, 0.5, -2.0, -0.8 + 0.2 * i, -0.3, 1.0, 0.2, 0.0, 0.0, 0.0, 0.6, 0.0};
        memcpy(fp + i * 12, one, sizeof(one));
    }
    memset(fp + 7 * 12 + 3, 0, 9 * sizeof(double));
    int32_t accum[N_PX * 4];
    uint8_t rgb[N_PX * 3];
    rt_stats st;
    rt_render_options bad;
    memset(&bad, 0, sizeof(bad));
    bad.struct_size = sizeof(bad);
    bad.block_threads = 100;

    /* argument checks come first: nothing is written */
    memset(accum, 0x55, sizeof(accum));
    memset(rgb, 0x55, sizeof(rgb));
    CHECK(rt_render_footprints(NULL, 0, N_PX, fp, 20, 10, 5, 100, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints(scene, 0, N_PX, NULL, 20, 10, 5, 100, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints(scene, 0, N_PX, fp, 20, 10, 5, 100, 0, NULL, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints(scene, 0, (size_t) INT32_MAX + 1u, fp, 20, 10, 5, 100, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints(scene, 0, N_PX, fp, 0, 10, 5, 100, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints(scene, 0, N_PX, fp, 20, -1, 5, 100, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints(scene, 0, N_PX, fp, 20, 0x1000000, 5, 100, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints_device(scene, 0, N_PX, fp, 20, 10, 5, 100, 0, accum, rgb, NULL, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(accum[0] == 0x55555555 && accum[N_PX * 4 - 1] == 0x55555555 && rgb[0] == 0x55);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_footprints(scene, 0, 0, NULL, 20, 10, 5, 100, 0, NULL, NULL, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.kernel_ms == 0.0);
    CHECK(rt_render_footprints_device(scene, 0, 0, NULL, 20, 10, 5, 100, 0, NULL, NULL, NULL, NULL, NULL) == RT_OK);
    printf("footprints: argument checks ok\n");

    const int rc = rt_render_footprints(scene, 0, N_PX, fp, 20, 10, 5, 100, RT_RENDER_COUNTERS, accum, rgb, &st);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        CHECK(accum[0] == 0x55555555);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    uint64_t samples = 0;
    for (int i = 0; i < N_PX; ++i) samples += (uint64_t) accum[i * 4];
    CHECK(st.pixels == N_PX && st.samples == samples && st.rays >= samples - 11u && st.pixels_early >= 1u);
    for (int i = 0; i < N_PX; ++i)
        printf("pixel %d %d %d %d %d %u %u %u\n", i, accum[i * 4], accum[i * 4 + 1], accum[i * 4 + 2], accum[i * 4 + 3], rgb[i * 3],
               rgb[i * 3 + 1], rgb[i * 3 + 2]);
    /* the timed variant, without rgb, gives the same sums */
    int32_t again[N_PX * 4];
    CHECK(rt_render_footprints(scene, 0, N_PX, fp, 20, 10, 5, 100, 0, again, NULL, NULL) == RT_OK);
    CHECK(memcmp(again, accum, sizeof(accum)) == 0);
    printf("footprints: rendered %d pixels on the GPU\n", N_PX);
    rt_scene_destroy(scene);
    return 0;
}
