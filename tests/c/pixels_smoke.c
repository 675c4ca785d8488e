/* Plain-C consumer of the pixel-list entry points of include/rtfs_amd.h (rt_render_pixels, rt_render_pixels_extend and their
 * device variants): argument checks without a GPU; with one, ten pixels of a small frame -- out of order, one of them twice --
 * rendered as a list and printed for tests/test_gpu_pixels.py to hold against the oracle's frame.
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/pixels_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

#define MAX_W 12
#define MAX_H 7
#define COLS (2 * MAX_W + 1)
#define ROWS (2 * MAX_H + 1)
#define N_PX 10

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

    const double origin[3] = {0.0, 0.5, -2.0}, view[3] = {0.0, 0.0, 1.0}, up[3] = {0.0, 1.0, 0.0};
    rt_camera cam12, cam24;
    CHECK(rt_camera_make_basic(12, 1.0, (double) COLS / (double) ROWS, origin, view, up, &cam12) == RT_OK);
    cam12.bounce_depth = 10;
    cam24 = cam12;
    cam24.samples_per_pixel = 24;

    /* the four corners, the centre, pixels on the spheres and the floor; out of order; entry 9 repeats entry 2 */
    int32_t px[N_PX] = {ROWS * COLS - 1, 0, 7 * COLS + 12, COLS - 1, 9 * COLS + 20, 8 * COLS + 5, (ROWS - 1) * COLS, 6 * COLS + 18, 12 * COLS + 3,
                        7 * COLS + 12};
    int32_t accum[N_PX * 4];
    uint8_t rgb[N_PX * 3];
    rt_stats st;
    rt_render_options bad;
    memset(&bad, 0, sizeof(bad));
    bad.struct_size = sizeof(bad);
    bad.block_threads = 100;

    /* argument checks come first: nothing is written, no device is needed */
    memset(accum, 0x55, sizeof(accum));
    memset(rgb, 0x55, sizeof(rgb));
    CHECK(rt_render_pixels(NULL, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels(scene, NULL, MAX_W, MAX_H, 5, 0, N_PX, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels(scene, &cam24, 0, MAX_H, 5, 0, N_PX, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, NULL, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, NULL, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, (size_t) INT32_MAX + 1u, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels(scene, &cam24, 40000, 40000, 5, 0, N_PX, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT); /* > INT32_MAX pixels */
    CHECK(rt_render_pixels_device(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, accum, rgb, NULL, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels_extend(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, 11, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels_extend(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, 25, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels_extend_device(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, 12, NULL, rgb, NULL, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    /* an entry outside the frame: the host variants find it before any device call */
    px[4] = -1;
    CHECK(rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    px[4] = ROWS * COLS;
    CHECK(rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_pixels_extend(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, 12, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    px[4] = 9 * COLS + 20;
    CHECK(accum[0] == 0x55555555 && accum[N_PX * 4 - 1] == 0x55555555 && rgb[0] == 0x55 && rgb[N_PX * 3 - 1] == 0x55);
    /* empty lists, and target == samples_done, are no-ops with zeroed stats */
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, NULL, 0, NULL, NULL, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.kernel_ms == 0.0);
    CHECK(rt_render_pixels_device(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL) == RT_OK);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_pixels_extend(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, 24, accum, rgb, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && accum[0] == 0x55555555 && rgb[0] == 0x55);
    CHECK(rt_render_pixels_extend_device(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, NULL, 0, 12, NULL, NULL, NULL, NULL, NULL) == RT_OK);
    printf("pixels: argument checks ok\n");

    const int rc = rt_render_pixels(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, RT_RENDER_COUNTERS, accum, rgb, &st);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        CHECK(rt_render_pixels_extend(scene, &cam24, MAX_W, MAX_H, 5, 0, N_PX, px, 0, 12, accum, rgb, NULL) == RT_ERR_NO_DEVICE);
        CHECK(accum[0] == 0x55555555);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    uint64_t samples = 0;
    for (int i = 0; i < N_PX; ++i) samples += (uint64_t) accum[i * 4];
    CHECK(st.pixels == N_PX && st.samples == samples && st.rays >= samples);
    for (int i = 0; i < N_PX; ++i)
        printf("pixel %d %d %d %d %d %d %u %u %u\n", i, px[i], accum[i * 4], accum[i * 4 + 1], accum[i * 4 + 2], accum[i * 4 + 3], rgb[i * 3],
               rgb[i * 3 + 1], rgb[i * 3 + 2]);
    CHECK(memcmp(accum + 9 * 4, accum + 2 * 4, 16) == 0 && memcmp(rgb + 9 * 3, rgb + 2 * 3, 3) == 0); /* the duplicate */
    printf("pixels: rendered %d list entries on the GPU\n", N_PX);
    rt_scene_destroy(scene);
    return 0;
}
