/* Plain-C consumer of the extension-by-map entry points of include/rtfs_amd.h (rt_render_extend_map, rt_render_footprints_extend_map
 * and their device variants): argument checks without a GPU; with one, a small frame rendered at 12 samples per pixel, then continued
 * by a map that sends every even pixel to 24 and leaves the odd ones, compared pixel by pixel with direct renders at 24 and at 12,
 * with a digest printed for tests/test_gpu_extend_map.py to hold against the oracle's.
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/extend_map_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
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
#define N_PX (ROWS * COLS)

static uint64_t digest(const int32_t *accum, const uint8_t *rgb) { /* FNV-1a over the PixelStats words, then the rgb bytes */
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < N_PX * 4; ++i)
        for (int b = 0; b < 4; ++b) { h ^= (uint64_t) (((uint32_t) accum[i] >> (8 * b)) & 0xFFu); h *= 1099511628211ull; }
    for (int i = 0; i < N_PX * 3; ++i) { h ^= (uint64_t) rgb[i]; h *= 1099511628211ull; }
    return h;
}

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
    rt_camera cam12, cam24, cam11;
    CHECK(rt_camera_make_basic(12, 1.0, (double) COLS / (double) ROWS, origin, view, up, &cam12) == RT_OK);
    cam12.bounce_depth = 10;
    cam24 = cam12;
    cam24.samples_per_pixel = 24;
    cam11 = cam12;
    cam11.samples_per_pixel = 11;

    static int32_t accum[N_PX * 4], base[N_PX * 4], direct[N_PX * 4], targets[N_PX];
    static uint8_t rgb[N_PX * 3], rgb_base[N_PX * 3], rgb_direct[N_PX * 3];
    double fp[2 * 12] = {0.0, 0.5, -2.0, -0.2, -0.3, 1.0, 0.2, 0.0, 0.0, 0.0, 0.6, 0.0, 0.0, 0.5, -2.0, 0.0, -0.3, 1.0, 0.2, 0.0, 0.0, 0.0, 0.6, 0.0};
    rt_stats st;
    rt_render_options bad;
    memset(&bad, 0, sizeof(bad));
    bad.struct_size = sizeof(bad);
    bad.block_threads = 100;
    for (int i = 0; i < N_PX; ++i) targets[i] = (i % 2 == 0) ? 24 : 0;

    /* argument checks come first: nothing is written, no device is needed */
    memset(accum, 0x55, sizeof(accum));
    memset(rgb, 0x55, sizeof(rgb));
    CHECK(rt_render_extend_map(NULL, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_extend_map(scene, NULL, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_extend_map(scene, &cam11, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, NULL, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, NULL, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS + 1, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_extend_map_device(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, NULL, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints_extend_map(scene, 0, 2, fp, 11, 10, 5, 0, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints_extend_map(scene, 0, 2, fp, 24, 10, 5, 0, 0, NULL, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints_extend_map(scene, 0, 2, NULL, 24, 10, 5, 0, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_footprints_extend_map_device(scene, 0, 2, fp, 24, 10, 5, 0, 0, targets, NULL, rgb, NULL, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(accum[0] == 0x55555555 && accum[N_PX * 4 - 1] == 0x55555555 && rgb[0] == 0x55 && rgb[N_PX * 3 - 1] == 0x55);
    /* empty shards are no-ops with zeroed stats */
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, 0, 0, NULL, NULL, NULL, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.kernel_ms == 0.0);
    CHECK(rt_render_extend_map_device(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL) == RT_OK);
    CHECK(rt_render_footprints_extend_map(scene, 0, 0, NULL, 24, 10, 5, 0, 0, NULL, NULL, NULL, &st) == RT_OK);
    CHECK(rt_render_footprints_extend_map_device(scene, 0, 0, NULL, 24, 10, 5, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL) == RT_OK);
    printf("extend_map: argument checks ok\n");

    const int rc = rt_render(scene, &cam12, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, base, rgb_base, NULL);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, NULL) == RT_ERR_NO_DEVICE);
        CHECK(accum[0] == 0x55555555);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    memcpy(accum, base, sizeof(accum));
    memset(rgb, 0x55, sizeof(rgb));
    CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, &st) == RT_OK);
    CHECK(rt_render(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, direct, rgb_direct, NULL) == RT_OK);
    uint64_t added = 0, early = 0, continued = 0, left = 0;
    for (int i = 0; i < N_PX; ++i) {
        const int cont = base[i * 4] == 12 && targets[i] > 12;
        const int32_t *want = cont ? direct + i * 4 : base + i * 4;
        const uint8_t *want_rgb = cont ? rgb_direct + i * 3 : rgb_base + i * 3;
        CHECK(memcmp(accum + i * 4, want, 16) == 0 && memcmp(rgb + i * 3, want_rgb, 3) == 0);
        added += (uint64_t) (accum[i * 4] - base[i * 4]);
        early += base[i * 4] == 11;
        continued += (uint64_t) cont;
        left += base[i * 4] == 12 && !cont;
    }
    CHECK(st.pixels == N_PX && st.samples == added && added == 12 * continued && st.pixels_early == early && early > 0 && continued > 0 && left > 0);
    printf("extend_map: %d pixels, %llu final, %llu continued 12 -> 24, %llu left at 12, digest %016llx\n", N_PX, (unsigned long long) early,
           (unsigned long long) continued, (unsigned long long) left, (unsigned long long) digest(accum, rgb));
    /* a target above the cap: refused, unchanged */
    memcpy(direct, accum, sizeof(accum));
    for (int i = 0; i < N_PX; ++i) targets[i] = 25;
    memset(rgb, 0x55, sizeof(rgb));
    CHECK(rt_render_extend_map(scene, &cam24, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, targets, accum, rgb, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(memcmp(accum, direct, sizeof(accum)) == 0 && rgb[0] == 0x55 && rgb[N_PX * 3 - 1] == 0x55);
    printf("extend_map: a target above the cap is refused and the buffer left unchanged\n");
    rt_scene_destroy(scene);
    return 0;
}
