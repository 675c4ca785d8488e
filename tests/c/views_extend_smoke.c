/* Plain-C consumer of rt_render_views_extend(_device) and rt_render_views_extend_map(_device) (include/rtfs_amd.h): the argument checks only.
 * Every call below is refused, or is a no-op, before any device call, so the program needs no GPU and LAUNCHES NOTHING (the GPU coverage
 * of these entry points is tests/test_gpu_views_extend.py's, from Python).
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/views_extend_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)
#define REFUSED(call, text) CHECK((call) == RT_ERR_INVALID_ARGUMENT && strcmp(rt_last_error(), text) == 0)

#define MAX_W 4
#define MAX_H 3
#define COLS (2 * MAX_W + 1)
#define ROWS (2 * MAX_H + 1)
#define K 3
#define PX (K * ROWS * COLS)

int main(void) {
    rt_hittable h[1];
    memset(h, 0, sizeof(h));
    h[0].kind = RT_HITTABLE_SPHERE; h[0].style = RT_SPHERE_LAMBERT_REFLECTION; h[0].point[2] = 3.0; h[0].radius = 1.0;
    h[0].albedo = 0.8; h[0].ior = 1.0; h[0].rgb[0] = 200; h[0].rgb[1] = 100; h[0].rgb[2] = 50; h[0].texture = -1;
    rt_scene *scene = NULL;
    CHECK(rt_scene_create(h, 1, NULL, 0, &scene) == RT_OK);

    const double origin[3] = {0.0, 0.0, -1.0}, view[3] = {0.0, 0.0, 1.0}, up[3] = {0.0, 1.0, 0.0};
    const uint64_t seeds[K] = {5, 5, 9};
    rt_camera cams[K], other[K];
    for (int v = 0; v < K; ++v) {
        CHECK(rt_camera_make_basic(40, 1.0, (double) COLS / (double) ROWS, origin, view, up, &cams[v]) == RT_OK);
        cams[v].bounce_depth = 3;
    }
    static int32_t accum[PX * 4], targets[PX];
    static uint8_t rgb[PX * 3];
    memset(accum, 0x55, sizeof(accum));
    memset(rgb, 0x55, sizeof(rgb));
    for (int i = 0; i < PX; ++i) targets[i] = 40;
    rt_stats st;
    rt_render_options bad;
    memset(&bad, 0, sizeof(bad));
    bad.struct_size = sizeof(bad);
    bad.block_threads = 100;

    /* the batch's own checks, with the batch's messages */
    REFUSED(rt_render_views_extend(NULL, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 12, accum, rgb, NULL), "scene is NULL");
    REFUSED(rt_render_views_extend(scene, NULL, K, MAX_W, MAX_H, seeds, 0, 0, 0, 12, accum, rgb, NULL), "cameras is NULL");
    REFUSED(rt_render_views_extend(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 12, NULL, rgb, NULL), "accum is NULL");
    REFUSED(rt_render_views_extend(scene, cams, -1, MAX_W, MAX_H, seeds, 0, 0, 0, 12, accum, rgb, NULL), "n_views must be >= 0");
    REFUSED(rt_render_views_extend_map(NULL, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, targets, accum, rgb, NULL), "scene is NULL");
    REFUSED(rt_render_views_extend_map(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, targets, NULL, rgb, NULL), "accum is NULL");
    memcpy(other, cams, sizeof(cams)); other[2].samples_per_pixel = 41;
    REFUSED(rt_render_views_extend(scene, other, K, MAX_W, MAX_H, seeds, 0, 0, 0, 12, accum, rgb, NULL),
            "the cameras of a batch must share samples_per_pixel and bounce_depth");
    REFUSED(rt_render_views_extend_map_device(scene, other, K, MAX_W, MAX_H, seeds, 0, 0, 0, targets, accum, rgb, NULL, NULL, NULL),
            "the cameras of a batch must share samples_per_pixel and bounce_depth");
    REFUSED(rt_render_views_extend_device(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 12, accum, rgb, NULL, &bad, NULL),
            "block_threads must be 0, 256, 512, 768 or 1024");
    REFUSED(rt_render_views_extend_map_device(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, targets, accum, rgb, NULL, &bad, NULL),
            "block_threads must be 0, 256, 512, 768 or 1024");
    /* ... then the extension's, with the extension's */
    REFUSED(rt_render_views_extend(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 11, accum, rgb, NULL),
            "samples_done must be >= 12 (below, firstTrial differs and Count cannot tell a stopped pixel from a finished one)");
    REFUSED(rt_render_views_extend_device(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 41, accum, rgb, NULL, NULL, NULL),
            "the target samples_per_pixel is below samples_done");
    REFUSED(rt_render_views_extend_map(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, NULL, accum, rgb, NULL), "targets is NULL");
    for (int v = 0; v < K; ++v) other[v].samples_per_pixel = 11;
    REFUSED(rt_render_views_extend_map(scene, other, K, MAX_W, MAX_H, seeds, 0, 0, 0, targets, accum, rgb, NULL),
            "a map's samples_per_pixel (the bound on every target) must be >= 12 (a buffer rendered below cannot be continued)");
    /* no views, and a target equal to samples_done: no-ops with zeroed stats */
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_views_extend(scene, NULL, 0, MAX_W, MAX_H, NULL, 0, 0, 0, 12, NULL, NULL, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.rays == 0 && st.kernel_ms == 0.0);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_views_extend_map_device(scene, NULL, 0, MAX_W, MAX_H, NULL, 0, 0, 0, NULL, NULL, NULL, NULL, NULL, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.rays == 0 && st.kernel_ms == 0.0);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_views_extend(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 40, accum, rgb, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.rays == 0 && st.kernel_ms == 0.0);
    CHECK(rt_render_views_extend_device(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, 40, accum, rgb, NULL, NULL, NULL) == RT_OK);
    /* nothing was written by any of them */
    for (int i = 0; i < PX * 4; ++i) CHECK(accum[i] == 0x55555555);
    for (int i = 0; i < PX * 3; ++i) CHECK(rgb[i] == 0x55);
    printf("views extend: argument checks ok\n");
    rt_scene_destroy(scene);
    return 0;
}
