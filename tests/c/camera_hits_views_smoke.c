/* Plain-C consumer of rt_camera_hits_views / rt_camera_hits_views_device (include/rtfs_amd.h): argument checks without a GPU; with one,
 * ONE launch -- three cameras over a 9 x 7 frame, six of its pixels out of order, one of them twice, two samples each, a seed per view --
 * printed for tests/test_gpu_camera_hits_views.py to hold against three single rt_camera_hits calls (doubles as their bit patterns).
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/camera_hits_views_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
#include "rtfs_amd.h"

#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

#define MAX_W 4
#define MAX_H 3
#define COLS (2 * MAX_W + 1)
#define ROWS (2 * MAX_H + 1)
#define K 3
#define N_PX 6
#define FIRST 4
#define N_S 2
#define SLOTS (K * N_PX * N_S)

static uint64_t bits(double d) {
    uint64_t u;
    memcpy(&u, &d, sizeof(u));
    return u;
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

    /* three eyes on a line, the same view direction; the cameras differ in samples_per_pixel and bounce_depth, which a batch admits */
    const double origins[K][3] = {{0.0, 0.5, -2.0}, {1.0, 0.5, -2.0}, {-1.5, 1.0, -2.5}}, view[3] = {0.0, 0.0, 1.0}, up[3] = {0.0, 1.0, 0.0};
    const uint64_t seeds[K] = {5, 5, 11};
    rt_camera cams[K], badcams[K];
    for (int v = 0; v < K; ++v) {
        CHECK(rt_camera_make_basic(24 + v, 1.0, (double) COLS / (double) ROWS, origins[v], view, up, &cams[v]) == RT_OK);
        cams[v].bounce_depth = 10 + v;
    }

    /* corners, the centre, a pixel on the floor; out of order; entry 5 repeats entry 1 */
    int32_t px[N_PX] = {ROWS * COLS - 1, 3 * COLS + 4, 0, COLS - 1, 5 * COLS + 2, 3 * COLS + 4};
    int32_t hit[SLOTS];
    double strike[SLOTS * 3], rays[SLOTS * 6];
    rt_stats st;
    rt_render_options bad;
    memset(&bad, 0, sizeof(bad));
    bad.struct_size = sizeof(bad);
    bad.block_threads = 100;

    /* argument checks come first: nothing is written, no device is needed */
    memset(hit, 0x55, sizeof(hit));
    memset(strike, 0x55, sizeof(strike));
    memset(rays, 0x55, sizeof(rays));
    CHECK(rt_camera_hits_views(NULL, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, -1, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, NULL, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, K, 0, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    memcpy(badcams, cams, sizeof(cams)); badcams[2].samples_per_pixel = 0;
    CHECK(rt_camera_hits_views(scene, badcams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, -1, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, 0, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, (size_t) INT32_MAX / 4u, px, 0, 2, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, NULL, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, ROWS * COLS + 1, NULL, 0, 1, 0, hit, NULL, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_hits_views_device(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    /* an entry outside the frame: the host variant finds it before any device call */
    px[4] = ROWS * COLS;
    CHECK(rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, 0, hit, strike, rays, NULL) == RT_ERR_INVALID_ARGUMENT);
    px[4] = 5 * COLS + 2;
    CHECK(hit[0] == 0x55555555 && hit[SLOTS - 1] == 0x55555555);
    CHECK(bits(strike[0]) == 0x5555555555555555ull && bits(strike[SLOTS * 3 - 1]) == 0x5555555555555555ull);
    CHECK(bits(rays[0]) == 0x5555555555555555ull && bits(rays[SLOTS * 6 - 1]) == 0x5555555555555555ull);
    /* no views, or an empty list, is a no-op with zeroed stats */
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_camera_hits_views(scene, NULL, 0, MAX_W, MAX_H, NULL, 0, 0, N_PX, px, 0, 1, 0, NULL, NULL, NULL, &st) == RT_OK);
    CHECK(st.samples == 0 && st.pixels == 0 && st.rays == 0 && st.kernel_ms == 0.0);
    CHECK(rt_camera_hits_views_device(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, 0, NULL, 0, 1, 0, NULL, NULL, NULL, NULL, NULL, NULL) == RT_OK);
    printf("camera hits views: argument checks ok\n");

    /* the one launch */
    const int rc = rt_camera_hits_views(scene, cams, K, MAX_W, MAX_H, seeds, 0, 0, N_PX, px, FIRST, N_S, RT_RENDER_COUNTERS, hit, strike, rays, &st);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        CHECK(hit[0] == 0x55555555);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    CHECK(st.pixels == K * N_PX && st.samples == SLOTS && st.rays == SLOTS && st.reflections == 0);
    for (int i = 0; i < SLOTS; ++i) {
        printf("slot %d %d %d %d %d", i, i / (N_PX * N_S), px[(i / N_S) % N_PX], FIRST + i % N_S, hit[i]);
        for (int k = 0; k < 3; ++k) printf(" %016" PRIx64, bits(strike[i * 3 + k]));
        for (int k = 0; k < 6; ++k) printf(" %016" PRIx64, bits(rays[i * 6 + k]));
        printf("\n");
    }
    for (int v = 0; v < K; ++v) { /* the duplicate, in every view */
        CHECK(memcmp(hit + (v * N_PX + 5) * N_S, hit + (v * N_PX + 1) * N_S, N_S * sizeof(int32_t)) == 0);
        CHECK(memcmp(rays + (v * N_PX + 5) * N_S * 6, rays + (v * N_PX + 1) * N_S * 6, N_S * 6 * sizeof(double)) == 0);
    }
    printf("camera hits views: %d slots answered on the GPU\n", SLOTS);
    rt_scene_destroy(scene);
    return 0;
}
