/* Plain-C consumer of rt_camera_paths / rt_trace_paths (include/rtfs_amd.h): argument checks without a GPU; with one, ONE launch of
 * each family -- six pixels of a small frame, one of them twice, three samples each, four records a path; five rays, one with a zero
 * vector -- printed for tests/test_gpu_paths.py to hold against the composer.
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/paths_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
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
#define N_PX 6
#define FIRST 4
#define N_S 3
#define SLOTS (N_PX * N_S)
#define K 4
#define N_RAYS 5

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
    rt_camera cam;
    CHECK(rt_camera_make_basic(24, 1.0, (double) COLS / (double) ROWS, origin, view, up, &cam) == RT_OK);
    cam.bounce_depth = 10;

    int32_t px[N_PX] = {7 * COLS + 12, 0, 9 * COLS + 20, 8 * COLS + 5, ROWS * COLS - 1, 7 * COLS + 12}; /* entry 5 repeats entry 0 */
    const double rays[N_RAYS * 6] = {0.0, 0.5, -2.0, 0.0, 0.0, 1.0,   0.0, 0.5, -2.0, 0.7, -0.2, 2.0,   0.0, 0.5, -2.0, 0.0, 0.0, 0.0,
                                     0.0, 0.5, -2.0, 0.0, -1.0, 0.3,  5.0, 5.0, 5.0, -1.0, -1.0, -1.0};
    int32_t nv[SLOTS], end[SLOTS], hit[SLOTS * K], summary[N_PX * RT_PATH_SUMMARY_WORDS];
    uint8_t colour[SLOTS * 3], colour_after[SLOTS * K * 3];
    double first_ray[SLOTS * 6], strike[SLOTS * K * 3], ray_after[SLOTS * K * 6];
    rt_path_outputs out, bad;
    memset(&out, 0, sizeof(out));
    out.struct_size = sizeof(out); out.max_vertices = K;
    out.n_vertices = nv; out.end = end; out.colour = colour; out.first_ray = first_ray;
    out.hit_index = hit; out.strike = strike; out.colour_after = colour_after; out.ray_after = ray_after; out.summary = summary;
    rt_stats st;

    /* argument checks come first: nothing is written, no device is needed */
    memset(nv, 0x55, sizeof(nv));
    memset(summary, 0x55, sizeof(summary));
    CHECK(rt_camera_paths(NULL, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, 0, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    bad = out; bad.struct_size = 8;
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, 0, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    bad = out; bad.max_vertices = -1;
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, 0, &bad, NULL) == RT_ERR_INVALID_ARGUMENT);
    memset(&bad, 0, sizeof(bad)); bad.struct_size = sizeof(bad); bad.max_vertices = K;
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, 0, &bad, NULL) == RT_ERR_INVALID_ARGUMENT); /* every output NULL */
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, 0, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_trace_paths(scene, 0, N_RAYS, rays, NULL, 1, 0, 0, 10, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT); /* first_ray and summary: camera paths only */
    px[3] = ROWS * COLS;
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, 0, &out, NULL) == RT_ERR_INVALID_ARGUMENT); /* an entry outside the frame */
    px[3] = 8 * COLS + 5;
    CHECK(nv[0] == 0x55555555 && nv[SLOTS - 1] == 0x55555555 && summary[0] == 0x55555555);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, 0, NULL, 0, 1, 0, &out, &st) == RT_OK); /* an empty list is a no-op with zeroed stats */
    CHECK(st.samples == 0 && st.pixels == 0 && st.kernel_ms == 0.0);
    printf("paths: argument checks ok\n");

    /* the one launch of each family */
    int rc = rt_camera_paths(scene, &cam, MAX_W, MAX_H, 5, 0, N_PX, px, FIRST, N_S, RT_RENDER_COUNTERS, &out, &st);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        CHECK(nv[0] == 0x55555555);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    CHECK(st.pixels == N_PX && st.samples == SLOTS);
    uint64_t sum = 0;
    for (int i = 0; i < SLOTS; ++i) sum += (uint64_t) nv[i];
    CHECK(st.reflections == sum);
    printf("camera n_vertices:");
    for (int i = 0; i < SLOTS; ++i) printf(" %d", nv[i]);
    printf("\ncamera end:");
    for (int i = 0; i < SLOTS; ++i) printf(" %d", end[i]);
    printf("\ncamera colour:");
    for (int i = 0; i < SLOTS * 3; ++i) printf(" %d", colour[i]);
    printf("\n");
    CHECK(memcmp(nv + 5 * N_S, nv, N_S * sizeof(int32_t)) == 0 && memcmp(summary + 5 * RT_PATH_SUMMARY_WORDS, summary, RT_PATH_SUMMARY_WORDS * sizeof(int32_t)) == 0);
    CHECK(summary[0] == N_S && summary[12] == N_S);

    out.first_ray = NULL; out.summary = NULL;
    rc = rt_trace_paths(scene, 0, N_RAYS, rays, NULL, 9, 100, 2, 10, 0, &out, &st);
    CHECK(rc == RT_OK && st.pixels == N_RAYS && st.samples == N_RAYS);
    CHECK(end[2] == RT_PATH_NO_RAY && nv[2] == 0 && hit[2 * K] == -1);
    printf("rays n_vertices:");
    for (int i = 0; i < N_RAYS; ++i) printf(" %d", nv[i]);
    printf("\nrays colour:");
    for (int i = 0; i < N_RAYS * 3; ++i) printf(" %d", colour[i]);
    printf("\npaths: traced on the GPU\n");
    rt_scene_destroy(scene);
    return 0;
}
