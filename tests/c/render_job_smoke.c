/* Plain-C consumer of the render-job entry points of include/rtfs_amd.h (rt_render_job_start .. rt_render_job_destroy,
 * rt_format_pixel_map_present and its device form): argument checks without a GPU; with one, a small frame rendered as a job that a
 * budget stops after three units, its partial spill, and the frame finished -- held here against rt_render's frame, byte for byte.
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/render_job_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lamdhip64 -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the three HIP runtime calls a C program needs to own device buffers (hip_runtime_api.h is C++-flavoured; these are its C symbols) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind);
#define HIP_D2H 2

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

#define MAX_W 12
#define MAX_H 7
#define COLS (2 * MAX_W + 1)
#define ROWS (2 * MAX_H + 1)
#define NPX (ROWS * COLS)

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

    /* argument checks come first: nothing is written, no device is needed (the pointers below are never followed) */
    static int32_t accum[NPX * 4], want_accum[NPX * 4];
    static uint8_t rgb[NPX * 3], want_rgb[NPX * 3], present[NPX], spill[NPX * 25], spill_d[NPX * 25];
    rt_render_job *job = (rt_render_job *) (uintptr_t) 0x5A5A;
    rt_job_progress pr;
    rt_job_result res;
    memset(&pr, 0, sizeof(pr)); pr.struct_size = sizeof(pr);
    memset(&res, 0, sizeof(res)); res.struct_size = sizeof(res);
    CHECK(rt_render_job_start(NULL, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, accum, rgb, present, NULL, NULL, &job) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_start(scene, NULL, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, accum, rgb, present, NULL, NULL, &job) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS + 1, 0, accum, rgb, present, NULL, NULL, &job) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, NULL, rgb, present, NULL, NULL, &job) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, accum, rgb, NULL, NULL, NULL, &job) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, accum, rgb, present, NULL, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, RT_RENDER_COUNTERS, accum, rgb, present, NULL, NULL, &job) == RT_ERR_UNSUPPORTED);
    CHECK(job == (rt_render_job *) (uintptr_t) 0x5A5A);
    CHECK(rt_render_job_progress(NULL, &pr) == RT_ERR_INVALID_ARGUMENT && rt_render_job_stop(NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_job_wait(NULL, &res, NULL) == RT_ERR_INVALID_ARGUMENT && rt_render_job_finish(NULL, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    rt_render_job_destroy(NULL);
    /* the host formatter: two pixels of a 2x2 image */
    {
        const uint8_t px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, here[4] = {0, 1, 0, 1};
        const uint8_t expect[11] = {',', '1', '\n', 4, 5, 6, '1', ',', '1', '\n', 10};
        uint8_t out[16];
        CHECK(rt_format_pixel_map_present(px, here, 2, 2, out, sizeof(out)) == 13);
        CHECK(memcmp(out, expect, 11) == 0 && out[11] == 11 && out[12] == 12);
        CHECK(rt_format_pixel_map_present(NULL, here, 2, 2, out, sizeof(out)) == -RT_ERR_INVALID_ARGUMENT);
    }
    printf("render job: argument checks ok\n");

    if (rt_device_count() == 0) {
        CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, accum, rgb, present, NULL, NULL, &job) == RT_ERR_NO_DEVICE);
        CHECK(job == (rt_render_job *) (uintptr_t) 0x5A5A);
        rt_scene_destroy(scene);
        return 0;
    }

    CHECK(rt_render(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, want_accum, want_rgb, NULL) == RT_OK);
    unsigned char *d = NULL; /* accum, rgb, present, spill */
    const size_t rgb_at = (size_t) NPX * 16u, present_at = rgb_at + (size_t) NPX * 3u + 5u, spill_at = present_at + NPX + 3u;
    CHECK(hipMalloc((void **) &d, spill_at + sizeof(spill)) == 0);
    rt_render_options opt;
    memset(&opt, 0, sizeof(opt));
    opt.struct_size = sizeof(opt);
    opt.passes = 1;
    opt.chunk_pixels = 16;
    CHECK(rt_dev_set_job_limits(3, -1) == RT_OK); /* exactly units 0, 1 and 2 of 16 pixels */
    CHECK(rt_render_job_start(scene, &cam, MAX_W, MAX_H, 5, 0, 0, 1, ROWS, 0, d, d + rgb_at, d + present_at, NULL, &opt, &job) == RT_OK);
    CHECK(rt_render_job_progress(job, &pr) == RT_OK && pr.pixels_total == NPX && pr.pixels_final <= NPX && pr.state != 1);
    rt_stats st;
    CHECK(rt_render_job_wait(job, &res, &st) == RT_OK);
    int64_t plan[8];
    CHECK(rt_dev_last_job_plan(plan) == RT_OK && plan[0] == 1 && plan[1] == 16 && plan[2] == (NPX + 15) / 16 && plan[4] == 3);
    CHECK(res.complete == 0 && res.stop_requested == 0 && res.pixels_total == NPX && res.n_present == 48 && st.pixels == 48);
    CHECK(rt_render_job_progress(job, &pr) == RT_OK && pr.state == 2 && pr.pixels_final == 48);
    CHECK(hipMemcpy(accum, d, sizeof(accum), HIP_D2H) == 0 && hipMemcpy(rgb, d + rgb_at, sizeof(rgb), HIP_D2H) == 0);
    CHECK(hipMemcpy(present, d + present_at, sizeof(present), HIP_D2H) == 0);
    for (int i = 0; i < NPX; ++i) {
        CHECK(present[i] == (i < 48 ? 1 : 0));
        if (i < 48) CHECK(memcmp(accum + i * 4, want_accum + i * 4, 16) == 0 && memcmp(rgb + i * 3, want_rgb + i * 3, 3) == 0);
        else CHECK(accum[i * 4] == 0 && accum[i * 4 + 3] == 0 && rgb[i * 3] == 0 && rgb[i * 3 + 2] == 0);
    }
    /* the partial spill, on the device and on the host */
    int64_t n_d = 0;
    CHECK(rt_format_pixel_map_present_device(0, d + rgb_at, d + present_at, ROWS, COLS, d + spill_at, sizeof(spill), NULL, NULL, &n_d) == RT_OK);
    const int64_t n_h = rt_format_pixel_map_present(rgb, present, ROWS, COLS, spill, sizeof(spill));
    CHECK(n_h > 0 && n_h == n_d && hipMemcpy(spill_d, d + spill_at, (size_t) n_d, HIP_D2H) == 0 && memcmp(spill, spill_d, (size_t) n_h) == 0);
    /* and the rest of the frame */
    CHECK(rt_render_job_finish(job, NULL, &st) == RT_OK && st.pixels == NPX - 48);
    CHECK(hipMemcpy(accum, d, sizeof(accum), HIP_D2H) == 0 && hipMemcpy(rgb, d + rgb_at, sizeof(rgb), HIP_D2H) == 0);
    CHECK(hipMemcpy(present, d + present_at, sizeof(present), HIP_D2H) == 0);
    CHECK(memcmp(accum, want_accum, sizeof(accum)) == 0 && memcmp(rgb, want_rgb, sizeof(rgb)) == 0);
    for (int i = 0; i < NPX; ++i) CHECK(present[i] == 1);
    rt_render_job_destroy(job);
    CHECK(hipFree(d) == 0);
    printf("render job: %d of %d pixels before the budget, the frame finished on the GPU\n", 48, NPX);
    rt_scene_destroy(scene);
    return 0;
}
