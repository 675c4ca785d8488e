/* Plain-C consumer of the ray-list entry points of include/rtfs_amd.h (rt_hit_objects, rt_trace_rays): argument checks
 * without a GPU; with one, the answers for a fixed scene and fixed rays, printed exactly (hex floats) for
 * tests/test_gpu_ray_queries.py to hold against the oracle.
 * Build: gcc -std=c99 -Wall -Werror -I include tests/c/ray_query_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

#define N_RAYS 8

int main(void) {
    /* the scene test_gpu_ray_queries.py rebuilds for the oracle: a Lambert sphere, a glass sphere, a fuzzed floor, a light dome */
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

    /* origin xyz, vector xyz: vectors of any length (Ray.make' unitises them on the device); the last is below the tolerance */
    const double rays[N_RAYS * 6] = {
        0.0, 0.0, 0.0, 0.0, 0.0, 1.0,      0.0, 0.0, 0.0, 1.5, 0.0, 4.0,      0.0, 0.0, 0.0, 0.0, -2.0, 5.0,
        0.0, 0.0, 0.0, 0.0, 1.0, 0.0,      0.3, 0.2, -1.0, 0.0, 0.0, 250.0,   5.0, 0.0, 3.0, -1e-3, 0.0, 0.0,
        1.5, 0.0, 4.0, 0.0, 0.0, 1.0,      0.0, 0.0, 0.0, 1e-5, 0.0, 0.0,
    };
    int32_t hit[N_RAYS];
    double strike[N_RAYS * 3];
    uint32_t rng[N_RAYS * 4];
    uint8_t colour[N_RAYS * 3];
    for (int i = 0; i < N_RAYS; ++i) { rng[i * 4] = 11u + (uint32_t) i; rng[i * 4 + 1] = 7u * (uint32_t) i + 3u; rng[i * 4 + 2] = 12345u; rng[i * 4 + 3] = 999u; }

    /* argument checks come first: nothing is written */
    memset(hit, 0x55, sizeof(hit));
    CHECK(rt_hit_objects(NULL, 0, N_RAYS, rays, 0, hit, strike, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_hit_objects(scene, 0, N_RAYS, NULL, 0, hit, strike, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_hit_objects(scene, 0, N_RAYS, rays, 0, NULL, strike, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_hit_objects(scene, 0, (size_t) INT32_MAX + 1u, rays, 0, hit, strike, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_trace_rays(scene, 0, N_RAYS, rays, rng, 0, 0, 0, -1, 0, colour, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_trace_rays(scene, 0, N_RAYS, rays, rng, 0, 0, 0, 5, 0, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(hit[0] == 0x55555555 && rng[0] == 11u);
    CHECK(rt_hit_objects(scene, 0, 0, NULL, 0, NULL, NULL, NULL) == RT_OK);
    CHECK(rt_trace_rays(scene, 0, 0, NULL, NULL, 0, 0, 0, 5, 0, NULL, NULL) == RT_OK);
    printf("ray queries: argument checks ok\n");

    const int rc = rt_hit_objects(scene, 0, N_RAYS, rays, 0, hit, strike, NULL);
    if (rt_device_count() == 0) {
        CHECK(rc == RT_ERR_NO_DEVICE);
        rt_scene_destroy(scene);
        return 0;
    }
    CHECK(rc == RT_OK);
    rt_stats st;
    CHECK(rt_trace_rays(scene, 0, N_RAYS, rays, rng, 0, 0, 0, 10, RT_RENDER_COUNTERS, colour, &st) == RT_OK);
    CHECK(st.rays >= N_RAYS - 1 && st.samples == 0 && st.pixels == 0);
    for (int i = 0; i < N_RAYS; ++i)
        printf("hit %d %d %a %a %a\n", i, hit[i], strike[i * 3], strike[i * 3 + 1], strike[i * 3 + 2]);
    for (int i = 0; i < N_RAYS; ++i)
        printf("trace %d %u %u %u %u %u %u %u\n", i, colour[i * 3], colour[i * 3 + 1], colour[i * 3 + 2], rng[i * 4], rng[i * 4 + 1], rng[i * 4 + 2], rng[i * 4 + 3]);
    /* the stream-keyed form: (seed 5, stream_base 100 + i, sample 2) */
    CHECK(rt_trace_rays(scene, 0, N_RAYS, rays, NULL, 5, 100, 2, 10, 0, colour, NULL) == RT_OK);
    for (int i = 0; i < N_RAYS; ++i) printf("stream %d %u %u %u\n", i, colour[i * 3], colour[i * 3 + 1], colour[i * 3 + 2]);
    printf("ray queries: traced %d rays on the GPU\n", N_RAYS);
    rt_scene_destroy(scene);
    return 0;
}
