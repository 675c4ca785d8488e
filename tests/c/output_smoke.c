/* Plain-C consumer of the device output entry points of include/rtfs_amd.h (rt_ppm_max_bytes, rt_pixel_map_bytes,
 * rt_gamma_correct_device, rt_format_ppm_device, rt_format_pixel_map_device, rt_write_ppm_device, rt_render_ppm): the host arithmetic
 * and every refusal without a GPU; with one, the 3x2 image of the reference's PPM example formatted, gamma-corrected, written and
 * printed for tests/test_gpu_output.py to hold against tests/golden/PpmOutputExample.txt and the oracle.  argv[1]: a directory for
 * the files it writes.
 * Build: gcc -std=c99 -pedantic -Wall -Werror -I include tests/c/output_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lamdhip64 -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

/* the three HIP runtime calls a C program needs to own device memory (hip_runtime_api.h is C++ in places; hipMemcpyKind: 1 host to
 * device, 2 device to host) */
extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind);

static void print_hex(const char *name, const unsigned char *p, int64_t n) {
    int64_t i;
    printf("%s ", name);
    for (i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    const uint8_t image[18] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 255, 255, 0, 255, 255, 255, 0, 0, 0}; /* TestPpmOutput.fs:12-46 */
    unsigned char text[256 + 64];
    char path[1024], bad_path[1100];
    int64_t length = -7;
    rt_stats st;
    rt_camera cam;
    rt_hittable h[1];
    rt_scene *scene = NULL;
    const double origin[3] = {0.0, 0.0, 0.0}, view[3] = {0.0, 0.0, 1.0}, up[3] = {0.0, 1.0, 0.0};
    void *d_rgb = NULL, *d_out = NULL, *d_len = NULL;

    if (argc < 2) { fprintf(stderr, "usage: output_smoke <directory>\n"); return 2; }
    snprintf(path, sizeof(path), "%s/c_write.ppm", argv[1]);
    snprintf(bad_path, sizeof(bad_path), "%s/no-such-directory/x.ppm", argv[1]);

    /* host arithmetic */
    CHECK(rt_ppm_max_bytes(2, 3) == 11 + 12 * 6 - 1);
    CHECK(rt_ppm_max_bytes(1601, 2401) == 46128028);
    CHECK(rt_ppm_max_bytes(0, 3) == -RT_ERR_INVALID_ARGUMENT && rt_ppm_max_bytes(3, -1) == -RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_ppm_max_bytes(65536, 65536) == -RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_pixel_map_bytes(2, 3) == 5 * 6 + 3 * 1 + 2 * 2); /* rows 0, 1: one digit over three pixels; cols 0, 1, 2: two digits per row */
    CHECK(rt_pixel_map_bytes(0, 3) == -RT_ERR_INVALID_ARGUMENT && rt_pixel_map_bytes(65536, 65536) == -RT_ERR_INVALID_ARGUMENT);

    /* refusals: before any device is entered, nothing written */
    memset(text, 0x55, sizeof(text));
    CHECK(rt_format_ppm_device(0, NULL, 2, 3, 0, text, sizeof(text), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_ppm_device(0, image, 0, 3, 0, text, sizeof(text), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_ppm_device(0, image, 2, -3, 0, text, sizeof(text), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_ppm_device(0, image, 65536, 65536, 0, text, sizeof(text), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_ppm_device(0, image, 2, 3, 0, text, 0, NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_pixel_map_device(0, NULL, 2, 3, text, sizeof(text), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_pixel_map_device(0, image, 2, 0, text, sizeof(text), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_pixel_map_device(0, image, 2, 3, text, 0, NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_gamma_correct_device(0, 18, NULL, text, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_gamma_correct_device(0, 18, image, NULL, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_gamma_correct_device(0, 0, NULL, NULL, NULL) == RT_OK);
    CHECK(rt_write_ppm_device(NULL, 0, image, 2, 3, 0, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_ppm_device(path, 0, NULL, 2, 3, 0, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_ppm_device(bad_path, 0, image, 2, 3, 0, NULL) == RT_ERR_IO);
    CHECK(length == -7 && text[0] == 0x55 && text[sizeof(text) - 1] == 0x55);

    memset(h, 0, sizeof(h));
    h[0].kind = RT_HITTABLE_UNBOUNDED_SPHERE; h[0].style = RT_SPHERE_LIGHT_SOURCE; h[0].radius = 100.0;
    h[0].albedo = 1.0; h[0].ior = 1.0; h[0].rgb[0] = 230; h[0].rgb[1] = 120; h[0].rgb[2] = 7; h[0].texture = -1;
    CHECK(rt_scene_create(h, 1, NULL, 0, &scene) == RT_OK);
    CHECK(rt_camera_make_basic(12, 1.0, 3.0, origin, view, up, &cam) == RT_OK);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_ppm(NULL, &cam, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_ppm(scene, NULL, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_ppm(scene, &cam, 0, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_ppm(scene, &cam, 1, 1, 5, 0, 0, 1, NULL, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_ppm(scene, &cam, 1, 1, 5, 0, 0, 1, bad_path, NULL, &st) == RT_ERR_IO);
    CHECK(((unsigned char *) &st)[0] == 0x55);
    printf("output: refusals ok\n");

    if (rt_device_count() == 0) {
        CHECK(rt_format_ppm_device(0, image, 2, 3, 0, text, sizeof(text), NULL, NULL, &length) == RT_ERR_NO_DEVICE);
        CHECK(rt_format_pixel_map_device(0, image, 2, 3, text, sizeof(text), NULL, NULL, &length) == RT_ERR_NO_DEVICE);
        CHECK(rt_gamma_correct_device(0, 18, image, text, NULL) == RT_ERR_NO_DEVICE);
        CHECK(rt_write_ppm_device(path, 0, image, 2, 3, 0, NULL) == RT_ERR_NO_DEVICE);
        CHECK(rt_render_ppm(scene, &cam, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_NO_DEVICE);
        CHECK(length == -7 && text[0] == 0x55);
        printf("output: no device, no fallback\n");
        rt_scene_destroy(scene);
        return 0;
    }

    /* the 3x2 image on the device; the text buffer 64 bytes larger than asked and full of a sentinel */
    CHECK(hipMalloc(&d_rgb, 18) == 0 && hipMalloc(&d_out, sizeof(text)) == 0 && hipMalloc(&d_len, 8) == 0);
    CHECK(hipMemcpy(d_rgb, image, 18, 1) == 0 && hipMemcpy(d_out, text, sizeof(text), 1) == 0);
    CHECK(rt_format_ppm_device(0, d_rgb, 2, 3, 0, d_out, 256, d_len, NULL, &length) == RT_OK);
    CHECK(hipMemcpy(text, d_out, sizeof(text), 2) == 0);
    CHECK(length == 62 && text[62] == 0x55 && text[sizeof(text) - 1] == 0x55);
    print_hex("ppm", text, length);
    { int64_t on_device = 0; CHECK(hipMemcpy(&on_device, d_len, 8, 2) == 0 && on_device == 62); }
    /* one byte too few: refused on the device, nothing written */
    memset(text, 0x55, sizeof(text));
    CHECK(hipMemcpy(d_out, text, sizeof(text), 1) == 0);
    CHECK(rt_format_ppm_device(0, d_rgb, 2, 3, 0, d_out, 61, NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT && length == 62);
    CHECK(hipMemcpy(text, d_out, sizeof(text), 2) == 0 && text[0] == 0x55 && text[60] == 0x55);
    CHECK(rt_format_ppm_device(0, d_rgb, 2, 3, 1, NULL, 0, NULL, NULL, &length) == RT_OK && length > 0); /* length only */
    CHECK(rt_format_pixel_map_device(0, d_rgb, 2, 3, d_out, 256, NULL, NULL, &length) == RT_OK && length == rt_pixel_map_bytes(2, 3));
    CHECK(hipMemcpy(text, d_out, sizeof(text), 2) == 0);
    print_hex("map", text, length);
    CHECK(rt_gamma_correct_device(0, 18, d_rgb, d_out, NULL) == RT_OK);
    CHECK(hipMemcpy(text, d_out, 18, 2) == 0); /* (the null stream: the copy waits for the kernel) */
    print_hex("gamma", text, 18);
    CHECK(rt_write_ppm_device(path, 0, d_rgb, 2, 3, 0, NULL) == RT_OK);
    snprintf(path, sizeof(path), "%s/c_render.ppm", argv[1]);
    CHECK(rt_render_ppm(scene, &cam, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_OK);
    CHECK(st.pixels == 9 && st.samples > 0 && st.total_ms >= st.kernel_ms);
    CHECK(hipFree(d_rgb) == 0 && hipFree(d_out) == 0 && hipFree(d_len) == 0);
    printf("output: formatted on the GPU\n");
    rt_scene_destroy(scene);
    return 0;
}
