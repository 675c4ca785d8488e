/* Plain-C consumer of the PNG entry points of include/rtfs_amd.h (rt_format_png, rt_write_png, rt_png_max_bytes, rt_png_tile_bytes,
 * rt_format_png_device, rt_write_png_device, rt_render_png): the host formatter, the host arithmetic and every refusal without a GPU;
 * with one, the 3x2 image of the reference's PPM example encoded on the device and printed for tests/test_gpu_png.py to hold against
 * the host formatter and a decoder.  argv[1]: a directory for the files it writes.
 * Build: gcc -std=c99 -pedantic -Wall -Werror -I include tests/c/png_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lamdhip64 -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind); /* 1 host to device, 2 device to host */

static void print_hex(const char *name, const unsigned char *p, int64_t n) {
    int64_t i;
    printf("%s ", name);
    for (i = 0; i < n; ++i) printf("%02x", p[i]);
    printf("\n");
}

int main(int argc, char **argv) {
    const uint8_t image[18] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 255, 255, 0, 255, 255, 255, 0, 0, 0}; /* TestPpmOutput.fs:12-46 */
    const unsigned char signature[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    unsigned char file[256 + 64], host_file[256];
    char path[1024], bad_path[1100];
    int64_t length = -7, host_length;
    rt_stats st;
    rt_camera cam;
    rt_hittable h[1];
    rt_scene *scene = NULL;
    const double origin[3] = {0.0, 0.0, 0.0}, view[3] = {0.0, 0.0, 1.0}, up[3] = {0.0, 1.0, 0.0};
    void *d_rgb = NULL, *d_out = NULL, *d_len = NULL;

    if (argc < 2) { fprintf(stderr, "usage: png_smoke <directory>\n"); return 2; }
    snprintf(path, sizeof(path), "%s/c_write.png", argv[1]);
    snprintf(bad_path, sizeof(bad_path), "%s/no-such-directory/x.png", argv[1]);

    /* host arithmetic and the host formatter */
    CHECK(rt_png_tile_bytes() > 0);
    CHECK(rt_png_max_bytes(2, 3) == 68 + 2 * 10 + 5);
    CHECK(rt_png_max_bytes(0, 3) == -RT_ERR_INVALID_ARGUMENT && rt_png_max_bytes(65536, 65536) == -RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_png_max_bytes(27000, 27000) == -RT_ERR_UNSUPPORTED);
    host_length = rt_format_png(image, 2, 3, 0, NULL, 0); /* the length only */
    CHECK(host_length > 68 && host_length <= rt_png_max_bytes(2, 3));
    memset(host_file, 0x55, sizeof(host_file));
    CHECK(rt_format_png(image, 2, 3, 0, host_file, (size_t) host_length - 1) == -RT_ERR_INVALID_ARGUMENT && host_file[0] == 0x55); /* nothing written */
    CHECK(rt_format_png(image, 2, 3, 0, host_file, (size_t) host_length) == host_length);
    CHECK(memcmp(host_file, signature, 8) == 0 && host_file[host_length] == 0x55);
    CHECK(rt_format_png(NULL, 2, 3, 0, host_file, sizeof(host_file)) == -RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png(image, 0, 3, 0, host_file, sizeof(host_file)) == -RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_png(NULL, image, 2, 3, 0) == RT_ERR_INVALID_ARGUMENT && rt_write_png(path, NULL, 2, 3, 0) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_png(bad_path, image, 2, 3, 0) == RT_ERR_IO);
    CHECK(rt_write_png(path, image, 2, 3, 0) == RT_OK);
    print_hex("host", host_file, host_length);

    /* refusals of the device calls: before any device is entered, nothing written */
    memset(file, 0x55, sizeof(file));
    CHECK(rt_format_png_device(0, NULL, 2, 3, 0, file, sizeof(file), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_device(0, image, 0, 3, 0, file, sizeof(file), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_device(0, image, 2, -3, 0, file, sizeof(file), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_device(0, image, 65536, 65536, 0, file, sizeof(file), NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_device(0, image, 2, 3, 0, file, 0, NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_device(0, image, 27000, 27000, 0, file, sizeof(file), NULL, NULL, &length) == RT_ERR_UNSUPPORTED);
    CHECK(rt_write_png_device(NULL, 0, image, 2, 3, 0, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_png_device(path, 0, NULL, 2, 3, 0, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_png_device(bad_path, 0, image, 2, 3, 0, NULL) == RT_ERR_IO);
    CHECK(length == -7 && file[0] == 0x55 && file[sizeof(file) - 1] == 0x55);

    memset(h, 0, sizeof(h));
    h[0].kind = RT_HITTABLE_UNBOUNDED_SPHERE; h[0].style = RT_SPHERE_LIGHT_SOURCE; h[0].radius = 100.0;
    h[0].albedo = 1.0; h[0].ior = 1.0; h[0].rgb[0] = 230; h[0].rgb[1] = 120; h[0].rgb[2] = 7; h[0].texture = -1;
    CHECK(rt_scene_create(h, 1, NULL, 0, &scene) == RT_OK);
    CHECK(rt_camera_make_basic(12, 1.0, 3.0, origin, view, up, &cam) == RT_OK);
    memset(&st, 0x55, sizeof(st));
    CHECK(rt_render_png(NULL, &cam, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_png(scene, NULL, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_png(scene, &cam, 0, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_png(scene, &cam, 1, 1, 5, 0, 0, 1, NULL, NULL, &st) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_render_png(scene, &cam, 1, 1, 5, 0, 0, 1, bad_path, NULL, &st) == RT_ERR_IO);
    CHECK(((unsigned char *) &st)[0] == 0x55);
    printf("png: refusals ok\n");

    if (rt_device_count() == 0) {
        CHECK(rt_format_png_device(0, image, 2, 3, 0, file, sizeof(file), NULL, NULL, &length) == RT_ERR_NO_DEVICE);
        CHECK(rt_format_png_device(0, image, 2, 3, 0, NULL, 0, NULL, NULL, &length) == RT_ERR_NO_DEVICE);
        snprintf(path, sizeof(path), "%s/c_device.png", argv[1]);
        CHECK(rt_write_png_device(path, 0, image, 2, 3, 0, NULL) == RT_ERR_NO_DEVICE);
        CHECK(rt_render_png(scene, &cam, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_ERR_NO_DEVICE);
        CHECK(length == -7 && file[0] == 0x55);
        printf("png: no device, no fallback\n");
        rt_scene_destroy(scene);
        return 0;
    }

    /* the 3x2 image on the device; the output buffer 64 bytes larger than asked and full of a sentinel */
    CHECK(hipMalloc(&d_rgb, 18) == 0 && hipMalloc(&d_out, sizeof(file)) == 0 && hipMalloc(&d_len, 8) == 0);
    CHECK(hipMemcpy(d_rgb, image, 18, 1) == 0 && hipMemcpy(d_out, file, sizeof(file), 1) == 0);
    CHECK(rt_format_png_device(0, d_rgb, 2, 3, 0, d_out, 256, d_len, NULL, &length) == RT_OK);
    CHECK(hipMemcpy(file, d_out, sizeof(file), 2) == 0);
    CHECK(length == host_length && memcmp(file, host_file, (size_t) length) == 0 && file[length] == 0x55 && file[sizeof(file) - 1] == 0x55);
    print_hex("device", file, length);
    { int64_t on_device = 0; CHECK(hipMemcpy(&on_device, d_len, 8, 2) == 0 && on_device == host_length); }
    /* one byte too few: refused on the device, nothing written */
    memset(file, 0x55, sizeof(file));
    CHECK(hipMemcpy(d_out, file, sizeof(file), 1) == 0);
    CHECK(rt_format_png_device(0, d_rgb, 2, 3, 0, d_out, (size_t) host_length - 1, NULL, NULL, &length) == RT_ERR_INVALID_ARGUMENT && length == host_length);
    CHECK(hipMemcpy(file, d_out, sizeof(file), 2) == 0 && file[0] == 0x55 && file[host_length - 2] == 0x55);
    CHECK(rt_format_png_device(0, d_rgb, 2, 3, 1, NULL, 0, NULL, NULL, &length) == RT_OK && length > 68); /* length only */
    snprintf(path, sizeof(path), "%s/c_device.png", argv[1]);
    CHECK(rt_write_png_device(path, 0, d_rgb, 2, 3, 0, NULL) == RT_OK);
    snprintf(path, sizeof(path), "%s/c_render.png", argv[1]);
    CHECK(rt_render_png(scene, &cam, 1, 1, 5, 0, 0, 1, path, NULL, &st) == RT_OK);
    CHECK(st.pixels == 9 && st.samples > 0 && st.total_ms >= st.kernel_ms);
    CHECK(hipFree(d_rgb) == 0 && hipFree(d_out) == 0 && hipFree(d_len) == 0);
    printf("png: encoded on the GPU\n");
    rt_scene_destroy(scene);
    return 0;
}
