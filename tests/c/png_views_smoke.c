/* Plain-C consumer of the batch PNG entry points of include/rtfs_amd.h (rt_png_views_max_bytes, rt_format_png_views_device,
 * rt_write_png_views_device): three copies-with-a-twist of the 3x2 image of the reference's PPM example -- the image, its channel-reversed
 * form and its negative -- encoded on the device in one call and printed for tests/test_gpu_png_views.py to hold against the host
 * formatter and a decoder.  argv[1]: a directory for the files it writes.
 * Build: gcc -std=c99 -pedantic -Wall -Werror -I include tests/c/png_views_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lamdhip64 -lm */
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

#define K 3

int main(int argc, char **argv) {
    const uint8_t golden[18] = {255, 0, 0, 0, 255, 0, 0, 0, 255, 255, 255, 0, 255, 255, 255, 0, 0, 0}; /* TestPpmOutput.fs:12-46 */
    uint8_t images[K * 18];
    unsigned char files[K * 128 + 64], one[128];
    char names[K][1024];
    const char *paths[K];
    int64_t offsets[K + 1] = {-7, -7, -7, -7}, on_device[K + 1], capacity, total;
    void *d_rgb = NULL, *d_out = NULL, *d_offsets = NULL;
    int v, i;

    if (argc < 2) { fprintf(stderr, "usage: png_views_smoke <directory>\n"); return 2; }
    for (i = 0; i < 18; ++i) {
        images[i] = golden[i];
        images[18 + i] = golden[i - i % 3 + 2 - i % 3]; /* B, G, R */
        images[36 + i] = (uint8_t) (255 - golden[i]);
    }
    for (v = 0; v < K; ++v) { snprintf(names[v], sizeof(names[v]), "%s/c_view%d.png", argv[1], v); paths[v] = names[v]; }

    /* host arithmetic and the refusals: before any device is entered, nothing written */
    capacity = rt_png_views_max_bytes(K, 2, 3);
    CHECK(capacity == K * rt_png_max_bytes(2, 3) && capacity <= K * 128);
    CHECK(rt_png_views_max_bytes(-1, 2, 3) == -RT_ERR_INVALID_ARGUMENT && rt_png_views_max_bytes(K, 0, 3) == -RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_png_views_max_bytes(2, 27000, 27000) == -RT_ERR_UNSUPPORTED && rt_png_views_max_bytes(K, 27000, 27000) == -RT_ERR_INVALID_ARGUMENT); /* the batch's bound first */
    memset(files, 0x55, sizeof(files));
    CHECK(rt_format_png_views_device(0, NULL, K, 2, 3, 0, files, sizeof(files), NULL, NULL, offsets) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_views_device(0, images, -1, 2, 3, 0, files, sizeof(files), NULL, NULL, offsets) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_format_png_views_device(0, images, K, 2, 3, 0, files, 0, NULL, NULL, offsets) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_write_png_views_device(NULL, 0, images, K, 2, 3, 0, NULL) == RT_ERR_INVALID_ARGUMENT);
    CHECK(offsets[0] == -7 && files[0] == 0x55);
    CHECK(rt_format_png_views_device(0, NULL, 0, 2, 3, 0, NULL, 0, NULL, NULL, offsets) == RT_OK && offsets[0] == 0 && offsets[1] == -7); /* no view */
    printf("png views: refusals ok\n");
    if (rt_device_count() == 0) {
        CHECK(rt_format_png_views_device(0, images, K, 2, 3, 0, files, sizeof(files), NULL, NULL, offsets) == RT_ERR_NO_DEVICE);
        CHECK(rt_write_png_views_device(paths, 0, images, K, 2, 3, 0, NULL) == RT_ERR_NO_DEVICE);
        printf("png views: no device, no fallback\n");
        return 0;
    }

    /* the three images on the device; the output buffer 64 bytes larger than asked and full of a sentinel */
    CHECK(hipMalloc(&d_rgb, sizeof(images)) == 0 && hipMalloc(&d_out, sizeof(files)) == 0 && hipMalloc(&d_offsets, sizeof(on_device)) == 0);
    CHECK(hipMemcpy(d_rgb, images, sizeof(images), 1) == 0 && hipMemcpy(d_out, files, sizeof(files), 1) == 0);
    CHECK(rt_format_png_views_device(0, d_rgb, K, 2, 3, 0, d_out, (size_t) capacity, d_offsets, NULL, offsets) == RT_OK);
    CHECK(hipMemcpy(files, d_out, sizeof(files), 2) == 0 && hipMemcpy(on_device, d_offsets, sizeof(on_device), 2) == 0);
    total = offsets[K];
    CHECK(offsets[0] == 0 && total <= capacity && files[total] == 0x55 && files[sizeof(files) - 1] == 0x55);
    for (v = 0; v < K; ++v) { /* file v is rt_format_png of image v */
        const int64_t n = rt_format_png(images + 18 * v, 2, 3, 0, one, sizeof(one));
        CHECK(n > 68 && offsets[v + 1] - offsets[v] == n && memcmp(files + offsets[v], one, (size_t) n) == 0);
        printf("file%d ", v);
        for (i = 0; i < (int) n; ++i) printf("%02x", files[offsets[v] + i]);
        printf("\n");
    }
    for (v = 0; v <= K; ++v) CHECK(on_device[v] == offsets[v]);
    /* one byte too few: refused on the device, nothing written */
    memset(files, 0x55, sizeof(files));
    CHECK(hipMemcpy(d_out, files, sizeof(files), 1) == 0);
    CHECK(rt_format_png_views_device(0, d_rgb, K, 2, 3, 0, d_out, (size_t) total - 1, NULL, NULL, offsets) == RT_ERR_INVALID_ARGUMENT && offsets[K] == total);
    CHECK(hipMemcpy(files, d_out, sizeof(files), 2) == 0 && files[0] == 0x55 && files[total - 2] == 0x55);
    CHECK(rt_write_png_views_device(paths, 0, d_rgb, K, 2, 3, 0, NULL) == RT_OK);
    CHECK(hipFree(d_rgb) == 0 && hipFree(d_out) == 0 && hipFree(d_offsets) == 0);
    printf("png views: encoded on the GPU\n");
    return 0;
}
