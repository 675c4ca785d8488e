/* Plain-C consumer of the JPEG entry points of include/rtfs_amd.h (rt_jpeg_get_info, rt_decode_jpeg, rt_decode_jpeg_device): the host
 * decoder and every refusal without a GPU; with one, the same file decoded on the device and held to the host decoder's bitmap, and a
 * damaged file refused there with the output untouched.  argv[1]: a baseline JPEG; argv[2]: the same file with its scan damaged.
 * Build: gcc -std=c99 -pedantic -Wall -Werror -I include tests/c/jpeg_smoke.c -L ray-tracing-fsharp_amd -lrtfs_amd -lamdhip64 -lm */
#include "rtfs_amd.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { fprintf(stderr, "FAILED %s (line %d): %s\n", #cond, __LINE__, rt_last_error()); return 1; } \
    } while (0)

extern int hipMalloc(void **ptr, size_t size);
extern int hipFree(void *ptr);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind); /* 1 host to device, 2 device to host */
extern int hipMemset(void *dst, int value, size_t size);

static uint8_t *read_file(const char *path, size_t *n) {
    FILE *f = fopen(path, "rb");
    uint8_t *p;
    long len;
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    len = ftell(f);
    fseek(f, 0, SEEK_SET);
    p = (uint8_t *) malloc((size_t) len + 1);
    *n = fread(p, 1, (size_t) len, f);
    fclose(f);
    return p;
}

int main(int argc, char **argv) {
    size_t n = 0, n_bad = 0, bytes, i;
    uint8_t *file, *damaged, *host, *back;
    rt_jpeg_info info;
    rt_jpeg_stats stats;
    void *d_rgb = NULL;
    unsigned long sum = 0;

    if (argc < 3) { fprintf(stderr, "usage: jpeg_smoke <file.jpg> <damaged.jpg>\n"); return 2; }
    file = read_file(argv[1], &n);
    damaged = read_file(argv[2], &n_bad);
    CHECK(file != NULL && damaged != NULL && n > 4 && n_bad > 4);

    memset(&info, 0, sizeof(info));
    info.struct_size = sizeof(info);
    CHECK(rt_jpeg_get_info(file, n, &info) == RT_OK);
    CHECK(info.width > 0 && info.height > 0 && (info.components == 1 || info.components == 3) && info.entropy_bytes > 0 && (size_t) info.entropy_bytes < n);
    CHECK(info.sampling >= RT_JPEG_GREY && info.sampling <= RT_JPEG_420);
    bytes = (size_t) info.width * (size_t) info.height * 3u;
    host = (uint8_t *) malloc(bytes + 1);
    back = (uint8_t *) malloc(bytes + 1);
    memset(host, 0x55, bytes + 1);
    CHECK(rt_decode_jpeg(file, n, host, bytes - 1) == RT_ERR_INVALID_ARGUMENT && host[0] == 0x55); /* nothing written */
    CHECK(rt_decode_jpeg(NULL, n, host, bytes) == RT_ERR_INVALID_ARGUMENT && rt_decode_jpeg(file, n, NULL, bytes) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_decode_jpeg(file, 1, host, bytes) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_decode_jpeg(damaged, n_bad, host, bytes) == RT_ERR_INVALID_ARGUMENT && host[0] == 0x55 && host[bytes - 1] == 0x55);
    CHECK(rt_decode_jpeg(file, n, host, bytes) == RT_OK && host[bytes] == 0x55);
    for (i = 0; i < bytes; ++i) sum += host[i];
    printf("host %dx%d sum %lu\n", info.width, info.height, sum);

    /* refusals of the device call: before any device is entered */
    memset(&stats, 0, sizeof(stats));
    stats.struct_size = sizeof(stats);
    CHECK(rt_decode_jpeg_device(0, NULL, n, back, bytes, NULL, &stats) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_decode_jpeg_device(0, file, n, NULL, bytes, NULL, &stats) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_decode_jpeg_device(0, file, n, back, bytes - 1, NULL, &stats) == RT_ERR_INVALID_ARGUMENT);
    CHECK(rt_decode_jpeg_device(0, file, 2, back, bytes, NULL, &stats) == RT_ERR_INVALID_ARGUMENT);
    stats.struct_size = 4;
    CHECK(rt_decode_jpeg_device(0, file, n, back, bytes, NULL, &stats) == RT_ERR_INVALID_ARGUMENT);
    stats.struct_size = sizeof(stats);
    printf("jpeg: refusals ok\n");

    if (rt_device_count() == 0) {
        CHECK(rt_decode_jpeg_device(0, file, n, back, bytes, NULL, &stats) == RT_ERR_NO_DEVICE);
        printf("jpeg: no device, no fallback\n");
        return 0;
    }

    CHECK(hipMalloc(&d_rgb, bytes + 1) == 0 && hipMemset(d_rgb, 0x55, bytes + 1) == 0);
    CHECK(rt_decode_jpeg_device(0, damaged, n_bad, d_rgb, bytes, NULL, &stats) == RT_ERR_INVALID_ARGUMENT);
    CHECK(hipMemcpy(back, d_rgb, bytes + 1, 2) == 0);
    for (i = 0; i <= bytes; ++i) CHECK(back[i] == 0x55); /* nothing written */
    CHECK(rt_decode_jpeg_device(0, file, n, d_rgb, bytes, NULL, &stats) == RT_OK);
    CHECK(hipMemcpy(back, d_rgb, bytes + 1, 2) == 0);
    CHECK(memcmp(back, host, bytes) == 0 && back[bytes] == 0x55);
    CHECK(stats.rounds >= 1 && stats.rounds <= stats.subsequences && stats.decodes >= stats.subsequences && stats.blocks > 0 && stats.total_ms > 0.0);
    CHECK(hipFree(d_rgb) == 0);
    printf("jpeg: decoded on the GPU, %ld subsequences, %ld rounds\n", (long) stats.subsequences, (long) stats.rounds);
    free(file); free(damaged); free(host); free(back);
    return 0;
}
