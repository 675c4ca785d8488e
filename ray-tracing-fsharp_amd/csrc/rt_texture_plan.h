// rt_texture_plan.h -- where an image texture's texels lie in a scene's texel blob, and which byte of a bitmap lands on which byte of it.
// Plain C++ for host and device (no HIP calls), like rt_tree_plan.h: the host texture half (rt_scene.h), the kernel of rt_texture_kernels.h
// and tests/c/texture_plan_table.cpp all include this one definition.
//
// Layout.  IMAGE records in index order, width * height * 3 bytes each (rows of 3 * width bytes, no padding between rows), every image
// zero-padded to a multiple of 16 bytes; a record's texel_off is where its image starts.  Row y of an image is img.[y] of
// ParameterisedTexture.ofImage (Texture.fs:34): the bitmap's row height - 1 - y when the bitmap is "top first", as a decoder leaves it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_HD __host__ __device__
#else
#define RTX_HD
#endif

#define RTX_MAX_IMAGES 254   /* = the most texture records a scene takes */
#define RTX_UNIT 16u         /* the blob's granule: every image starts on one and is padded to one */
#define RTX_TOP_FIRST 1u     /* ImageEntry.flags: the source's rows are the bitmap's, top first */
#define RTX_FROM_DEVICE 2u   /* ImageEntry.flags: the image is placed by of_image_kernel (otherwise its range is somebody else's) */

namespace rtt {

static const uint64_t NO_BYTE = ~(uint64_t) 0; // source_index: the destination byte is padding
static const uint64_t MAX_BLOB = 0xFFFFFFFFull - 15u; // texel_off is 32 bits wide: the largest blob the new routes take

RTX_HD static inline uint64_t image_bytes(int32_t width, int32_t height) { return (uint64_t) (uint32_t) width * (uint64_t) (uint32_t) height * 3u; }
RTX_HD static inline uint64_t padded_bytes(int32_t width, int32_t height) { return (image_bytes(width, height) + (RTX_UNIT - 1u)) & ~(uint64_t) (RTX_UNIT - 1u); }

// off[i] for every record whose kind is image_kind (NO_BYTE for the others); returns the blob's size.  width, height > 0 for images.
static inline uint64_t texel_layout(const int32_t *kind, const int32_t *width, const int32_t *height, size_t n, int32_t image_kind, uint64_t *off) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        if (kind[i] != image_kind) { off[i] = NO_BYTE; continue; }
        off[i] = at;
        at += padded_bytes(width[i], height[i]);
    }
    return at;
}

// The byte of the source bitmap that lands on byte b of an image's padded range (b < padded_bytes), NO_BYTE for padding.
RTX_HD static inline uint64_t source_index(int32_t width, int32_t height, bool top_first, uint64_t b) {
    const uint64_t row = (uint64_t) (uint32_t) width * 3u;
    if (b >= row * (uint64_t) (uint32_t) height) return NO_BYTE;
    const uint64_t y = b / row, x = b - y * row;
#ifdef RTX_MUTANT_NO_FLIP
    top_first = false;
#endif
    return (top_first ? (uint64_t) (uint32_t) height - 1u - y : y) * row + x;
}

// source_index stepped: at() divides once, next() moves one destination byte on without dividing.
struct SourceCursor {
    uint64_t src;   // source_index of the current destination byte (meaningless once left == 0)
    uint64_t left;  // destination bytes of the image from the current one on; 0: padding from here
    uint32_t x, row; // byte within the row, bytes per row
    bool top_first;
};
RTX_HD static inline SourceCursor cursor_at(int32_t width, int32_t height, bool top_first, uint64_t b) {
    SourceCursor c;
    const uint64_t all = image_bytes(width, height);
    c.row = (uint32_t) width * 3u;
    c.top_first = top_first;
    c.left = b < all ? all - b : 0u;
    c.src = c.left ? source_index(width, height, top_first, b) : 0u;
    c.x = c.left ? (uint32_t) (b % c.row) : 0u;
    return c;
}
RTX_HD static inline void cursor_next(SourceCursor &c) {
    if (c.left == 0u) return;
    --c.left;
    ++c.src;
    if (++c.x == c.row) {
        c.x = 0u;
#ifndef RTX_MUTANT_NO_FLIP
        if (c.top_first && c.left) c.src -= 2u * (uint64_t) c.row; // the row above in the bitmap
#endif
    }
}

// The image a blob byte belongs to: the last i with offsets[i] <= blob_byte (offsets ascending, n <= RTX_MAX_IMAGES), -1 in front of the first.
RTX_HD static inline int32_t find_image(const uint64_t *offsets, uint32_t n, uint64_t blob_byte) {
    uint32_t lo = 0u, hi = n; // offsets[lo - 1] <= blob_byte < offsets[hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
#ifdef RTX_MUTANT_FIND
        if (offsets[mid] < blob_byte) lo = mid + 1u; else hi = mid;
#else
        if (offsets[mid] <= blob_byte) lo = mid + 1u; else hi = mid;
#endif
    }
    return (int32_t) lo - 1;
}

// One image of a table as of_image_kernel takes it.
struct ImageEntry {
    uint64_t off;       // where its padded range starts in the blob (a multiple of RTX_UNIT)
    const uint8_t *src; // the bitmap: height * width * 3 bytes, any alignment (RTX_FROM_DEVICE only)
    int32_t width, height;
    uint32_t flags, pad;
};

// What one lane of of_image_kernel does for the 16 blob bytes from `blob_byte` (a multiple of 16) on: false when they are not its to write
// (in front of the first image, behind the image's padded range, an image that is not device-sourced); otherwise out[0..16) and *valid =
// how many of them are texels (the rest is padding, 0).  Reads src[0 .. 3*width*height) only.
RTX_HD static inline bool place_unit(const uint64_t *offsets, const ImageEntry *entries, uint32_t n, uint64_t blob_byte, uint8_t out[16], uint32_t *valid) {
    const int32_t i = find_image(offsets, n, blob_byte);
    if (i < 0) return false;
    const ImageEntry e = entries[i];
    if (!(e.flags & RTX_FROM_DEVICE)) return false;
    const uint64_t b = blob_byte - e.off;
    if (b >= padded_bytes(e.width, e.height)) return false;
    SourceCursor c = cursor_at(e.width, e.height, (e.flags & RTX_TOP_FIRST) != 0u, b);
    *valid = c.left < RTX_UNIT ? (uint32_t) c.left : RTX_UNIT;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < RTX_UNIT; ++k) {
#ifdef RTX_MUTANT_PADDING
        out[k] = c.left ? e.src[c.src] : (uint8_t) 0xFF;
#else
        out[k] = c.left ? e.src[c.src] : (uint8_t) 0;
#endif
        cursor_next(c);
    }
    return true;
}

} // namespace rtt
