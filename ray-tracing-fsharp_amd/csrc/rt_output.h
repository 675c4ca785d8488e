// rt_output.h -- the output stage on the device: ImageOutput.writePpm's P3 text (ImageOutput.fs:163-197, PixelOutput.toPpm :20-30), the
// pixel-map bytes of ImageOutput.resume / toPpm (ImageOutput.fs:115-161) and PixelOutput.correct over a buffer (ImageOutput.fs:11-18).
// Pure byte arithmetic with a byte-exact contract: the host formatters rth::format_ppm / rth::format_pixel_map (rt_scene.h) are what
// every byte is held to.  DESIGN.md "Output on the device".
//
// A pixel's text has a variable length (P3: 5..11 bytes and 0 or 1 separator; pixel map: 5..25), so where a pixel's bytes go is a
// prefix sum over lengths.  Three launches on the caller's stream, and NO workgroup ever waits for another:
//   format_sums_kernel     one workgroup per tile of RTO_TILE_PIXELS pixels: the tile's byte count
//   format_scan_kernel     ONE workgroup: the exclusive scan of the tile counts (64-bit: a frame's text may pass 2^31 bytes), in trips of
//                          RTO_SCAN_THREADS with the running total in that workgroup's own registers; it also stores the total length and
//                          decides -- on the device, in front of the scatter -- whether the caller's buffer can hold it
//   format_scatter_kernel  one workgroup per tile: recomputes the lengths, scans them inside the tile, assembles the tile's contiguous
//                          byte range in LDS and copies it out with aligned dword stores; the ragged head and tail bytes go out as
//                          bytes, so no byte outside [offset, offset + length) is touched (the neighbouring tiles own those bytes, and
//                          the caller's buffer may end right there)
// d_rgb and d_out may have any byte alignment: both copies are "bytes up to the first aligned dword, dwords, bytes after the last".
//
// Gamma has ONE definition, rth::gamma_correct: the host fills a 256-byte table from it (the identity when gamma is off) and hands it
// over by value; nothing here restates it.  Each workgroup turns the table into "up to three ASCII digits + digit count" per byte
// value in LDS, so a channel is one LDS lookup.
#pragma once

#include "rt_launch_consts.h"

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rto {

enum { FMT_PPM = 0, FMT_MAP = 1 };

struct GammaTable { unsigned char v[256]; };          // PixelOutput.correct of every byte value, or the identity
struct PpmHeader { unsigned char text[32]; uint32_t len; }; // "P3\n<cols> <rows>\n255\n" (at most 29 bytes)

// Head of a format call's stream-ordered scratch; the tile counts / offsets (one uint64 per tile) follow at RTO_SCRATCH_HEAD.
struct FormatScratch {
    long long total;  // the length the output needs
    unsigned int go;  // 1: d_out is given and holds `total` bytes -- the scatter writes; 0: it writes nothing
    unsigned int pad;
};
static_assert(sizeof(FormatScratch) == RTO_SCRATCH_HEAD, "the tile array follows the head");

template <int FMT> struct Fmt;
template <> struct Fmt<FMT_PPM> { enum { MAX_BYTES = RTO_PPM_PIXEL_BYTES }; };
template <> struct Fmt<FMT_MAP> { enum { MAX_BYTES = RTO_MAP_PIXEL_BYTES }; };

// ---- pieces ------------------------------------------------------------------------------------------------------------------

// v in 0..255 as its decimal digits, left-aligned in bytes 0..2, the digit count in byte 3
__device__ inline uint32_t digit_entry(uint32_t v) {
    const uint32_t h = v / 100u, t = (v / 10u) % 10u, o = v % 10u;
    if (v >= 100u) return (48u + h) | ((48u + t) << 8) | ((48u + o) << 16) | (3u << 24);
    if (v >= 10u) return (48u + t) | ((48u + o) << 8) | (2u << 24);
    return (48u + o) | (1u << 24);
}
__device__ inline void fill_digit_table(uint32_t *tab, const GammaTable &g) { // 256 entries, any block size
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) tab[i] = digit_entry(g.v[i]);
}

// writeAsciiInt (ImageOutput.fs:115-129): the decimal digits of v, and NO digit for 0
__device__ inline uint32_t ascii_int_len(uint32_t v) {
    return (v > 0u) + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
__device__ inline uint32_t put_ascii_int(unsigned char *dst, uint32_t v) {
    const uint32_t n = ascii_int_len(v);
    for (uint32_t k = n; k-- > 0u;) { dst[k] = (unsigned char) (48u + v % 10u); v /= 10u; }
    return n;
}
__device__ inline uint32_t put_digits(unsigned char *dst, uint32_t entry) {
    const uint32_t n = entry >> 24;
    dst[0] = (unsigned char) entry;
    if (n > 1u) dst[1] = (unsigned char) (entry >> 8);
    if (n > 2u) dst[2] = (unsigned char) (entry >> 16);
    return n;
}

// Bytes of pixel g = (r, c) with colour p[0..2]; `last` = the image's last pixel, which alone has no separator behind it.
template <int FMT> __device__ inline uint32_t pixel_len(const uint32_t *tab, const unsigned char *p, uint32_t g, uint32_t r, uint32_t c, uint32_t last) {
    if (FMT == FMT_PPM) return (tab[p[0]] >> 24) + (tab[p[1]] >> 24) + (tab[p[2]] >> 24) + 2u + (g != last ? 1u : 0u);
    return ascii_int_len(r) + ascii_int_len(c) + 5u; // ',' '\n' R G B
}
template <int FMT> __device__ inline uint32_t put_pixel(unsigned char *dst, const uint32_t *tab, const unsigned char *p, uint32_t g, uint32_t r, uint32_t c,
                                                         uint32_t last, uint32_t cols) {
    uint32_t n = 0;
    if (FMT == FMT_PPM) {
        n += put_digits(dst + n, tab[p[0]]); dst[n++] = ' ';
        n += put_digits(dst + n, tab[p[1]]); dst[n++] = ' ';
        n += put_digits(dst + n, tab[p[2]]);
        if (g != last) dst[n++] = c == cols - 1u ? '\n' : ' '; // one space between a row's pixels, '\n' between rows, nothing at the end
    } else {
        n += put_ascii_int(dst + n, r); dst[n++] = ',';
        n += put_ascii_int(dst + n, c); dst[n++] = '\n';
        dst[n++] = p[0]; dst[n++] = p[1]; dst[n++] = p[2];
    }
    return n;
}

// Exclusive scan of one value per thread over the workgroup; `total` = the sum over all of it.  wave_tot: LDS, BLOCK / 64 entries,
// free again on return.
template <class T, int BLOCK> __device__ inline T block_exclusive_scan(T v, T *wave_tot, T &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t) d) inc += o;
    }
    if (lane == 63u) wave_tot[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (uint32_t w = 0; w < (uint32_t) (BLOCK / 64); ++w) {
        const T x = wave_tot[w];
        if (w < wave) base += x;
        tot += x;
    }
    total = tot;
    __syncthreads();
    return base + inc - v;
}

// len bytes between global memory and LDS, for a global address of ANY alignment a = address & 3: LDS byte a + i pairs with global
// byte i, so a dword that is aligned in global memory is aligned in LDS too.  Whole aligned dwords inside the range move as dwords;
// the bytes in front of the first and behind the last one move as bytes (at most 3 each).  Nothing outside [0, len) is read or written.
__device__ inline void stage_in(unsigned char *lds, const unsigned char *src, uint32_t len, uint32_t a) {
    const uint32_t want = (4u - a) & 3u, head = len < want ? len : want, words = (len - head) / 4u, tail0 = head + 4u * words;
    const uint32_t *s4 = (const uint32_t *) (src + head);
    uint32_t *l4 = (uint32_t *) (lds + a + head);
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) l4[w] = s4[w];
    if (threadIdx.x < head) lds[a + threadIdx.x] = src[threadIdx.x];
    if (threadIdx.x >= 64u && threadIdx.x - 64u < len - tail0) lds[a + tail0 + threadIdx.x - 64u] = src[tail0 + threadIdx.x - 64u];
}
__device__ inline void stage_out(unsigned char *dst, const unsigned char *lds, uint32_t len, uint32_t a) {
    const uint32_t want = (4u - a) & 3u, head = len < want ? len : want, words = (len - head) / 4u, tail0 = head + 4u * words;
    uint32_t *d4 = (uint32_t *) (dst + head);
    const uint32_t *l4 = (const uint32_t *) (lds + a + head);
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) d4[w] = l4[w];
    if (threadIdx.x < head) dst[threadIdx.x] = lds[a + threadIdx.x];
    if (threadIdx.x >= 64u && threadIdx.x - 64u < len - tail0) dst[tail0 + threadIdx.x - 64u] = lds[a + tail0 + threadIdx.x - 64u];
}

// What both per-tile kernels start with: the tile's colour bytes staged into `in` (LDS; P3 only -- a pixel map's lengths do not depend on
// the colours, and its scatter stages them itself), then this thread's RTO_THREAD_PIXELS consecutive pixels: len[k], and (g, r, c) of the
// first.  Returns the thread's byte count.  Pixels behind the image's end have length 0.
template <int FMT, bool NEED_RGB>
__device__ inline uint32_t thread_lengths(const unsigned char *rgb, uint32_t npx, uint32_t cols, const uint32_t *tab, unsigned char *in, uint32_t &a_in,
                                          uint32_t len[RTO_THREAD_PIXELS], uint32_t &g0, uint32_t &r0, uint32_t &c0) {
    const uint32_t p0 = blockIdx.x * (uint32_t) RTO_TILE_PIXELS, cnt = npx - p0 < (uint32_t) RTO_TILE_PIXELS ? npx - p0 : (uint32_t) RTO_TILE_PIXELS;
    const unsigned char *src = rgb + (size_t) p0 * 3u;
    a_in = (uint32_t) ((uintptr_t) src & 3u);
    if (NEED_RGB) stage_in(in, src, cnt * 3u, a_in);
    __syncthreads(); // (the digit table too)
    g0 = p0 + threadIdx.x * (uint32_t) RTO_THREAD_PIXELS;
    r0 = g0 / cols; c0 = g0 - r0 * cols;
    uint32_t r = r0, c = c0, sum = 0;
    for (uint32_t k = 0; k < (uint32_t) RTO_THREAD_PIXELS; ++k) {
        const uint32_t g = g0 + k;
        len[k] = g < npx ? pixel_len<FMT>(tab, in + a_in + (g - p0) * 3u, g, r, c, npx - 1u) : 0u;
        sum += len[k];
        if (++c == cols) { c = 0; ++r; }
    }
    return sum;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------

template <int FMT> __global__ __launch_bounds__(RTO_BLOCK) void format_sums_kernel(const unsigned char *rgb, uint32_t npx, uint32_t cols, const GammaTable gamma,
                                                                                   unsigned long long *tiles) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t in[RTO_TILE_PIXELS * 3 / 4 + 1];
    __shared__ uint32_t wave_tot[RTO_BLOCK / 64];
    if (FMT == FMT_PPM) fill_digit_table(tab, gamma);
    uint32_t a_in, len[RTO_THREAD_PIXELS], g0, r0, c0, total;
    const uint32_t mine = thread_lengths<FMT, FMT == FMT_PPM>(rgb, npx, cols, tab, (unsigned char *) in, a_in, len, g0, r0, c0);
    (void) block_exclusive_scan<uint32_t, RTO_BLOCK>(mine, wave_tot, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// tiles[i]: the byte count of tile i on entry, the offset of its first byte on return (`first` = the bytes in front of tile 0, the P3
// header).  ONE workgroup; more tiles than it has threads are walked in trips, the running total in `carry` -- every thread keeps the
// same copy in a register.
__global__ __launch_bounds__(RTO_SCAN_THREADS) void format_scan_kernel(unsigned long long *tiles, uint32_t n_tiles, unsigned long long first, FormatScratch *head,
                                                                       long long *d_length, unsigned long long capacity, int have_out) {
    __shared__ unsigned long long wave_tot[RTO_SCAN_THREADS / 64];
    unsigned long long carry = first;
    for (uint32_t base = 0; base < n_tiles; base += (uint32_t) RTO_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < n_tiles ? tiles[i] : 0ull;
        unsigned long long trip;
        const unsigned long long before = block_exclusive_scan<unsigned long long, RTO_SCAN_THREADS>(v, wave_tot, trip);
        if (i < n_tiles) tiles[i] = carry + before;
        carry += trip;
    }
    if (threadIdx.x == 0) {
        head->total = (long long) carry;
        head->go = (have_out && carry <= capacity) ? 1u : 0u; // too small a buffer: not one byte of it is written
        if (d_length) *d_length = (long long) carry;
    }
}

// STAGED: the tile's range assembled in LDS, then aligned dword stores (the product).  Plain (-DRTO_PLAIN_STORES, measurements only): every
// thread stores its own bytes to global memory one at a time.
template <int FMT, bool STAGED>
__global__ __launch_bounds__(RTO_BLOCK) void format_scatter_kernel(const unsigned char *rgb, uint32_t npx, uint32_t cols, const GammaTable gamma, const PpmHeader hdr,
                                                                   const unsigned long long *tiles, const FormatScratch *head, unsigned char *out) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t in[RTO_TILE_PIXELS * 3 / 4 + 1];
    __shared__ uint32_t wave_tot[RTO_BLOCK / 64];
    __shared__ uint32_t text[STAGED ? RTO_TILE_PIXELS * Fmt<FMT>::MAX_BYTES / 4 + 1 : 1];
    if (!head->go) return; // the same word for every thread of every workgroup
    if (FMT == FMT_PPM) fill_digit_table(tab, gamma);
    uint32_t a_in, len[RTO_THREAD_PIXELS], g0, r0, c0, total;
    const uint32_t mine = thread_lengths<FMT, true>(rgb, npx, cols, tab, (unsigned char *) in, a_in, len, g0, r0, c0);
    uint32_t at = block_exclusive_scan<uint32_t, RTO_BLOCK>(mine, wave_tot, total);
    unsigned char *dst = out + tiles[blockIdx.x];
    const uint32_t a_out = (uint32_t) ((uintptr_t) dst & 3u);
    unsigned char *to = STAGED ? (unsigned char *) text + a_out : dst;
    const uint32_t p0 = blockIdx.x * (uint32_t) RTO_TILE_PIXELS;
    uint32_t r = r0, c = c0;
    for (uint32_t k = 0; k < (uint32_t) RTO_THREAD_PIXELS; ++k) {
        const uint32_t g = g0 + k;
        if (g < npx) at += put_pixel<FMT>(to + at, tab, (const unsigned char *) in + a_in + (g - p0) * 3u, g, r, c, npx - 1u, cols);
        if (++c == cols) { c = 0; ++r; }
    }
    if (STAGED) {
        __syncthreads();
        stage_out(dst, (const unsigned char *) text, total, a_out);
    }
    if (FMT == FMT_PPM && blockIdx.x == 0 && threadIdx.x < hdr.len) out[threadIdx.x] = hdr.text[threadIdx.x];
}

// PixelOutput.correct over n bytes; out may be in (every byte is read and written by the same thread).  Dwords when both buffers
// are misaligned alike, bytes otherwise.
__global__ __launch_bounds__(RTO_BLOCK) void gamma_kernel(const unsigned char *in, unsigned char *out, unsigned long long n, const GammaTable gamma) {
    __shared__ unsigned char lut[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) lut[i] = gamma.v[i];
    __syncthreads();
    const unsigned long long tid = (unsigned long long) blockIdx.x * blockDim.x + threadIdx.x, step = (unsigned long long) gridDim.x * blockDim.x;
    const uint32_t a = (uint32_t) ((uintptr_t) in & 3u);
    if (a != (uint32_t) ((uintptr_t) out & 3u)) {
        for (unsigned long long i = tid; i < n; i += step) out[i] = lut[in[i]];
        return;
    }
    const unsigned long long want = (4u - a) & 3u, head = n < want ? n : want, words = (n - head) / 4ull, tail0 = head + 4ull * words;
    const uint32_t *s4 = (const uint32_t *) (in + head);
    uint32_t *d4 = (uint32_t *) (out + head);
    for (unsigned long long w = tid; w < words; w += step) {
        const uint32_t x = s4[w];
        d4[w] = (uint32_t) lut[x & 255u] | ((uint32_t) lut[(x >> 8) & 255u] << 8) | ((uint32_t) lut[(x >> 16) & 255u] << 16) | ((uint32_t) lut[x >> 24] << 24);
    }
    if (tid < head) out[tid] = lut[in[tid]];
    if (tid >= 64ull && tid - 64ull < n - tail0) out[tail0 + tid - 64ull] = lut[in[tail0 + tid - 64ull]];
}

} // namespace rto
