// rt_png_kernels.h -- Png.write (ImageOutput.fs:214-251) on the device: the file rt_png.h defines, from an image that is already there.
// The host formatter rtp::format_png is what every byte is held to; everything serial or table-like is rt_png.h's and is only CALLED here.
// DESIGN.md "PNG on the device".
//
// A tile is RTO_PNG_TILE_BYTES of the filtered stream and one byte-aligned deflate block, so where a tile's bytes go is a prefix sum over
// tile sizes -- the P3 text's scheme (rt_output.h), and its scan kernel.  Four launches, every dependence a kernel boundary:
//   png_sums_kernel     one workgroup per tile: stage the source bytes (3 bytes of halo for the Sub filter), filter, find the runs, count the
//                       tokens' symbols in LDS, one thread builds the code lengths and chooses the block type (rtp::plan_tile): the tile's
//                       byte count.  Tile 0 also stores the length of what follows the last tile, as one more "tile" for the scan.
//   format_scan_kernel  (rt_output.h) offsets, the file's length, and whether the caller's buffer holds it
//   png_scatter_kernel  one workgroup per tile: the same plan again (cheaper than carrying 288 lengths per tile through memory), a prefix sum
//                       of the tokens' bit counts inside the tile, the bits OR-ed into zeroed LDS words with LDS atomics, stage_out; and
//                       while the bytes are in LDS the tile's CRC-32 and the Adler-32 of its filtered bytes
//   png_finish_kernel   ONE workgroup: the partial sums combined in order (rtp::crc_combine / adler_combine, as a tree), then the 43 bytes in
//                       front of the tiles and the 25 behind them
// Each thread owns RTO_PNG_TILE_BYTES / RTO_BLOCK = 64 consecutive filtered bytes.
// The per-tile and per-image work is in device functions (png_tile_plan, png_scatter_tile, png_finish_image) that take the image's first byte
// and the tile's index inside its image: the four kernels above run them for one image, the png_views_* kernels at the end of this file
// for the K equal-sized images of a batch, still in four launches.
#pragma once

#include "rt_output.h"
#include "rt_png.h"

namespace rto {

enum { FMT_PNG = 2 };
enum { PNG_THREAD_BYTES = RTO_PNG_TILE_BYTES / RTO_BLOCK, PNG_IO_WORDS = RTO_PNG_TILE_BYTES / 4 + 4, PNG_NONE = 0xFFFFFFFFu };
static_assert(RTO_PNG_TILE_BYTES % RTO_BLOCK == 0 && RTO_PNG_TILE_BYTES <= 65535, "a tile divides among the threads and fits a stored block");

struct PngPartial { uint32_t crc, adler; }; // of a tile's bytes / of its filtered bytes

struct PngLds {
    uint32_t io[PNG_IO_WORDS];           // the source bytes coming in (T + 3 and up to 3 of alignment), later the tile going out (T + 5 and up to 3)
    uint8_t f[RTO_PNG_TILE_BYTES];       // the filtered bytes
    uint32_t hist[rtp::LL_SYMS];
    uint32_t first_brk[RTO_BLOCK], last_brk[RTO_BLOCK]; // per thread: the first and last run start among its bytes; later the CRC tree
    uint32_t wave_tot[RTO_BLOCK / 64];
    uint32_t adler[2];
    uint8_t lut[256];
    rtp::BuildScratch build;
    rtp::TilePlan plan;
};

struct PngThread {
    uint32_t n;                 // the tile's filtered bytes
    uint32_t c0, c1;            // this thread's bytes [c0, c1) of them
    uint32_t in_start, out_end; // where the run that holds byte c0 - 1 starts; where the run that holds byte c1 - 1 ends
};

// fn(tok, byte) for every token that begins among the thread's bytes, in order.
template <class Fn> __device__ inline void png_walk_tokens(const uint8_t *f, const PngThread &th, Fn fn) {
    uint32_t rs = 0u, re = th.c0;
    for (uint32_t p = th.c0; p < th.c1; ++p) {
        if (p == re) { // a run begins here -- or, at c0, goes on
            rs = (p == 0u || f[p] != f[p - 1u]) ? p : th.in_start;
            uint32_t q = p + 1u;
            while (q < th.c1 && f[q] == f[q - 1u]) ++q;
            re = q < th.c1 ? q : th.out_end;
        }
        const uint32_t tok = rtp::token_at(p - rs, re - rs);
        if (tok) fn(tok, f[p]);
    }
}

// What both per-tile kernels start with: L.f, the thread's part of it, and L.plan.  rgb: the image's first byte; tile: the tile's index
// inside its image; N: the image's filtered stream's length.  No byte in front of rgb is read: the Sub filter's halo stops there.
__device__ inline PngThread png_tile_plan(PngLds &L, const unsigned char *rgb, uint32_t tile, uint32_t N, uint32_t cols, const GammaTable &gamma) {
    const uint32_t T = (uint32_t) RTO_PNG_TILE_BYTES, S = 1u + 3u * cols, i0 = tile * T;
    PngThread th;
    th.n = N - i0 < T ? N - i0 : T;
    // the source bytes of filtered bytes i0 .. i0 + n - 1: filtered byte (r, j >= 1) is source byte r (S - 1) + j - 1; three more in front
    const uint32_t r0 = i0 / S, j0 = i0 - r0 * S, i1 = i0 + th.n - 1u, r1 = i1 / S, j1 = i1 - r1 * S;
    const uint32_t s_first = r0 * (S - 1u) + (j0 ? j0 - 1u : 0u), s_lo = s_first >= 3u ? s_first - 3u : 0u, s_hi = r1 * (S - 1u) + j1;
    const unsigned char *src = rgb + s_lo;
    const uint32_t a_in = (uint32_t) ((uintptr_t) src & 3u);
    stage_in((unsigned char *) L.io, src, s_hi - s_lo, a_in);
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) L.lut[i] = gamma.v[i];
    for (uint32_t i = threadIdx.x; i < (uint32_t) rtp::LL_SYMS; i += blockDim.x) L.hist[i] = 0u;
    if (threadIdx.x < 2u) L.adler[threadIdx.x] = 0u;
    __syncthreads();
    th.c0 = threadIdx.x * (uint32_t) PNG_THREAD_BYTES < th.n ? threadIdx.x * (uint32_t) PNG_THREAD_BYTES : th.n;
    th.c1 = th.c0 + (uint32_t) PNG_THREAD_BYTES < th.n ? th.c0 + (uint32_t) PNG_THREAD_BYTES : th.n;
    {
        const unsigned char *in = (const unsigned char *) L.io + a_in;
        const uint32_t i = i0 + th.c0, r = i / S;
        uint32_t j = i - r * S, at = r * (S - 1u) + (j ? j - 1u : 0u) - s_lo; // the next colour byte, as an index into `in`
        for (uint32_t p = th.c0; p < th.c1; ++p) {
            if (j == 0u) L.f[p] = 1u;
            else { L.f[p] = rtp::filter_sub(L.lut[in[at]], j >= 4u ? L.lut[in[at - 3u]] : (uint8_t) 0); ++at; }
            if (++j == S) j = 0u;
        }
    }
    __syncthreads();
    uint32_t fb = (uint32_t) PNG_NONE, lb = (uint32_t) PNG_NONE;
    for (uint32_t p = th.c0; p < th.c1; ++p)
        if (p == 0u || L.f[p] != L.f[p - 1u]) { if (fb == (uint32_t) PNG_NONE) fb = p; lb = p; }
    L.first_brk[threadIdx.x] = fb; L.last_brk[threadIdx.x] = lb;
    __syncthreads();
    th.in_start = 0u; th.out_end = th.n;
    for (uint32_t t = threadIdx.x; t-- > 0u;)
        if (L.last_brk[t] != (uint32_t) PNG_NONE) { th.in_start = L.last_brk[t]; break; }
    for (uint32_t t = threadIdx.x + 1u; t < (uint32_t) RTO_BLOCK; ++t)
        if (L.first_brk[t] != (uint32_t) PNG_NONE) { th.out_end = L.first_brk[t]; break; }
    uint32_t *hist = L.hist;
    png_walk_tokens(L.f, th, [hist](uint32_t tok, uint8_t byte) {
        uint32_t sym = byte, ebits, eval;
        if (tok != 1u) rtp::length_symbol(tok, sym, ebits, eval);
        atomicAdd(&hist[sym], 1u);
    });
    if (threadIdx.x == 0u) L.hist[rtp::EOB] = 1u; // no token is the end-of-block symbol: nobody else touches this word
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < (uint32_t) rtp::LL_SYMS; s += blockDim.x)
        if (L.hist[s]) L.build.order[rtp::rank_of(L.hist, (uint32_t) rtp::LL_SYMS, s)] = (uint16_t) s;
    __syncthreads();
    if (threadIdx.x == 0u) { // the serial part: 286 + 19 code lengths; the other waves wait at the barrier
        uint32_t m = 0u;
        for (uint32_t s = 0u; s < (uint32_t) rtp::LL_SYMS; ++s) m += L.hist[s] ? 1u : 0u;
        rtp::plan_tile(L.hist, m, th.n, L.build, L.plan);
    }
    __syncthreads();
    return th;
}

// value's low nbits at bit `bit` of zeroed words; bits above nbits are zero
__device__ inline void png_or_bits(uint32_t *words, uint32_t bit, uint32_t value, uint32_t nbits) {
    if (!value || !nbits) return;
    const unsigned long long x = (unsigned long long) value << (bit & 31u);
    atomicOr(&words[bit >> 5], (uint32_t) x);
    if (x >> 32) atomicOr(&words[(bit >> 5) + 1u], (uint32_t) (x >> 32));
}

__global__ __launch_bounds__(RTO_BLOCK) void png_sums_kernel(const unsigned char *rgb, uint32_t N, uint32_t cols, const GammaTable gamma, unsigned long long *tiles,
                                                             uint32_t n_tiles) {
    __shared__ PngLds L;
    (void) png_tile_plan(L, rgb, blockIdx.x, N, cols, gamma);
    if (threadIdx.x == 0u) {
        tiles[blockIdx.x] = L.plan.bytes;
        if (blockIdx.x == 0u) tiles[n_tiles] = (unsigned long long) rtp::TAIL_BYTES;
    }
}

// One tile of one image written to dst, and its partial sums to *part: the scatter of a frame and of a batch (the whole workgroup calls it).
__device__ __forceinline__ void png_scatter_tile(PngLds &L, const unsigned char *rgb, uint32_t tile, uint32_t N, uint32_t cols, const GammaTable &gamma, unsigned char *dst,
                                        PngPartial *part) {
    const PngThread th = png_tile_plan(L, rgb, tile, N, cols, gamma);
    for (uint32_t w = threadIdx.x; w < (uint32_t) PNG_IO_WORDS; w += blockDim.x) L.io[w] = 0u; // (the source bytes are not needed again)
    __syncthreads();
    const uint32_t a_out = (uint32_t) ((uintptr_t) dst & 3u), bytes = L.plan.bytes;
    unsigned char *ob = (unsigned char *) L.io + a_out;
    if (L.plan.btype == (uint32_t) rtp::BT_STORED) {
        if (threadIdx.x == 0u) { ob[0] = 0u; ob[1] = (uint8_t) th.n; ob[2] = (uint8_t) (th.n >> 8); ob[3] = (uint8_t) ~th.n; ob[4] = (uint8_t) (~th.n >> 8); }
        for (uint32_t p = th.c0; p < th.c1; ++p) ob[(uint32_t) rtp::STORED_HEAD + p] = L.f[p];
    } else {
        const rtp::TilePlan &plan = L.plan;
        uint32_t *words = L.io;
        const uint32_t bit0 = 8u * a_out;
        uint32_t mine = 0u, total;
        png_walk_tokens(L.f, th, [&mine, &plan](uint32_t tok, uint8_t byte) { uint32_t v; mine += rtp::token_bits(plan, tok, byte, v); });
        const uint32_t before = block_exclusive_scan<uint32_t, RTO_BLOCK>(mine, L.wave_tot, total);
        const uint32_t eob_at = plan.body_bits - plan.ll_len[rtp::EOB];
        uint32_t at = bit0 + eob_at - total + before; // the header's bits end where the tokens' begin
        png_walk_tokens(L.f, th, [&at, words, &plan](uint32_t tok, uint8_t byte) {
            uint32_t v;
            const uint32_t nb = rtp::token_bits(plan, tok, byte, v);
            png_or_bits(words, at, v, nb);
            at += nb;
        });
        if (threadIdx.x == 0u) {
            (void) rtp::write_block_header(plan, [words, bit0](uint32_t pos, uint32_t v, uint32_t nb) { png_or_bits(words, bit0 + pos, v, nb); });
            png_or_bits(words, bit0 + eob_at, plan.ll_code[rtp::EOB], plan.ll_len[rtp::EOB]);
            png_or_bits(words, 8u * (a_out + bytes - 2u), 0xFFFFu, 16u); // 000, zeros to the byte boundary, 00 00 FF FF
        }
    }
    // Adler-32 of the filtered bytes: sums from zero per thread, then s2 carries s1 over the bytes behind the thread's
    {
        uint32_t s1 = 0u, s2 = 0u;
        for (uint32_t p = th.c0; p < th.c1; ++p) { s1 += L.f[p]; s2 += s1; }
        atomicAdd(&L.adler[0], s1);
        atomicAdd(&L.adler[1], (s2 + s1 * (th.n - th.c1)) % (uint32_t) rtp::ADLER_MOD);
    }
    __syncthreads();
    stage_out(dst, (const unsigned char *) L.io, bytes, a_out);
    // CRC-32 of the tile's bytes: a piece per thread, combined as a tree
    const uint32_t piece = (bytes + (uint32_t) RTO_BLOCK - 1u) / (uint32_t) RTO_BLOCK;
    const uint32_t b0 = threadIdx.x * piece < bytes ? threadIdx.x * piece : bytes, b1 = b0 + piece < bytes ? b0 + piece : bytes;
    uint32_t *pc = L.first_brk, *pl = L.last_brk;
    pc[threadIdx.x] = rtp::crc32_of(ob + b0, b1 - b0); pl[threadIdx.x] = b1 - b0;
    __syncthreads();
    for (uint32_t d = 1u; d < (uint32_t) RTO_BLOCK; d <<= 1) {
        if ((threadIdx.x & (2u * d - 1u)) == 0u) {
            pc[threadIdx.x] = rtp::crc_combine(pc[threadIdx.x], pc[threadIdx.x + d], pl[threadIdx.x + d]);
            pl[threadIdx.x] += pl[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
        const uint32_t M = (uint32_t) rtp::ADLER_MOD;
        part->crc = pc[0];
        part->adler = (((th.n + L.adler[1]) % M) << 16) | ((1u + L.adler[0]) % M);
    }
}

__global__ __launch_bounds__(RTO_BLOCK) void png_scatter_kernel(const unsigned char *rgb, uint32_t N, uint32_t cols, const GammaTable gamma,
                                                                const unsigned long long *tiles, const FormatScratch *head, PngPartial *parts, unsigned char *out) {
    __shared__ PngLds L;
    if (!head->go) return; // the same word for every thread of every workgroup
    png_scatter_tile(L, rgb, blockIdx.x, N, cols, gamma, out + tiles[blockIdx.x], parts + blockIdx.x);
}

struct PngFinishLds {
    uint32_t pc[RTO_BLOCK], pa[RTO_BLOCK];
    unsigned long long plen[RTO_BLOCK], pun[RTO_BLOCK];
};

// (Force-inlined, as png_scatter_tile is: left as a call it takes the calling convention's registers and a scratch frame.)
// One image's file finished by one workgroup: its tiles' partial sums combined in order, then the 43 bytes at `file` and the 25 behind its
// last tile.  tiles[0 .. n_tiles]: the offsets, in `out`, of the image's tiles and of its tail; idat: the IDAT chunk's length.
__device__ __forceinline__ void png_finish_image(PngFinishLds &F, uint32_t rows, uint32_t cols, uint32_t N, const unsigned long long *tiles, uint32_t n_tiles, uint32_t idat,
                                        const PngPartial *parts, unsigned char *file, unsigned char *out) {
    const uint32_t per = (n_tiles + (uint32_t) RTO_BLOCK - 1u) / (uint32_t) RTO_BLOCK;
    const uint32_t t0 = threadIdx.x * per < n_tiles ? threadIdx.x * per : n_tiles, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    uint32_t crc = 0u, adler = 1u;
    unsigned long long len = 0ull, un = 0ull;
    for (uint32_t t = t0; t < t1; ++t) {
        const unsigned long long bytes = tiles[t + 1u] - tiles[t];
        const uint32_t i0 = t * (uint32_t) RTO_PNG_TILE_BYTES, n = N - i0 < (uint32_t) RTO_PNG_TILE_BYTES ? N - i0 : (uint32_t) RTO_PNG_TILE_BYTES;
        crc = rtp::crc_combine(crc, parts[t].crc, bytes); len += bytes;
        adler = rtp::adler_combine(adler, parts[t].adler, n); un += n;
    }
    F.pc[threadIdx.x] = crc; F.pa[threadIdx.x] = adler; F.plen[threadIdx.x] = len; F.pun[threadIdx.x] = un;
    __syncthreads();
    for (uint32_t d = 1u; d < (uint32_t) RTO_BLOCK; d <<= 1) {
        if ((threadIdx.x & (2u * d - 1u)) == 0u) {
            F.pc[threadIdx.x] = rtp::crc_combine(F.pc[threadIdx.x], F.pc[threadIdx.x + d], F.plen[threadIdx.x + d]); F.plen[threadIdx.x] += F.plen[threadIdx.x + d];
            F.pa[threadIdx.x] = rtp::adler_combine(F.pa[threadIdx.x], F.pa[threadIdx.x + d], F.pun[threadIdx.x + d]); F.pun[threadIdx.x] += F.pun[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
        rtp::write_head(rows, cols, idat, [file](uint32_t i, uint8_t b) { file[i] = b; });
        unsigned char *tail = out + tiles[n_tiles];
        rtp::write_tail(F.pa[0], rtp::crc_combine(rtp::idat_crc_start(), F.pc[0], F.plen[0]), [tail](uint32_t i, uint8_t b) { tail[i] = b; });
    }
}

// tiles[0 .. n_tiles]: the offsets of the tiles and of the file's tail.
__global__ __launch_bounds__(RTO_BLOCK) void png_finish_kernel(uint32_t rows, uint32_t cols, uint32_t N, const unsigned long long *tiles, uint32_t n_tiles,
                                                               const FormatScratch *head, const PngPartial *parts, unsigned char *out) {
    __shared__ PngFinishLds F;
    if (!head->go) return;
    const uint32_t idat = (uint32_t) ((unsigned long long) head->total - (unsigned long long) rtp::HEAD_BYTES - (unsigned long long) rtp::TAIL_BYTES +
                                      (unsigned long long) rtp::IDAT_EXTRA);
    png_finish_image(F, rows, cols, N, tiles, n_tiles, idat, parts, out, out);
}

// ---- a batch of equal-sized images (rt_png.h "a batch of equal-sized images"; DESIGN.md "PNG files of a batch of views") -------------------
// Image v is the image_bytes bytes at rgb + v * image_bytes, its file what the kernels above write for it alone; the K files stand behind one
// another in `out`.  The same four launches whatever K is: workgroup b of the per-tile kernels serves image b / tiles, tile b % tiles, the
// scan runs over every image's entries at once, and the finish step is one workgroup per image.  `entries` is the batch's scan array
// (rtp::views_entry), `offsets` its K + 1 file starts.
struct PngViews {
    const unsigned char *rgb;
    unsigned long long image_bytes; // rows * cols * 3
    uint32_t n_views, tiles;        // tiles per image
    uint32_t rows, cols, N;         // N: an image's filtered bytes
};

__global__ __launch_bounds__(RTO_BLOCK) void png_views_sums_kernel(const PngViews b, const GammaTable gamma, unsigned long long *entries) {
    __shared__ PngLds L;
    const uint32_t v = blockIdx.x / b.tiles, t = blockIdx.x - v * b.tiles;
    (void) png_tile_plan(L, b.rgb + (unsigned long long) v * b.image_bytes, t, b.N, b.cols, gamma);
    if (threadIdx.x == 0u) {
        entries[rtp::views_entry(v, t, b.tiles)] = L.plan.bytes;
        if (t == 0u) entries[rtp::views_entry(v, b.tiles, b.tiles)] = rtp::views_tail_entry_bytes(v, b.n_views);
    }
}

// format_scan_kernel over the batch's entries (64-bit counts: 2 K entries of 1 x 1 images may pass 2^32), which also leaves the K + 1 file
// starts: in `offsets` (the call's scratch, for the finish step and the host) and in d_offsets when the caller gave it.
__global__ __launch_bounds__(RTO_SCAN_THREADS) void png_views_scan_kernel(unsigned long long *entries, const PngViews b, FormatScratch *head, long long *offsets,
                                                                          long long *d_offsets, unsigned long long capacity, int have_out) {
    __shared__ unsigned long long wave_tot[RTO_SCAN_THREADS / 64];
    const unsigned long long n = rtp::views_entry_count(b.n_views, b.tiles), per = rtp::views_image_entries(b.tiles);
    unsigned long long carry = rtp::views_first_bytes();
    for (unsigned long long base = 0ull; base < n; base += (unsigned long long) RTO_SCAN_THREADS) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long c = i < n ? entries[i] : 0ull;
        unsigned long long trip;
        const unsigned long long before = block_exclusive_scan<unsigned long long, RTO_SCAN_THREADS>(c, wave_tot, trip);
        if (i < n) {
            entries[i] = carry + before;
            const unsigned long long v = i / per;
            if (i == rtp::views_entry(v, 0u, b.tiles)) { // an image's first tile: its file starts HEAD_BYTES in front
                const long long start = (long long) rtp::views_file_start(entries, v, b.tiles);
                offsets[v] = start;
                if (d_offsets) d_offsets[v] = start;
            }
        }
        carry += trip;
    }
    if (threadIdx.x == 0) {
        head->total = (long long) carry;
        head->go = rtp::views_go(carry, capacity, have_out != 0) ? 1u : 0u; // too small a buffer: not one byte of it is written
        offsets[b.n_views] = (long long) carry;
        if (d_offsets) d_offsets[b.n_views] = (long long) carry;
    }
}

__global__ __launch_bounds__(RTO_BLOCK) void png_views_scatter_kernel(const PngViews b, const GammaTable gamma, const unsigned long long *entries, const FormatScratch *head,
                                                                      PngPartial *parts, unsigned char *out) {
    __shared__ PngLds L;
    if (!head->go) return; // the same word for every thread of every workgroup
    const uint32_t v = blockIdx.x / b.tiles, t = blockIdx.x - v * b.tiles;
    png_scatter_tile(L, b.rgb + (unsigned long long) v * b.image_bytes, t, b.N, b.cols, gamma, out + entries[rtp::views_entry(v, t, b.tiles)], parts + blockIdx.x);
}

// One workgroup per image.  parts: one PngPartial per tile, image by image.
__global__ __launch_bounds__(RTO_BLOCK) void png_views_finish_kernel(const PngViews b, const unsigned long long *entries, const FormatScratch *head, const PngPartial *parts,
                                                                     unsigned char *out) {
    __shared__ PngFinishLds F;
    if (!head->go) return;
    const uint32_t v = blockIdx.x;
    png_finish_image(F, b.rows, b.cols, b.N, entries + rtp::views_entry(v, 0u, b.tiles), b.tiles, rtp::views_idat_length(entries, v, b.tiles, (uint64_t) head->total),
                     parts + (unsigned long long) v * b.tiles, out + rtp::views_file_start(entries, v, b.tiles), out);
}

} // namespace rto
