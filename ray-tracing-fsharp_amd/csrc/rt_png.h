// rt_png.h -- the PNG this library writes, defined ONCE: Png.write (ImageOutput.fs:214-251) hands PixelOutput.toSkia colours
// (ImageOutput.fs:32-39) to Skia's encoder, whose bytes nobody can reproduce; PNG is lossless, so the PIXELS are pinned (R, G, B after
// PixelOutput.correct or as they are, alpha 255) and the container bytes are defined here.  Plain C++ over plain integers: the host
// formatter (rtp::format_png below) and the kernels (rt_png_kernels.h) inline the same functions, and tests/c/png_host_table.cpp drives
// them on a CPU.  DESIGN.md "PNG on the device".
//
//   file     signature, IHDR (cols, rows, 8, 2, 0, 0, 0), ONE IDAT, IEND
//   IDAT     zlib header 78 01, the tiles, a final empty stored block (01 00 00 FF FF), Adler-32 of the filtered stream
//   filter   every row is type 1 (Sub): the byte 1, then x[j] - x[j-3] mod 256 over the gamma-mapped bytes (x[j-3] = 0 in the first pixel)
//   tile     RTO_PNG_TILE_BYTES of the filtered stream (the last one shorter) as ONE deflate block that ends on a byte boundary: a stored
//            block, or a fixed / dynamic Huffman block with an empty stored block (000, padding, 00 00 FF FF) behind it.  A tile owns a
//            whole byte range, and no match reaches back across a tile's start.
//   tokens   run-length only: a run of equal bytes inside a tile is its first byte as a literal, then matches of at most 258 at
//            distance 1 cut greedily; a remainder below 3 goes out as literals.  token_at is a pure function of (position in run, run length).
//   block    the smallest of dynamic, fixed and stored, in that order on ties; the sizes are known before a bit is written.
#pragma once
#include "rt_launch_consts.h"

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTP_HD __host__ __device__ inline
#else
#define RTP_HD static inline
#endif

namespace rtp {

enum { LL_SYMS = 288, LL_USED = 286, EOB = 256, CL_SYMS = 19, LL_MAX_BITS = 15, CL_MAX_BITS = 7, MIN_MATCH = 3, MAX_MATCH = 258 };
enum { BT_STORED = 0, BT_FIXED = 1, BT_DYNAMIC = 2 };
enum {
    HEAD_BYTES = 43,  // signature 8, IHDR chunk 25, IDAT length and name 8, zlib header 2
    TAIL_BYTES = 25,  // final block 5, Adler-32 4, IDAT's CRC 4, IEND chunk 12
    STORED_HEAD = 5,  // 00, LEN, NLEN
    SYNC_BYTES = 4,   // 00 00 FF FF behind the three header bits and the padding
    IDAT_EXTRA = 11   // bytes of the IDAT data that are not tiles: zlib header 2, final block 5, Adler-32 4
};

// ---- sizes ----
RTP_HD uint64_t filtered_bytes(uint64_t rows, uint64_t cols) { return rows * (1u + 3u * cols); }
RTP_HD uint64_t tile_count(uint64_t rows, uint64_t cols) { return (filtered_bytes(rows, cols) + (uint64_t) RTO_PNG_TILE_BYTES - 1u) / (uint64_t) RTO_PNG_TILE_BYTES; }
// the file of an image whose every tile is stored: no output is longer
RTP_HD uint64_t max_bytes(uint64_t rows, uint64_t cols) {
    return (uint64_t) HEAD_BYTES + filtered_bytes(rows, cols) + (uint64_t) STORED_HEAD * tile_count(rows, cols) + (uint64_t) TAIL_BYTES;
}
// a chunk's length is a 31-bit number (PNG 5.3): the worst-case IDAT must fit
RTP_HD bool supported(uint64_t rows, uint64_t cols) { return max_bytes(rows, cols) - HEAD_BYTES - TAIL_BYTES + IDAT_EXTRA <= 0x7fffffffull; }

// ---- filter ----
RTP_HD uint8_t filter_sub(uint8_t x, uint8_t left) { return (uint8_t) (x - left); }

// ---- tokens ----
// Byte k (from 0) of a run of L equal bytes: 0 = covered by a match that began earlier, 1 = a literal, 3..258 = a match of that length begins here.
RTP_HD uint32_t token_at(uint32_t k, uint32_t L) {
    if (k == 0u) return 1u;
    const uint32_t j = k - 1u, rest = L - 1u, full = rest / (uint32_t) MAX_MATCH * (uint32_t) MAX_MATCH, rem = rest - full;
    if (j < full) return j % (uint32_t) MAX_MATCH == 0u ? (uint32_t) MAX_MATCH : 0u;
    if (rem < (uint32_t) MIN_MATCH) return 1u;
    return j == full ? rem : 0u;
}
// RFC 1951 3.2.5: a match length's symbol, the count of its extra bits and their value
RTP_HD void length_symbol(uint32_t len, uint32_t &sym, uint32_t &ebits, uint32_t &eval) {
    const uint32_t x = len - 3u;
    if (x < 8u) { sym = 257u + x; ebits = 0u; eval = 0u; return; }
    if (x == 255u) { sym = 285u; ebits = 0u; eval = 0u; return; }
    const uint32_t e = 1u + (x >= 16u) + (x >= 32u) + (x >= 64u) + (x >= 128u);
    sym = 261u + 4u * e + ((x >> e) & 3u); ebits = e; eval = x & ((1u << e) - 1u);
}
RTP_HD uint32_t length_extra_bits(uint32_t sym) { return (sym < 265u || sym >= 285u) ? 0u : (sym - 261u) / 4u; }
RTP_HD uint32_t fixed_length(uint32_t sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; } // RFC 1951 3.2.6
enum { FIXED_DIST_BITS = 5 };

// ---- checksums ----
RTP_HD uint32_t crc_byte(uint32_t reg, uint8_t b) { // the register of CRC-32 (reflected, 0xEDB88320) after one more byte; crc = ~reg, reg starts at ~0
    reg ^= b;
    for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (0xEDB88320u & (0u - (reg & 1u)));
    return reg;
}
RTP_HD uint32_t crc32_of(const uint8_t *p, uint64_t n, uint32_t crc = 0u) {
    uint32_t reg = ~crc;
    for (uint64_t i = 0; i < n; ++i) reg = crc_byte(reg, p[i]);
    return ~reg;
}
RTP_HD uint32_t gf2_mul(uint32_t a, uint32_t b) { // a * b mod P over GF(2), bit 31 = x^0
    uint32_t p = 0u;
    for (uint32_t m = 0x80000000u; m != 0u; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
RTP_HD uint32_t gf2_x_pow_8n(uint64_t n) { // x^(8n) mod P
    uint32_t p = 0x80000000u, sq = 0x00800000u; // x^0, x^8
    for (; n != 0u; n >>= 1) {
        if (n & 1u) p = gf2_mul(p, sq);
        sq = gf2_mul(sq, sq);
    }
    return p;
}
// crc32(A || B) from crc32(A), crc32(B) and B's length: the conditioning of both ends cancels
RTP_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return gf2_mul(gf2_x_pow_8n(len_b), crc_a) ^ crc_b; }

enum { ADLER_MOD = 65521 };
RTP_HD uint32_t adler32_of(const uint8_t *p, uint64_t n, uint32_t adler = 1u) {
    uint32_t a = adler & 0xffffu, b = adler >> 16;
    for (uint64_t i = 0; i < n; ++i) { a = (a + p[i]) % (uint32_t) ADLER_MOD; b = (b + a) % (uint32_t) ADLER_MOD; }
    return (b << 16) | a;
}
// adler32(A || B) from adler32(A), adler32(B) and B's length: B's sums began at a = 1 instead of A's a, len_b times over
RTP_HD uint32_t adler_combine(uint32_t ad_a, uint32_t ad_b, uint64_t len_b) {
    const uint64_t M = (uint64_t) ADLER_MOD, a1 = ad_a & 0xffffu, b1 = ad_a >> 16, a2 = ad_b & 0xffffu, b2 = ad_b >> 16;
    const uint64_t a = (a1 + a2 + M - 1u) % M, b = (b1 + b2 + (len_b % M) * ((a1 + M - 1u) % M)) % M;
    return (uint32_t) ((b << 16) | a);
}

// ---- Huffman code lengths ----
// The symbols in use come sorted by (count, symbol): rank_of is the position of one of them -- 256 threads each take a symbol, the host loops.
template <class Freq> RTP_HD uint32_t rank_of(Freq freq, uint32_t n, uint32_t s) {
    const uint32_t f = (uint32_t) freq[s];
    uint32_t r = 0u;
    for (uint32_t t = 0u; t < n; ++t) {
        const uint32_t g = (uint32_t) freq[t];
        r += (g != 0u && (g < f || (g == f && t < s))) ? 1u : 0u;
    }
    return r;
}

struct BuildScratch {
    uint16_t order[LL_SYMS];       // the symbols in use, by rising (count, symbol)
    uint32_t weight[2 * LL_SYMS];  // leaves 0 .. m-1 in that order, then the merged nodes in the order they are made
    uint16_t parent[2 * LL_SYMS];
    uint16_t depth[2 * LL_SYMS];
};

// Code lengths of at most max_bits for the m >= 0 symbols of s.order (counts in freq), 0 for every other symbol of 0 .. n-1.
//   m == 1: that symbol and one other get length 1 -- zlib's inflate refuses an incomplete code-length code; this encoder never gets there
//           (a tile has a literal and the end-of-block symbol; a header has at least two distinct lengths).
//   tree:   two queues -- the sorted leaves and the merged nodes, which are made in rising order of weight -- so every merge takes the
//           two smallest fronts; a parent's index is above its children's, so one downward sweep gives the depths.
//   limit:  leaves deeper than max_bits are counted at max_bits; the Kraft sum, in units of 2^-max_bits, then exceeds 2^max_bits by
//           `excess`.  zlib's repair step -- move the deepest leaf above max_bits one level down and make a max_bits leaf its brother
//           (count[b]--, count[b+1] += 2, count[max_bits]--) -- lowers the sum by exactly one unit, so `excess` steps make the code
//           complete.  A step is always possible: the Kraft sum Q of the leaves above max_bits starts below 1 (deeper leaves exist) and
//           no step raises it, so with excess > 0 some leaf sits AT max_bits; and were all m <= 2^max_bits leaves there, excess were <= 0.
//   assign: the counts per length go to the leaves from the rarest on, longest first -- as good as the tree's own placement.
template <class Freq, class Len> RTP_HD void build_lengths(Freq freq, uint32_t n, uint32_t m, uint32_t max_bits, BuildScratch &s, Len len) {
    for (uint32_t i = 0u; i < n; ++i) len[i] = 0;
    if (m == 0u) return;
    if (m == 1u) { len[s.order[0]] = 1; len[s.order[0] == 0u ? 1u : 0u] = 1; return; }
    for (uint32_t i = 0u; i < m; ++i) s.weight[i] = (uint32_t) freq[s.order[i]];
    uint32_t leaf = 0u, node = m, made = m;
    for (; made < 2u * m - 1u; ++made) {
        uint32_t w = 0u;
        for (int k = 0; k < 2; ++k) {
            const bool take_leaf = leaf < m && (node >= made || s.weight[leaf] <= s.weight[node]);
            const uint32_t pick = take_leaf ? leaf++ : node++;
            w += s.weight[pick];
            s.parent[pick] = (uint16_t) made;
        }
        s.weight[made] = w;
    }
    uint32_t count[LL_MAX_BITS + 1];
    for (uint32_t b = 0u; b <= max_bits; ++b) count[b] = 0u;
    s.depth[2u * m - 2u] = 0u;
    for (uint32_t i = 2u * m - 2u; i-- > 0u;) {
        const uint32_t d = (uint32_t) s.depth[s.parent[i]] + 1u;
        s.depth[i] = (uint16_t) d;
        if (i < m) count[d < max_bits ? d : max_bits]++;
    }
    uint32_t units = 0u;
    for (uint32_t b = 1u; b <= max_bits; ++b) units += count[b] << (max_bits - b);
    for (uint32_t excess = units > (1u << max_bits) ? units - (1u << max_bits) : 0u; excess > 0u; --excess) {
        uint32_t b = max_bits - 1u;
        while (count[b] == 0u) --b;
        count[b]--; count[b + 1u] += 2u; count[max_bits]--;
    }
    uint32_t i = 0u;
    for (uint32_t b = max_bits; b >= 1u; --b)
        for (uint32_t c = count[b]; c > 0u; --c) len[s.order[i++]] = (uint8_t) b;
}

// Canonical codes (RFC 1951 3.2.2) of n symbols, stored with their bits reversed: deflate packs a Huffman code from its most significant bit.
template <class Len, class Code> RTP_HD void assign_codes(Len len, uint32_t n, uint32_t max_bits, Code code) {
    uint32_t next[LL_MAX_BITS + 2];
    for (uint32_t b = 0u; b <= max_bits + 1u; ++b) next[b] = 0u;
    for (uint32_t i = 0u; i < n; ++i) next[(uint32_t) len[i] + 1u]++;
    next[1] = 0u; // length 0: no code
    for (uint32_t b = 2u; b <= max_bits; ++b) next[b] = (next[b] + next[b - 1u]) << 1; // next[b]: first code of length b
    for (uint32_t i = 0u; i < n; ++i) {
        const uint32_t l = (uint32_t) len[i];
        uint32_t c = l ? next[l]++ : 0u, r = 0u;
        for (uint32_t k = 0u; k < l; ++k) { r = (r << 1) | (c & 1u); c >>= 1; }
        code[i] = r;
    }
}

// ---- a tile's plan: everything known before a bit is written ----
struct TilePlan {
    uint32_t btype;      // BT_*
    uint32_t bytes;      // of the whole tile, sync marker included
    uint32_t body_bits;  // Huffman blocks: header and tokens and end-of-block, in front of the marker
    uint32_t hlit, hclen, n_cl, dist_len;
    uint8_t ll_len[LL_SYMS];    // of the chosen block type
    uint16_t ll_code[LL_SYMS];
    uint8_t cl_len[CL_SYMS];
    uint8_t cl_code[CL_SYMS];
    uint16_t cl_tok[LL_SYMS];   // the dynamic header's code-length symbols: symbol | extra value << 8
};
RTP_HD uint32_t cl_order(uint32_t i) { // RFC 1951 3.2.7
    const uint8_t o[CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}
RTP_HD uint32_t cl_extra_bits(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
RTP_HD uint32_t huffman_tile_bytes(uint32_t body_bits) { return (body_bits + 3u + 7u) / 8u + (uint32_t) SYNC_BYTES; }

// Symbols 16 / 17 / 18 over the HLIT + 1 lengths: a run of zeros as 18s of at most 138 while 11 or more remain, then one 17 for 3..10, else
// zeros; a run of another length as itself once, then 16s of at most 6 while 3 or more remain, then itself.
template <class Seq> RTP_HD uint32_t code_length_tokens(Seq seq, uint32_t n, uint16_t *tok) {
    uint32_t out = 0u;
    for (uint32_t i = 0u; i < n;) {
        const uint32_t v = (uint32_t) seq(i);
        uint32_t run = 1u;
        while (i + run < n && (uint32_t) seq(i + run) == v) ++run;
        i += run;
        if (v == 0u) {
            for (; run >= 11u;) { const uint32_t c = run < 138u ? run : 138u; tok[out++] = (uint16_t) (18u | ((c - 11u) << 8)); run -= c; }
            if (run >= 3u) { tok[out++] = (uint16_t) (17u | ((run - 3u) << 8)); run = 0u; }
        } else {
            tok[out++] = (uint16_t) v; --run;
            for (; run >= 3u;) { const uint32_t c = run < 6u ? run : 6u; tok[out++] = (uint16_t) (16u | ((c - 3u) << 8)); run -= c; }
        }
        for (; run > 0u; --run) tok[out++] = (uint16_t) v;
    }
    return out;
}

// The serial part of a tile.  hist: the tile's literal/length counts with hist[EOB] = 1 already in; s.order: its symbols in use, sorted
// (rank_of), m of them; n: the tile's filtered bytes.
template <class Hist> RTP_HD void plan_tile(Hist hist, uint32_t m, uint32_t n, BuildScratch &s, TilePlan &p) {
    build_lengths(hist, (uint32_t) LL_SYMS, m, (uint32_t) LL_MAX_BITS, s, p.ll_len);
    uint32_t matches = 0u, dyn = 0u, fixed = 3u;
    for (uint32_t i = 0u; i < (uint32_t) LL_USED; ++i) {
        const uint32_t h = (uint32_t) hist[i], e = i > (uint32_t) EOB ? length_extra_bits(i) : 0u;
        if (i > (uint32_t) EOB) matches += h;
        dyn += h * ((uint32_t) p.ll_len[i] + e);
        fixed += h * (fixed_length(i) + e);
    }
    p.dist_len = matches ? 1u : 0u; // ONE distance code (distance 1): a code of length 1; a tile without a match: HDIST = 1 with length 0
    dyn += matches * p.dist_len;
    fixed += matches * (uint32_t) FIXED_DIST_BITS;
    p.hlit = (uint32_t) LL_USED;
    while (p.hlit > 257u && p.ll_len[p.hlit - 1u] == 0u) --p.hlit;
    const uint8_t *ll = p.ll_len;
    const uint32_t hlit = p.hlit, dist_len = p.dist_len;
    p.n_cl = code_length_tokens([ll, hlit, dist_len](uint32_t i) { return i < hlit ? (uint32_t) ll[i] : dist_len; }, hlit + 1u, p.cl_tok);
    uint32_t cl_freq[CL_SYMS];
    for (uint32_t i = 0u; i < (uint32_t) CL_SYMS; ++i) cl_freq[i] = 0u;
    for (uint32_t i = 0u; i < p.n_cl; ++i) cl_freq[p.cl_tok[i] & 255u]++;
    uint32_t cm = 0u;
    for (uint32_t i = 0u; i < (uint32_t) CL_SYMS; ++i)
        if (cl_freq[i]) { s.order[rank_of(cl_freq, (uint32_t) CL_SYMS, i)] = (uint16_t) i; ++cm; }
    build_lengths(cl_freq, (uint32_t) CL_SYMS, cm, (uint32_t) CL_MAX_BITS, s, p.cl_len);
    assign_codes(p.cl_len, (uint32_t) CL_SYMS, (uint32_t) CL_MAX_BITS, p.cl_code);
    p.hclen = (uint32_t) CL_SYMS;
    while (p.hclen > 4u && p.cl_len[cl_order(p.hclen - 1u)] == 0u) --p.hclen;
    uint32_t head = 3u + 5u + 5u + 4u + 3u * p.hclen;
    for (uint32_t i = 0u; i < p.n_cl; ++i) head += (uint32_t) p.cl_len[p.cl_tok[i] & 255u] + cl_extra_bits(p.cl_tok[i] & 255u);
    const uint32_t dyn_bytes = huffman_tile_bytes(head + dyn), fixed_bytes = huffman_tile_bytes(fixed), stored_bytes = (uint32_t) STORED_HEAD + n;
    if (dyn_bytes <= fixed_bytes && dyn_bytes <= stored_bytes) {
        p.btype = BT_DYNAMIC; p.bytes = dyn_bytes; p.body_bits = head + dyn;
    } else if (fixed_bytes <= stored_bytes) {
        p.btype = BT_FIXED; p.bytes = fixed_bytes; p.body_bits = fixed; p.dist_len = (uint32_t) FIXED_DIST_BITS;
        for (uint32_t i = 0u; i < (uint32_t) LL_SYMS; ++i) p.ll_len[i] = (uint8_t) fixed_length(i);
    } else {
        p.btype = BT_STORED; p.bytes = stored_bytes; p.body_bits = 0u;
    }
    if (p.btype != BT_STORED) assign_codes(p.ll_len, (uint32_t) LL_SYMS, (uint32_t) LL_MAX_BITS, p.ll_code);
}

// A Huffman block's header through put(bit position, value, bit count) -- at most 16 bits a call; returns the bit position behind it.
template <class Put> RTP_HD uint32_t write_block_header(const TilePlan &p, Put put) {
    put(0u, (uint32_t) p.btype << 1, 3u); // BFINAL = 0
    uint32_t at = 3u;
    if (p.btype != BT_DYNAMIC) return at;
    put(at, p.hlit - 257u, 5u); at += 5u;
    put(at, 0u, 5u); at += 5u; // HDIST = 1
    put(at, p.hclen - 4u, 4u); at += 4u;
    for (uint32_t i = 0u; i < p.hclen; ++i) { put(at, (uint32_t) p.cl_len[cl_order(i)], 3u); at += 3u; }
    for (uint32_t i = 0u; i < p.n_cl; ++i) {
        const uint32_t sym = p.cl_tok[i] & 255u, l = p.cl_len[sym], e = cl_extra_bits(sym);
        put(at, (uint32_t) p.cl_code[sym] | ((uint32_t) (p.cl_tok[i] >> 8) << l), l + e);
        at += l + e;
    }
    return at;
}
// One token's bits (a literal, or a match of `tok` bytes at distance 1 -- distance code 0 under both block types) and their count.
RTP_HD uint32_t token_bits(const TilePlan &p, uint32_t tok, uint8_t byte, uint32_t &value) {
    if (tok == 1u) { value = p.ll_code[byte]; return p.ll_len[byte]; }
    uint32_t sym, ebits, eval;
    length_symbol(tok, sym, ebits, eval);
    value = (uint32_t) p.ll_code[sym] | (eval << p.ll_len[sym]);
    return (uint32_t) p.ll_len[sym] + ebits + p.dist_len;
}

// The file's first HEAD_BYTES and last TAIL_BYTES through put(index, byte).  idat_crc: crc32 of "IDAT" and the chunk's data.
template <class Put> RTP_HD void write_head(uint32_t rows, uint32_t cols, uint32_t idat_len, Put put) {
    const uint8_t sig[12] = {137, 80, 78, 71, 13, 10, 26, 10, 0, 0, 0, 13};
    uint8_t ihdr[17] = {'I', 'H', 'D', 'R', 0, 0, 0, 0, 0, 0, 0, 0, 8, 2, 0, 0, 0};
    for (int k = 0; k < 4; ++k) { ihdr[4 + k] = (uint8_t) (cols >> (24 - 8 * k)); ihdr[8 + k] = (uint8_t) (rows >> (24 - 8 * k)); }
    const uint32_t crc = crc32_of(ihdr, 17u);
    for (uint32_t i = 0u; i < 12u; ++i) put(i, sig[i]);
    for (uint32_t i = 0u; i < 17u; ++i) put(12u + i, ihdr[i]);
    for (uint32_t k = 0u; k < 4u; ++k) { put(29u + k, (uint8_t) (crc >> (24u - 8u * k))); put(33u + k, (uint8_t) (idat_len >> (24u - 8u * k))); }
    put(37u, (uint8_t) 'I'); put(38u, (uint8_t) 'D'); put(39u, (uint8_t) 'A'); put(40u, (uint8_t) 'T');
    put(41u, (uint8_t) 0x78); put(42u, (uint8_t) 0x01);
}
RTP_HD uint32_t idat_crc_start() { // crc32 of "IDAT" 78 01
    const uint8_t b[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    return crc32_of(b, 6u);
}
// crc_tiles: crc32 of "IDAT", the zlib header and every tile.
template <class Put> RTP_HD void write_tail(uint32_t adler, uint32_t crc_tiles, Put put) {
    uint8_t t[TAIL_BYTES] = {1, 0, 0, 0xFF, 0xFF, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int k = 0; k < 4; ++k) t[5 + k] = (uint8_t) (adler >> (24 - 8 * k));
    const uint32_t crc = crc32_of(t, 9u, crc_tiles);
    for (int k = 0; k < 4; ++k) t[9 + k] = (uint8_t) (crc >> (24 - 8 * k));
    for (uint32_t i = 0u; i < (uint32_t) TAIL_BYTES; ++i) put(i, t[i]);
}

// ---- a batch of equal-sized images: K files behind one another, offsets by ONE scan (DESIGN.md "PNG files of a batch of views") ----
// An image has tile_count + 1 scan entries, its tiles and then its TAIL: entry (v, t) is tile t of image v, entry (v, tiles) the bytes between
// image v's last tile and image v + 1's first -- v's TAIL_BYTES and, but behind the last image, the next file's HEAD_BYTES.  The scan starts
// at HEAD_BYTES (file 0's head), so a scanned tile entry is the offset of that tile, a scanned tail entry the offset of that file's last 25
// bytes, and the scan's total is the length of all files: no byte is charged twice or left out, and the capacity decision is exact.
// -DRTP_VIEWS_MUTANT=1..3 (tests/c/png_views_table.cpp's own builds, CPU only): three wrong layouts that the table must catch.
#ifndef RTP_VIEWS_MUTANT
#define RTP_VIEWS_MUTANT 0
#endif
RTP_HD uint64_t views_image_entries(uint64_t tiles) { return tiles + 1u; }
RTP_HD uint64_t views_entry_count(uint64_t n_views, uint64_t tiles) { return n_views * views_image_entries(tiles); }
RTP_HD uint64_t views_entry(uint64_t v, uint64_t t, uint64_t tiles) { // t == tiles: the image's tail entry
#if RTP_VIEWS_MUTANT == 2
    return v * views_image_entries(tiles) + t - (v ? 1u : 0u);
#else
    return v * views_image_entries(tiles) + t;
#endif
}
RTP_HD uint64_t views_first_bytes() { return (uint64_t) HEAD_BYTES; } // in front of entry 0
// What the entries that are not tiles count: t == tiles -> the tail and the next head; every other entry counts its tile's bytes.
RTP_HD uint64_t views_tail_entry_bytes(uint64_t v, uint64_t n_views) {
#if RTP_VIEWS_MUTANT == 1
    return (uint64_t) TAIL_BYTES + (v > 0u ? (uint64_t) HEAD_BYTES : 0u); // the head in front of image v charged behind image v
#else
    return (uint64_t) TAIL_BYTES + (v + 1u < n_views ? (uint64_t) HEAD_BYTES : 0u);
#endif
}
// From the scanned entries (offsets): where file v starts and ends, and its IDAT chunk's length.  `total` is the scan's total.
template <class Scanned> RTP_HD uint64_t views_file_start(Scanned scanned, uint64_t v, uint64_t tiles) { return (uint64_t) scanned[views_entry(v, 0u, tiles)] - (uint64_t) HEAD_BYTES; }
template <class Scanned> RTP_HD uint64_t views_file_end(Scanned scanned, uint64_t v, uint64_t tiles) { return (uint64_t) scanned[views_entry(v, tiles, tiles)] + (uint64_t) TAIL_BYTES; }
template <class Scanned> RTP_HD uint32_t views_idat_length(Scanned scanned, uint64_t v, uint64_t tiles, uint64_t total) {
#if RTP_VIEWS_MUTANT == 3
    (void) scanned; (void) v; (void) tiles;
    return (uint32_t) (total - (uint64_t) HEAD_BYTES - (uint64_t) TAIL_BYTES + (uint64_t) IDAT_EXTRA);
#else
    (void) total;
    return (uint32_t) ((uint64_t) scanned[views_entry(v, tiles, tiles)] - (uint64_t) scanned[views_entry(v, 0u, tiles)] + (uint64_t) IDAT_EXTRA);
#endif
}
// The writing kernels run only into a buffer that holds every file whole.
RTP_HD bool views_go(uint64_t total, uint64_t capacity, bool have_out) { return have_out && total <= capacity; }
// the K files of images whose every tile is stored: no batch is longer
RTP_HD uint64_t views_max_bytes(uint64_t n_views, uint64_t rows, uint64_t cols) { return n_views * max_bytes(rows, cols); }

// ---- the host formatter: the same functions in loops ----
// One tile: f[0 .. n) filtered bytes into out (zeroed, at least STORED_HEAD + n bytes); returns the tile's byte count.  out == nullptr: the count only.
static inline uint32_t format_tile(const uint8_t *f, uint32_t n, uint8_t *out, BuildScratch &s, TilePlan &p) {
    uint32_t hist[LL_SYMS] = {0};
    hist[EOB] = 1u;
    for (uint32_t i = 0u; i < n;) {
        uint32_t L = 1u;
        while (i + L < n && f[i + L] == f[i]) ++L;
        for (uint32_t k = 0u; k < L; ++k) {
            const uint32_t t = token_at(k, L);
            if (t == 1u) hist[f[i]]++;
            else if (t) { uint32_t sym, eb, ev; length_symbol(t, sym, eb, ev); hist[sym]++; }
        }
        i += L;
    }
    uint32_t m = 0u;
    for (uint32_t i = 0u; i < (uint32_t) LL_SYMS; ++i)
        if (hist[i]) { s.order[rank_of(hist, (uint32_t) LL_SYMS, i)] = (uint16_t) i; ++m; }
    plan_tile(hist, m, n, s, p);
    if (!out) return p.bytes;
    if (p.btype == BT_STORED) {
        out[0] = 0; out[1] = (uint8_t) n; out[2] = (uint8_t) (n >> 8); out[3] = (uint8_t) ~n; out[4] = (uint8_t) (~n >> 8);
        for (uint32_t i = 0u; i < n; ++i) out[STORED_HEAD + i] = f[i];
        return p.bytes;
    }
    auto put = [out](uint32_t at, uint32_t v, uint32_t nbits) {
        for (uint64_t x = (uint64_t) v << (at & 7u), b = at >> 3; nbits && x; x >>= 8, ++b) out[b] |= (uint8_t) x;
    };
    uint32_t at = write_block_header(p, put);
    for (uint32_t i = 0u; i < n;) {
        uint32_t L = 1u;
        while (i + L < n && f[i + L] == f[i]) ++L;
        for (uint32_t k = 0u; k < L; ++k) {
            const uint32_t t = token_at(k, L);
            if (!t) continue;
            uint32_t v;
            const uint32_t nb = token_bits(p, t, f[i], v);
            put(at, v, nb); at += nb;
        }
        i += L;
    }
    put(at, p.ll_code[EOB], p.ll_len[EOB]); // then the marker: 000, zeros to the byte boundary, 00 00 FF FF
    out[p.bytes - 2u] = 0xFF; out[p.bytes - 1u] = 0xFF;
    return p.bytes;
}

// The whole file of rgb (rows x cols x 3) mapped through gamma[256] into out, which holds max_bytes(rows, cols); returns the length.
static inline uint64_t format_png(const uint8_t *rgb, uint32_t rows, uint32_t cols, const uint8_t *gamma, uint8_t *out) {
    const uint64_t N = filtered_bytes(rows, cols), stride = 1u + 3u * (uint64_t) cols, T = (uint64_t) RTO_PNG_TILE_BYTES;
    uint8_t *f = new uint8_t[(size_t) T];
    BuildScratch *s = new BuildScratch;
    TilePlan *p = new TilePlan;
    uint64_t at = (uint64_t) HEAD_BYTES;
    uint32_t adler = 1u, crc = idat_crc_start();
    for (uint64_t i0 = 0u; i0 < N; i0 += T) {
        const uint32_t n = (uint32_t) (N - i0 < T ? N - i0 : T);
        for (uint32_t k = 0u; k < n; ++k) {
            const uint64_t i = i0 + k, r = i / stride, j = i % stride;
            if (j == 0u) { f[k] = 1; continue; }
            const uint8_t *px = rgb + r * (stride - 1u) + (j - 1u);
            f[k] = filter_sub(gamma[px[0]], j >= 4u ? gamma[*(px - 3)] : (uint8_t) 0);
        }
        uint8_t *tile = out + at;
        for (uint32_t k = 0u; k < (uint32_t) STORED_HEAD + n; ++k) tile[k] = 0; // a tile is never longer than its stored form
        const uint32_t bytes = format_tile(f, n, tile, *s, *p);
        adler = adler_combine(adler, adler32_of(f, n), n);
        crc = crc_combine(crc, crc32_of(tile, bytes), bytes);
        at += bytes;
    }
    write_head(rows, cols, (uint32_t) (at - HEAD_BYTES + IDAT_EXTRA), [out](uint32_t i, uint8_t b) { out[i] = b; });
    uint8_t *tail = out + at;
    write_tail(adler, crc, [tail](uint32_t i, uint8_t b) { tail[i] = b; });
    delete[] f; delete s; delete p;
    return at + (uint64_t) TAIL_BYTES;
}

} // namespace rtp
