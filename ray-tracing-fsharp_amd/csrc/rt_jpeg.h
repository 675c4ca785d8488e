// rt_jpeg.h -- LoadImage.fromResource (RayTracing.App/LoadImage.fs:9-18): the decode of a baseline JPEG into the R, G, B bytes that
// ParameterisedTexture.ofImage (Texture.fs:30-48) takes, defined ONCE and bit for bit libjpeg's (Huffman, jpeg_idct_islow, "fancy"
// upsampling, the fixed-point YCbCr conversion).  Plain C++ over plain integers: the host decoder (rt_decode_jpeg), the kernels
// (rt_jpeg_kernels.h) and tests/c/jpeg_table.cpp, which drives the subsequence algorithm on a CPU, inline the same functions.
// DESIGN.md "JPEG on the device".
//
// Accepted: SOF0, 8-bit, 1 or 3 components (YCbCr) in ONE interleaved scan (Ss 0, Se 63, Ah Al 0), 8-bit quantisers, every component
// 1x1 or luma 2x1 / 2x2 over 1x1 chroma, with or without DRI, any APPn / COM.  Everything else that is a JPEG: RT_ERR_UNSUPPORTED; what
// is no JPEG, or a damaged one: RT_ERR_INVALID_ARGUMENT.
//
// The entropy-coded bytes, cleaned (FF 00 -> FF, FF D0..D7 removed), are ONE bit stream; the clean-stream bit positions of the removed
// restart markers are the `bounds`.  A decoder is (bit position p, zig-zag index k, block index within the MCU), and `step` advances
// one from any such state -- the true one or a guess -- over a subsequence.  The boundary rule needs no MCU count: the next bound (or
// the data's end) bounds every symbol; one that does not fit in front of it is not decoded, the decoder moves to the bound and begins
// the first block of an MCU there.  Whether the blocks in front of every bound number what the restart interval says is checked with
// the true states only (PlaceSink).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTJ_HD __host__ __device__ inline
#define RTJ_MEMBER __host__ __device__
#else
#define RTJ_HD static inline
#define RTJ_MEMBER
#endif

#define RTJ_DEFAULT_SUBSEQUENCE 128 /* bytes of clean stream per thread of the synchronising rounds (NOTES.md has the table) */
#define RTJ_MIN_SUBSEQUENCE 4       /* a symbol is at most 16 + 11 (DC) or 16 + 15 (AC) bits: every 32-bit run holds a symbol start */
#define RTJ_MAX_CLEAN_BYTES (1u << 28) /* bit positions are 32-bit */

namespace rtj {

enum { OK = 0, INVALID = 1, UNSUPPORTED = 4 };             // RT_OK, RT_ERR_INVALID_ARGUMENT, RT_ERR_UNSUPPORTED
enum { BAD_CODE = 1, BAD_INDEX = 2, BAD_COUNT = 4 };        // what a verified decode met
enum { GREY = 0, S444 = 1, S422 = 2, S420 = 3 };            // the sampling class

// BITS / HUFFVAL as libjpeg's decoding tables: a code of length l is the value's index `valoff[l] + code` when code <= maxcode[l];
// look[w]: (length << 8 | value) of the code that the 8 bits w begin with, 0 when it is longer than 8 bits.
struct Huff {
    int32_t maxcode[17], valoff[17];
    uint16_t look[256];
    uint8_t val[256];
};
struct Tables { Huff dc[3], ac[3]; }; // by component
struct Frame {
    uint32_t W, H, ncomp, cls, Ri, B;         // B: blocks per MCU
    uint32_t mcux, mcuy, total;               // total = mcux * mcuy * B blocks
    uint32_t hs[3], vs[3], first_blk[3];      // sampling factors; the first block of the component within the MCU
    uint32_t dc_base[3];                      // where the component's DC values begin in the by-component array
    uint32_t pw[3], cw[3], ch[3];             // plane width in samples with the MCU padding; the cropped plane (what upsampling sees)
    uint64_t plane_at[3], plane_bytes;        // planes in one buffer
    uint8_t comp_of[8];                       // block within the MCU -> component
    uint16_t q[3][64];                        // quantisers by component, zig-zag order as in the file
};
struct State { uint32_t p, kb; };             // bit position; k | block-in-MCU << 8
RTJ_HD bool same(State a, State b) { return a.p == b.p && a.kb == b.kb; }

RTJ_HD uint32_t natural_of(uint32_t k) { // zig-zag index -> row * 8 + column
    return (uint32_t) (uint8_t) "\x00\x01\x08\x10\x09\x02\x03\x0a\x11\x18\x20\x19\x12\x0b\x04\x05\x0c\x13\x1a\x21\x28\x30\x29\x22\x1b\x14\x0d\x06\x07\x0e\x15\x1c"
                                "\x23\x2a\x31\x38\x39\x32\x2b\x24\x1d\x16\x0f\x17\x1e\x25\x2c\x33\x3a\x3b\x34\x2d\x26\x1f\x27\x2e\x35\x3c\x3d\x36\x2f\x37\x3e\x3f"[k];
}

// ---- the bit stream ----------------------------------------------------------------------------------------------------------
// the 32 bits at bit position p; bytes behind the end read as FF.  No byte at or behind nbytes is touched.
RTJ_HD uint32_t window(const uint8_t *d, uint32_t nbytes, uint32_t p) {
    const uint32_t i = p >> 3;
    uint64_t w = 0;
    for (uint32_t k = 0; k < 5u; ++k) w = (w << 8) | (i + k < nbytes ? d[i + k] : 0xFFu);
    return (uint32_t) ((w << (p & 7u)) >> 8);
}
RTJ_HD bool lookup(const Huff &h, uint32_t w, uint32_t &len, uint32_t &sym) {
    const uint32_t e = h.look[w >> 24];
    if (e) { len = e >> 8; sym = e & 255u; return true; }
    for (uint32_t l = 9; l <= 16u; ++l) {
        const int32_t code = (int32_t) (w >> (32u - l));
        if (code <= h.maxcode[l]) { len = l; sym = h.val[(uint32_t) (h.valoff[l] + code) & 255u]; return true; }
    }
    return false;
}
RTJ_HD int32_t extend(uint32_t v, uint32_t n) { return n == 0u ? 0 : (v >= (1u << (n - 1u)) ? (int32_t) v : (int32_t) v - (int32_t) (1u << n) + 1); }
// the first j with bounds[j] >= p
RTJ_HD uint32_t next_bound(const uint32_t *bounds, uint32_t nb, uint32_t p) {
    uint32_t lo = 0, hi = nb;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (bounds[mid] < p) lo = mid + 1u; else hi = mid; }
    return lo;
}

// The subsequence step: from state s, every symbol that STARTS in front of bit `end` (end <= nbits).  Leaves the state behind the last
// of them in s and returns the number of blocks completed.  sink.coef(n, k, v): the coefficient (k == 0: the DC difference) at zig-zag
// index k of the n-th block this call works on (0: the one it entered in); sink.bound(j, n): bound j is passed with n blocks completed;
// sink.bad(what).  Every iteration consumes at least one bit or passes one bound.
template <class Sink>
RTJ_HD uint32_t step(const Frame &f, const Tables &t, const uint8_t *data, uint32_t nbits, const uint32_t *bounds, uint32_t nb, State &s, uint32_t end, Sink &sink) {
    uint32_t p = s.p, k = s.kb & 255u, blk = s.kb >> 8, n = 0;
    uint32_t j = next_bound(bounds, nb, p), limit = j < nb ? bounds[j] : nbits;
    const uint32_t nbytes = (nbits + 7u) >> 3;
    while (p < end) {
        if (p >= limit) { // (j < nb: limit == nbits would have ended the loop)
            sink.bound(j, n);
            k = 0; blk = 0; ++j;
            limit = j < nb ? bounds[j] : nbits;
            continue;
        }
        const uint32_t w = window(data, nbytes, p), room = limit - p, c = f.comp_of[blk & 7u];
        uint32_t len = 0, sym = 0;
        if (!lookup(k == 0u ? t.dc[c] : t.ac[c], w, len, sym)) {
            if (room < 16u) { p = limit; continue; } // the pad bits in front of a bound: an unfinished symbol
            sink.bad((uint32_t) BAD_CODE); // any fixed rule will do: a verified decode that meets it is an error
            p += 1u; k = 0;
            continue;
        }
        const uint32_t ext = k == 0u ? (sym < 12u ? sym : 11u) : (sym & 15u);
        if (len + ext > room) { p = limit; continue; }
        const int32_t v = extend(ext ? (w << len) >> (32u - ext) : 0u, ext);
        p += len + ext;
        if (k == 0u) {
            sink.coef(n, 0u, v);
            k = 1;
        } else if ((sym & 15u) == 0u) {
            k = (sym >> 4) == 15u ? k + 16u : 64u; // sixteen zeros, or the end of the block
        } else {
            k += sym >> 4;
            if (k > 63u) { sink.bad((uint32_t) BAD_INDEX); k = 64; }
            else { sink.coef(n, k, v); ++k; }
        }
        if (k >= 64u) { k = 0; ++n; blk = blk + 1u >= f.B ? 0u : blk + 1u; }
    }
    s.p = p; s.kb = k | (blk << 8);
    return n;
}

struct NoSink {
    RTJ_MEMBER void coef(uint32_t, uint32_t, int32_t) {}
    RTJ_MEMBER void bound(uint32_t, uint32_t) {}
    RTJ_MEMBER void bad(uint32_t) {}
};
// The placing sink: `first` = the blocks completed in front of the subsequence.  Every store is behind a check against the total.
struct PlaceSink {
    const Frame *f;
    int16_t *coefs;
    uint32_t first, flags;
    RTJ_MEMBER void coef(uint32_t n, uint32_t k, int32_t v) {
        const uint64_t g = (uint64_t) first + n;
        if (g < f->total) coefs[g * 64u + k] = (int16_t) v;
    }
    RTJ_MEMBER void bound(uint32_t j, uint32_t n) { // the blocks in front of bound j: exactly (j + 1) intervals' worth
        if ((uint64_t) first + n != ((uint64_t) j + 1u) * f->Ri * f->B) flags |= (uint32_t) BAD_COUNT;
    }
    RTJ_MEMBER void bad(uint32_t what) { flags |= what; }
};

// Subsequence i of S bytes: its bits, and the state it is guessed to start in (the true one for i == 0 and on a bound).
RTJ_HD uint32_t sub_end(uint32_t i, uint32_t S, uint32_t nbits) { const uint64_t e = ((uint64_t) i + 1u) * S * 8u; return e < nbits ? (uint32_t) e : nbits; }
RTJ_HD State sub_guess(uint32_t i, uint32_t S) { return State{i * S * 8u, 0u}; }
// One round for subsequence i.  Round 0 decodes from the guess; a later one takes the end state its predecessor left in the round
// before, and decodes again only when that differs from what it started from.  Returns whether it decoded.
RTJ_HD bool sync_round(const Frame &f, const Tables &t, const uint8_t *data, uint32_t nbits, const uint32_t *bounds, uint32_t nb, uint32_t S, uint32_t i, uint32_t round,
                       State *start, const State *end_prev, State *end_cur, uint32_t *count) {
    if (round > 0u) {
        const State cand = i == 0u ? start[0] : end_prev[i - 1u];
        if (same(cand, start[i])) { end_cur[i] = end_prev[i]; return false; }
        start[i] = cand;
    } else {
        start[i] = sub_guess(i, S);
    }
    State s = start[i];
    NoSink sink;
    count[i] = step(f, t, data, nbits, bounds, nb, s, sub_end(i, S, nbits), sink);
    end_cur[i] = s;
    return true;
}

// ---- the clean stream ----------------------------------------------------------------------------------------------------------
RTJ_HD bool is_rst(uint32_t b) { return b - 0xD0u < 8u; }
// Within the entropy-coded bytes every FF is followed by 00 or D0..D7 (anything else ends them), so both rules are local.
RTJ_HD bool is_bound(const uint8_t *raw, uint32_t n, uint32_t i) { return raw[i] == 0xFFu && i + 1u < n && is_rst(raw[i + 1u]); }
RTJ_HD bool is_kept(const uint8_t *raw, uint32_t n, uint32_t i) {
    if (is_bound(raw, n, i)) return false;
    return !(i > 0u && raw[i - 1u] == 0xFFu && (raw[i] == 0u || is_rst(raw[i])));
}

// ---- samples ---------------------------------------------------------------------------------------------------------------------
// jpeg_idct_islow's pass over v[0], v[st], .. v[7 * st]; 32-bit arithmetic that wraps (a damaged file may overflow it; libjpeg's int does
// the same on every machine this runs on), D(x, n) with an arithmetic shift.
RTJ_HD int32_t descale(uint32_t x, uint32_t n) { return (int32_t) (x + (1u << (n - 1u))) >> n; }
RTJ_HD void idct_pass(int32_t *v, uint32_t st, uint32_t n) {
    const uint32_t i0 = (uint32_t) v[0], i1 = (uint32_t) v[st], i2 = (uint32_t) v[2 * st], i3 = (uint32_t) v[3 * st], i4 = (uint32_t) v[4 * st],
                   i5 = (uint32_t) v[5 * st], i6 = (uint32_t) v[6 * st], i7 = (uint32_t) v[7 * st];
    uint32_t z1 = (i2 + i6) * 4433u;
    const uint32_t t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u, t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t o0 = i7, o1 = i5, o2 = i3, o3 = i1;
    z1 = o0 + o3;
    uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    o0 *= 2446u; o1 *= 16819u; o2 *= 25172u; o3 *= 12299u;
    z1 *= (uint32_t) -7373; z2 *= (uint32_t) -20995;
    z3 = z3 * (uint32_t) -16069 + z5; z4 = z4 * (uint32_t) -3196 + z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    v[0] = descale(t10 + o3, n); v[st] = descale(t11 + o2, n); v[2 * st] = descale(t12 + o1, n); v[3 * st] = descale(t13 + o0, n);
    v[4 * st] = descale(t13 - o0, n); v[5 * st] = descale(t12 - o1, n); v[6 * st] = descale(t11 - o2, n); v[7 * st] = descale(t10 - o3, n);
}
RTJ_HD uint8_t clamp255(int32_t x) { return (uint8_t) (x < 0 ? 0 : (x > 255 ? 255 : x)); }
// One block: coef in zig-zag order (coef[0] is not read: dc is the summed DC), quantisers alike; samples to out[row * stride + column].
RTJ_HD void idct_block(const int16_t *coef, int32_t dc, const uint16_t *q, uint8_t *out, size_t stride) {
    int32_t ws[64];
    ws[0] = (int32_t) ((uint32_t) dc * q[0]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 1; k < 64u; ++k) ws[natural_of(k)] = (int32_t) coef[k] * (int32_t) q[k];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t c = 0; c < 8u; ++c) idct_pass(ws + c, 8u, 11u);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t r = 0; r < 8u; ++r) {
        idct_pass(ws + 8u * r, 1u, 18u);
        for (uint32_t c = 0; c < 8u; ++c) out[r * stride + c] = clamp255((int32_t) ((uint32_t) ws[8u * r + c] + 128u));
    }
}
// Block g in decode order: its component, where its DC difference lies in the by-component array (gi), the first index of its restart
// interval there (seg), and its block row and column in the component's plane.
RTJ_HD void block_place(const Frame &f, uint32_t g, uint32_t &c, uint32_t &gi, uint32_t &seg, uint32_t &brow, uint32_t &bcol) {
    const uint32_t m = g / f.B, jb = g - m * f.B;
    c = f.comp_of[jb];
    const uint32_t local = jb - f.first_blk[c], per = f.hs[c] * f.vs[c], my = m / f.mcux, mx = m - my * f.mcux;
    gi = f.dc_base[c] + m * per + local;
    seg = f.dc_base[c] + (f.Ri ? m / f.Ri * f.Ri * per : 0u);
    brow = my * f.vs[c] + local / f.hs[c];
    bcol = mx * f.hs[c] + local % f.hs[c];
}
// dcsum: the inclusive sums (modulo 2^32) of the by-component DC differences; the block's DC is its sum within its restart interval
RTJ_HD int32_t block_dc(const uint32_t *dcsum, uint32_t gi, uint32_t seg) { return (int32_t) (int16_t) (dcsum[gi] - (seg ? dcsum[seg - 1u] : 0u)); }
RTJ_HD void block_samples(const Frame &f, const int16_t *coefs, const uint32_t *dcsum, uint32_t g, uint8_t *planes) {
    uint32_t c, gi, seg, brow, bcol;
    block_place(f, g, c, gi, seg, brow, bcol);
    idct_block(coefs + (size_t) g * 64u, block_dc(dcsum, gi, seg), f.q[c], planes + f.plane_at[c] + ((size_t) brow * 8u * f.pw[c] + (size_t) bcol * 8u), f.pw[c]);
}

// libjpeg's "fancy" upsampling of the cropped chroma plane, one output sample: edges replicated.
RTJ_HD uint32_t chroma_at(const Frame &f, const uint8_t *plane, uint32_t c, uint32_t x, uint32_t y) {
    const uint32_t pw = f.pw[c], cw = f.cw[c], ch = f.ch[c];
    if (f.cls != (uint32_t) S422 && f.cls != (uint32_t) S420) return plane[(size_t) y * pw + x];
    const uint32_t i = x >> 1, near = (x & 1u) ? (i + 1u < cw ? i + 1u : i) : (i ? i - 1u : 0u);
    if (f.cls == (uint32_t) S422) {
        const uint8_t *row = plane + (size_t) y * pw;
        return (3u * row[i] + row[near] + ((x & 1u) ? 2u : 1u)) >> 2;
    }
    const uint32_t jr = y >> 1, other = (y & 1u) ? (jr + 1u < ch ? jr + 1u : jr) : (jr ? jr - 1u : 0u);
    const uint8_t *a = plane + (size_t) jr * pw, *b = plane + (size_t) other * pw;
    const uint32_t s = 3u * a[i] + b[i], sn = 3u * a[near] + b[near];
    return (3u * s + sn + ((x & 1u) ? 7u : 8u)) >> 4;
}
RTJ_HD void pixel_rgb(const Frame &f, const uint8_t *planes, uint32_t x, uint32_t y, uint8_t *rgb) {
    const int32_t Y = planes[f.plane_at[0] + (size_t) y * f.pw[0] + x];
    if (f.ncomp == 1u) { rgb[0] = rgb[1] = rgb[2] = (uint8_t) Y; return; }
    const int32_t cb = (int32_t) chroma_at(f, planes + f.plane_at[1], 1u, x, y) - 128, cr = (int32_t) chroma_at(f, planes + f.plane_at[2], 2u, x, y) - 128;
    rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
    rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

} // namespace rtj

// ======================================================================================================================================
// Host only: the header parse, the sequential decoder and the subsequence algorithm as a loop.
// ======================================================================================================================================
#include <string>
#include <vector>

namespace rtj {

struct Parsed {
    Frame f{};
    Tables t{}; // (a greyscale file fills dc[0] and ac[0] alone: the rest goes to the device as zeros)
    size_t ecs_at = 0, ecs_raw = 0; // the entropy-coded bytes in the file
    uint32_t n_clean = 0, n_rst = 0;
};
static inline int refuse(std::string &err, int code, const std::string &msg) { err = "jpeg: " + msg; return code; }
static inline std::string at(size_t pos) { return " at byte " + std::to_string(pos); }

static inline int build_huff(const uint8_t *bits, const uint8_t *vals, uint32_t nvals, bool dc, Huff &h, std::string &err, size_t pos) {
    for (uint32_t w = 0; w < 256u; ++w) h.look[w] = 0;
    for (uint32_t i = 0; i < 256u; ++i) h.val[i] = i < nvals ? vals[i] : 0;
    uint32_t code = 0, k = 0;
    h.maxcode[0] = -1; h.valoff[0] = 0;
    for (uint32_t l = 1; l <= 16u; ++l) {
        h.valoff[l] = (int32_t) k - (int32_t) code;
        if (code + bits[l - 1u] > (1u << l)) return refuse(err, INVALID, "a Huffman table with more codes of length " + std::to_string(l) + " than there are" + at(pos));
        for (uint32_t i = 0; i < bits[l - 1u]; ++i, ++k, ++code) {
            if (dc && vals[k] > 11u) return refuse(err, INVALID, "a DC Huffman table with the category " + std::to_string(vals[k]) + at(pos));
            if (l <= 8u)
                for (uint32_t w = code << (8u - l); w < ((code + 1u) << (8u - l)); ++w) h.look[w] = (uint16_t) (l << 8 | vals[k]);
        }
        h.maxcode[l] = bits[l - 1u] ? (int32_t) code - 1 : -1;
        code <<= 1;
    }
    return OK;
}

static inline int parse(const uint8_t *d, size_t n, Parsed &out, std::string &err) {
    if (n < 2u || d[0] != 0xFFu || d[1] != 0xD8u) return refuse(err, INVALID, "no SOI marker at byte 0");
    uint8_t qt[4][64]; bool have_q[4] = {false, false, false, false};
    std::vector<Huff> huff(8); bool have_h[8] = {false, false, false, false, false, false, false, false}; // [class * 4 + id]
    bool have_sof = false; int adobe = -1;
    uint32_t cid[3] = {0, 0, 0}, tq[3] = {0, 0, 0};
    Frame &f = out.f;
    f = Frame{};
    size_t pos = 2;
    for (;;) {
        if (pos + 2u > n) return refuse(err, INVALID, "the file ends before any scan" + at(pos));
        if (d[pos] != 0xFFu) return refuse(err, INVALID, "no marker" + at(pos));
        const uint32_t m = d[pos + 1u];
        if (m == 0xFFu) { ++pos; continue; } // a fill byte
        if (m == 0x01u || is_rst(m)) { pos += 2u; continue; }
        if (m == 0xD9u) return refuse(err, INVALID, "EOI before any scan" + at(pos));
        if (m == 0xD8u) return refuse(err, INVALID, "a second SOI" + at(pos));
        if (pos + 4u > n) return refuse(err, INVALID, "a segment that runs past the end" + at(pos));
        const size_t L = (size_t) d[pos + 2u] << 8 | d[pos + 3u];
        if (L < 2u || pos + 2u + L > n) return refuse(err, INVALID, "a segment that runs past the end" + at(pos));
        const uint8_t *seg = d + pos + 4u;
        const size_t sl = L - 2u;
        if (m == 0xDBu) {
            for (size_t p = 0; p < sl;) {
                if (seg[p] >> 4) return refuse(err, UNSUPPORTED, "a 16-bit quantisation table" + at(pos));
                if ((seg[p] & 15u) > 3u || p + 65u > sl) return refuse(err, INVALID, "a malformed DQT segment" + at(pos));
                for (uint32_t k = 0; k < 64u; ++k) qt[seg[p] & 15u][k] = seg[p + 1u + k];
                have_q[seg[p] & 15u] = true;
                p += 65u;
            }
        } else if (m == 0xC4u) {
            for (size_t p = 0; p < sl;) {
                if (p + 17u > sl || (seg[p] >> 4) > 1u || (seg[p] & 15u) > 3u) return refuse(err, INVALID, "a malformed DHT segment" + at(pos));
                uint32_t nv = 0;
                for (uint32_t l = 0; l < 16u; ++l) nv += seg[p + 1u + l];
                if (nv > 256u || p + 17u + nv > sl) return refuse(err, INVALID, "a malformed DHT segment" + at(pos));
                const uint32_t slot = (seg[p] >> 4) * 4u + (seg[p] & 15u);
                const int rc = build_huff(seg + p + 1u, seg + p + 17u, nv, (seg[p] >> 4) == 0u, huff[slot], err, pos);
                if (rc != OK) return rc;
                have_h[slot] = true;
                p += 17u + nv;
            }
        } else if (m == 0xC0u) {
            if (have_sof) return refuse(err, INVALID, "a second frame header" + at(pos));
            if (sl < 6u) return refuse(err, INVALID, "a malformed SOF0 segment" + at(pos));
            if (seg[0] != 8u) return refuse(err, UNSUPPORTED, std::to_string(seg[0]) + "-bit samples" + at(pos));
            f.H = (uint32_t) seg[1] << 8 | seg[2]; f.W = (uint32_t) seg[3] << 8 | seg[4]; f.ncomp = seg[5];
            if (f.W == 0u || f.H == 0u) return refuse(err, INVALID, "a zero dimension" + at(pos));
            if (f.ncomp == 4u) return refuse(err, UNSUPPORTED, "4 components (CMYK / YCCK)" + at(pos));
            if (f.ncomp != 1u && f.ncomp != 3u) return refuse(err, UNSUPPORTED, std::to_string(f.ncomp) + " components" + at(pos));
            if (sl < 6u + 3u * f.ncomp) return refuse(err, INVALID, "a malformed SOF0 segment" + at(pos));
            if ((uint64_t) f.W * f.H > (uint64_t) INT32_MAX) return refuse(err, INVALID, "an image of more than INT32_MAX pixels");
            for (uint32_t c = 0; c < f.ncomp; ++c) {
                cid[c] = seg[6u + 3u * c]; f.hs[c] = seg[7u + 3u * c] >> 4; f.vs[c] = seg[7u + 3u * c] & 15u; tq[c] = seg[8u + 3u * c];
                if (f.hs[c] == 0u || f.vs[c] == 0u || tq[c] > 3u) return refuse(err, INVALID, "a malformed SOF0 segment" + at(pos));
            }
            have_sof = true;
        } else if ((m >= 0xC1u && m <= 0xCFu && m != 0xC8u) ) {
            if (m == 0xC2u) return refuse(err, UNSUPPORTED, "a progressive JPEG (SOF2)" + at(pos));
            if (m >= 0xC9u) return refuse(err, UNSUPPORTED, "arithmetic coding" + at(pos));
            return refuse(err, UNSUPPORTED, "a frame of type SOF" + std::to_string(m - 0xC0u) + at(pos));
        } else if (m == 0xDDu) {
            if (sl != 2u) return refuse(err, INVALID, "a malformed DRI segment" + at(pos));
            f.Ri = (uint32_t) seg[0] << 8 | seg[1];
        } else if (m == 0xEEu && sl >= 12u && seg[0] == 'A' && seg[1] == 'd' && seg[2] == 'o' && seg[3] == 'b' && seg[4] == 'e') {
            adobe = seg[11];
        } else if (m == 0xDAu) {
            if (!have_sof) return refuse(err, INVALID, "a scan before the frame header" + at(pos));
            if (sl < 1u || sl != 4u + 2u * seg[0]) return refuse(err, INVALID, "a malformed SOS segment" + at(pos));
            if (seg[0] != f.ncomp) return refuse(err, UNSUPPORTED, "a scan of " + std::to_string(seg[0]) + " of the " + std::to_string(f.ncomp) + " components (multiple scans)" + at(pos));
            if (f.ncomp == 3u && adobe >= 0 && adobe != 1) return refuse(err, UNSUPPORTED, "an Adobe marker with the transform " + std::to_string(adobe));
            for (uint32_t c = 0; c < f.ncomp; ++c) {
                const uint32_t id = seg[1u + 2u * c], td = seg[2u + 2u * c] >> 4, ta = seg[2u + 2u * c] & 15u;
                if (id != cid[c]) {
                    for (uint32_t o = 0; o < f.ncomp; ++o)
                        if (id == cid[o]) return refuse(err, UNSUPPORTED, "scan components in another order than the frame's" + at(pos));
                    return refuse(err, INVALID, "a scan component " + std::to_string(id) + " that the frame does not define" + at(pos));
                }
                if (td > 3u || ta > 3u || !have_h[td] || !have_h[4u + ta]) return refuse(err, INVALID, "a Huffman table referenced before it is defined" + at(pos));
                if (!have_q[tq[c]]) return refuse(err, INVALID, "a quantisation table referenced before it is defined" + at(pos));
                out.t.dc[c] = huff[td]; out.t.ac[c] = huff[4u + ta];
                for (uint32_t k = 0; k < 64u; ++k) f.q[c][k] = qt[tq[c]][k];
            }
            const uint8_t *tail = seg + 1u + 2u * f.ncomp;
            if (tail[0] != 0u || tail[1] != 63u || tail[2] != 0u) return refuse(err, UNSUPPORTED, "a scan that is not Ss 0, Se 63, Ah Al 0" + at(pos));
            pos += 2u + L;
            break;
        }
        pos += 2u + L;
    }
    // the frame's geometry
    if (f.ncomp == 1u) { f.hs[0] = f.vs[0] = 1u; f.cls = GREY; }
    else {
        const uint32_t h = f.hs[0], v = f.vs[0];
        if (f.hs[1] != 1u || f.vs[1] != 1u || f.hs[2] != 1u || f.vs[2] != 1u || !((h == 1u && v == 1u) || (h == 2u && v == 1u) || (h == 2u && v == 2u)))
            return refuse(err, UNSUPPORTED, "sampling factors other than 4:4:4, 4:2:2 and 4:2:0");
        f.cls = h == 1u ? S444 : (v == 1u ? S422 : S420);
    }
    const uint32_t hmax = f.hs[0], vmax = f.vs[0];
    f.mcux = (f.W + 8u * hmax - 1u) / (8u * hmax); f.mcuy = (f.H + 8u * vmax - 1u) / (8u * vmax);
    f.B = 0;
    const uint64_t mcus = (uint64_t) f.mcux * f.mcuy;
    uint64_t dc_at = 0, plane_at = 0;
    for (uint32_t c = 0; c < f.ncomp; ++c) {
        f.first_blk[c] = f.B;
        for (uint32_t b = 0; b < f.hs[c] * f.vs[c]; ++b) f.comp_of[f.B++] = (uint8_t) c;
        f.dc_base[c] = (uint32_t) dc_at; dc_at += mcus * f.hs[c] * f.vs[c];
        f.pw[c] = f.mcux * f.hs[c] * 8u;
        f.cw[c] = (f.W * f.hs[c] + hmax - 1u) / hmax; f.ch[c] = (f.H * f.vs[c] + vmax - 1u) / vmax;
        f.plane_at[c] = plane_at; plane_at += (uint64_t) f.pw[c] * f.mcuy * f.vs[c] * 8u;
    }
    f.plane_bytes = plane_at;
    f.total = (uint32_t) (mcus * f.B); // (at most 3 * (2^31 / 64 + the padding): 32 bits hold it)
    // the entropy-coded bytes: up to the first FF that neither 00 nor D0..D7 follows
    out.ecs_at = pos;
    size_t i = pos, kept = 0;
    uint32_t rst = 0;
    while (i < n) {
        if (d[i] != 0xFFu) { ++i; ++kept; continue; }
        if (i + 1u < n && d[i + 1u] == 0u) { i += 2u; ++kept; continue; }
        if (i + 1u < n && is_rst(d[i + 1u])) { i += 2u; ++rst; continue; }
        break;
    }
    out.ecs_raw = i - pos;
    if (out.ecs_raw > (size_t) 0x7fffffffu) return refuse(err, UNSUPPORTED, "more than 2^31 - 1 bytes of entropy-coded data and restart markers");
    if (kept >= (size_t) RTJ_MAX_CLEAN_BYTES) return refuse(err, UNSUPPORTED, "more than 2^28 entropy-coded bytes");
    out.n_clean = (uint32_t) kept; out.n_rst = rst;
    // what follows: another scan is refused; the rest (EOI, or nothing) is not looked at
    while (i + 4u <= n && d[i] == 0xFFu) {
        const uint32_t m = d[i + 1u];
        if (m == 0xFFu) { ++i; continue; }
        if (m == 0xDAu) return refuse(err, UNSUPPORTED, "a second scan (multiple scans)" + at(i));
        if (m == 0xD9u || m == 0x01u || is_rst(m)) break;
        i += 2u + ((size_t) d[i + 2u] << 8 | d[i + 3u]);
    }
    return OK;
}

static inline const char *stream_error(uint32_t flags) {
    if (flags & (uint32_t) BAD_CODE) return "jpeg: the entropy-coded data holds a code that is not in its Huffman table";
    if (flags & (uint32_t) BAD_INDEX) return "jpeg: the entropy-coded data holds a coefficient index past 63";
    return "jpeg: the entropy-coded data does not hold the blocks the frame and the restart interval call for (a stream that ends early?)";
}

// What the host knows of the stream before a bit of it is decoded: the restart markers number what the interval calls for, one between
// every two intervals (none without DRI).  With too few the last interval would hold more than Ri MCUs, which no count in front of a
// bound can tell.
static inline uint32_t marker_flags(const Parsed &ps) {
    const uint64_t mcus = (uint64_t) ps.f.mcux * ps.f.mcuy, want = ps.f.Ri ? (mcus + ps.f.Ri - 1u) / ps.f.Ri - 1u : 0u;
    return (uint64_t) ps.n_rst == want ? 0u : (uint32_t) BAD_COUNT;
}

// The clean stream and the bounds, sequentially.
static inline void clean_stream(const uint8_t *raw, uint32_t n, std::vector<uint8_t> &clean, std::vector<uint32_t> &bounds) {
    for (uint32_t i = 0; i < n; ++i) {
        if (is_bound(raw, n, i)) bounds.push_back((uint32_t) clean.size() * 8u);
        else if (is_kept(raw, n, i)) clean.push_back(raw[i]);
    }
}

// The decode in the device route's order of events.  S == 0: one sequential run of `step`; S >= RTJ_MIN_SUBSEQUENCE: the synchronising
// rounds over subsequences of S bytes, a loop in place of the threads, then the placing run per subsequence.  plan (may be null): S,
// subsequences, rounds, subsequence decodes, blocks, bounds.  Nothing of rgb is written unless the status is OK.
static inline int decode_host(const uint8_t *d, size_t n, uint8_t *rgb, size_t capacity, uint32_t S, int64_t *plan, std::string &err) {
    Parsed ps;
    const int rc = parse(d, n, ps, err);
    if (rc != OK) return rc;
    const Frame &f = ps.f;
    if (capacity < (size_t) f.W * f.H * 3u) return refuse(err, INVALID, "capacity " + std::to_string(capacity) + " below the " + std::to_string((size_t) f.W * f.H * 3u) + " bytes of the bitmap");
    if (marker_flags(ps)) { err = stream_error(marker_flags(ps)); return INVALID; }
    std::vector<uint8_t> clean;
    std::vector<uint32_t> bounds;
    clean_stream(d + ps.ecs_at, (uint32_t) ps.ecs_raw, clean, bounds);
    const uint32_t nbits = (uint32_t) clean.size() * 8u, nb = (uint32_t) bounds.size();
    const uint32_t ns = S ? (uint32_t) ((clean.size() + S - 1u) / S) : (nbits ? 1u : 0u), span = S ? S : (uint32_t) clean.size();
    std::vector<State> start(ns), end0(ns), end1(ns);
    std::vector<uint32_t> count(ns + 1u, 0u);
    uint32_t rounds = 0;
    uint64_t decodes = 0;
    for (uint32_t r = 0; r < ns; ++r) { // after round r the first r + 1 subsequences are true: ns rounds at the most
        State *cur = (r & 1u) ? end1.data() : end0.data();
        const State *prev = (r & 1u) ? end0.data() : end1.data();
        uint32_t ran = 0;
        for (uint32_t i = 0; i < ns; ++i) ran += sync_round(f, ps.t, clean.data(), nbits, bounds.data(), nb, span, i, r, start.data(), prev, cur, count.data()) ? 1u : 0u;
        if (ran == 0u) break;
        ++rounds; decodes += ran;
    }
    uint32_t flags = 0, first = 0;
    std::vector<int16_t> coefs((size_t) f.total * 64u, (int16_t) 0);
    for (uint32_t i = 0; i < ns; ++i) { // the exclusive scan of the counts, and the placing run
        PlaceSink sink{&f, coefs.data(), first, 0u};
        State s = start[i];
        (void) step(f, ps.t, clean.data(), nbits, bounds.data(), nb, s, sub_end(i, span, nbits), sink);
        flags |= sink.flags;
        first += count[i];
    }
    if (first != f.total) flags |= (uint32_t) BAD_COUNT;
    if (plan) { plan[0] = span; plan[1] = ns; plan[2] = rounds; plan[3] = (int64_t) decodes; plan[4] = first; plan[5] = nb; plan[6] = plan[7] = 0; }
    if (flags) { err = stream_error(flags); return INVALID; }
    std::vector<uint32_t> dcsum(f.total);
    for (uint32_t g = 0; g < f.total; ++g) {
        uint32_t c, gi, seg, brow, bcol;
        block_place(f, g, c, gi, seg, brow, bcol);
        dcsum[gi] = (uint32_t) (int32_t) coefs[(size_t) g * 64u];
    }
    for (uint32_t i = 1; i < f.total; ++i) dcsum[i] += dcsum[i - 1u];
    std::vector<uint8_t> planes((size_t) f.plane_bytes);
    for (uint32_t g = 0; g < f.total; ++g) block_samples(f, coefs.data(), dcsum.data(), g, planes.data());
    for (uint32_t y = 0; y < f.H; ++y)
        for (uint32_t x = 0; x < f.W; ++x) pixel_rgb(f, planes.data(), x, y, rgb + ((size_t) y * f.W + x) * 3u);
    return OK;
}

} // namespace rtj
