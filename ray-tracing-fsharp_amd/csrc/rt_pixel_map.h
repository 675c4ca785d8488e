// rt_pixel_map.h -- ImageOutput.readPixelMap (ImageOutput.fs:46-113) as a scan, defined ONCE.  Plain C++ over plain integers: the kernels
// (rt_pixel_map_kernels.h) and tests/c/pixel_map_scan_table.cpp, which drives the chunked algorithm on a CPU against the sequential
// parser rth::parse_pixel_map (rt_scene.h), inline the same functions.  DESIGN.md "Resuming from a pixel map".
//
// A record is `<row digits> <non-digit> <column digits> <non-digit> R G B`; the three colour bytes are raw data and may be digits, commas
// or newlines, so no byte tells locally where a record begins.  The reader is nevertheless a five-state automaton over two letters,
// digit (48..57) and anything else:
//   state 0  in the row's digits        digit -> 0   other -> 1
//   state 1  in the column's digits     digit -> 1   other -> 2
//   state 2  first colour byte          any   -> 3
//   state 3  second colour byte         any   -> 4
//   state 4  third colour byte          any   -> 0, one record completed
// A run of bytes is a map from entry state to (exit state, records completed); maps compose associatively, so the entry state and the
// record ordinal of every chunk come out of a scan of the chunks' maps.
//
// Who handles a record: the chunk that holds the byte IN FRONT of the record's first byte -- the third colour byte of the record before
// it, which is where a walk in a known state sees a record begin (state 0 alone does not tell a record's first byte from the middle of
// its row digits).  The file's first record belongs to the chunk of byte 0.  Its owner reads the whole record, however many chunks and
// tiles its digits cross (leading zeros of any length), and nobody else touches it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPM_HD __host__ __device__ inline
#else
#define RPM_HD static inline
#endif

// ---- tiles and chunks (the kernels' shapes; tests read them through rt_pixel_map_tile_bytes() and its neighbours) ----
#define RPM_BLOCK 256         /* threads of a tile's workgroup */
#define RPM_CHUNK_BYTES 16    /* consecutive bytes per thread */
#define RPM_TILE_BYTES (RPM_BLOCK * RPM_CHUNK_BYTES) /* 4 KiB of the map (or of a presence map) staged in LDS */
#define RPM_SCAN_THREADS 1024 /* tile maps per trip of the one scanning workgroup: trips begin at 4 MiB */
#define RPM_HEAD_BYTES 32     /* struct rpm::ParseHead at the front of a call's scratch */

namespace rpm {

enum { STATES = 5, ROW = 0, COL = 1, C0 = 2, C1 = 3, C2 = 4 };
enum { COORD_MAX = 0x7fffffff }; // a digit run saturates here: no image has such a row or column, so the record is malformed

RPM_HD bool is_digit(uint32_t byte) { return byte - 48u < 10u; }
RPM_HD uint32_t next_state(uint32_t s, bool digit) { return s >= (uint32_t) C0 ? (s == (uint32_t) C2 ? 0u : s + 1u) : (digit ? s : s + 1u); }
// 10 * v + d, saturating at COORD_MAX (once there it stays there)
RPM_HD uint32_t push_digit(uint32_t v, uint32_t d) {
    const uint64_t x = 10ull * v + d;
    return v == (uint32_t) COORD_MAX || x >= (uint64_t) COORD_MAX ? (uint32_t) COORD_MAX : (uint32_t) x;
}

// Entry state -> (exit state, records completed): five 3-bit states in `st`, five 32-bit counts.
struct Map {
    uint32_t st;
    uint32_t cnt[STATES];
};
RPM_HD uint32_t exit_state(const Map &m, uint32_t s) { return (m.st >> (3u * s)) & 7u; }
// cnt[s] for an s that is not known at compile time, as four selects: the counts stay in registers on the device
RPM_HD uint32_t count_at(const Map &m, uint32_t s) {
    uint32_t c = m.cnt[0];
    for (uint32_t k = 1; k < (uint32_t) STATES; ++k) c = s == k ? m.cnt[k] : c;
    return c;
}
RPM_HD Map identity() {
    Map m;
    m.st = 0u;
    for (uint32_t s = 0; s < (uint32_t) STATES; ++s) { m.st |= s << (3u * s); m.cnt[s] = 0u; }
    return m;
}
// one byte's map
RPM_HD Map byte_map(uint32_t byte) {
    const bool d = is_digit(byte);
    Map m;
    m.st = 0u;
    for (uint32_t s = 0; s < (uint32_t) STATES; ++s) { m.st |= next_state(s, d) << (3u * s); m.cnt[s] = s == (uint32_t) C2 ? 1u : 0u; }
    return m;
}
// first `a`, then `b`
RPM_HD Map compose(const Map &a, const Map &b) {
    Map m;
    m.st = 0u;
    for (uint32_t s = 0; s < (uint32_t) STATES; ++s) {
        const uint32_t mid = exit_state(a, s);
        m.st |= exit_state(b, mid) << (3u * s);
        m.cnt[s] = a.cnt[s] + count_at(b, mid);
    }
    return m;
}
// the map of n bytes
RPM_HD Map run_map(const uint8_t *p, size_t n) {
    Map m = identity();
    for (size_t i = 0; i < n; ++i) {
        const bool d = is_digit(p[i]);
        uint32_t st = 0u;
        for (uint32_t s = 0; s < (uint32_t) STATES; ++s) {
            const uint32_t at = exit_state(m, s);
            m.cnt[s] += at == (uint32_t) C2 ? 1u : 0u;
            st |= next_state(at, d) << (3u * s);
        }
        m.st = st;
    }
    return m;
}

// Where a walk stands: the state in front of its next byte and the number of records completed in front of it.
struct Entry { uint32_t state, ordinal; };
RPM_HD Entry advance(Entry e, const Map &m) { return Entry{exit_state(m, e.state), e.ordinal + count_at(m, e.state)}; }

// The record that begins at data[start]: row and column (saturating), and `rgb_at`, the index of its first colour byte.  False: the
// data ends before the record's third colour byte -- a truncated tail, which the reader ignores (ImageOutput.fs:69-106).
struct Record { uint32_t row, col; size_t rgb_at; };
// consumeAsciiInteger (ImageOutput.fs:46-66): digits (none: 0), then ONE non-digit; false when the data ends first
RPM_HD bool read_number(const uint8_t *data, size_t n, size_t &pos, uint32_t &value) {
    uint32_t x = 0u;
    for (;;) {
        if (pos >= n) return false;
        const uint32_t b = data[pos++];
        if (!is_digit(b)) break;
        x = push_digit(x, b - 48u);
    }
    value = x;
    return true;
}
RPM_HD bool read_record(const uint8_t *data, size_t n, size_t start, Record &r) {
    size_t pos = start;
    uint32_t row = 0u, col = 0u;
    if (!read_number(data, n, pos, row) || !read_number(data, n, pos, col)) return false;
    if (n - pos < 3u) return false;
    r.row = row; r.col = col; r.rgb_at = pos;
    return true;
}
RPM_HD bool in_image(const Record &r, uint32_t rows, uint32_t cols) { return r.row < rows && r.col < cols; }

// The records a chunk owns.  The walk enters data[begin] in `e` and consumes [begin, end); f(start, ordinal) is called for every record
// that begins behind a byte of the chunk (and for the file's first record when begin == 0), in file order.
template <class F> RPM_HD void for_owned_records(const uint8_t *chunk, size_t begin, size_t end, Entry e, F &&f) {
    if (begin == 0u && begin < end) f((size_t) 0, 0u);
    for (size_t i = begin; i < end; ++i) {
        const bool last = e.state == (uint32_t) C2;
        e.state = next_state(e.state, is_digit(chunk[i - begin]));
        if (last) f(i + 1u, ++e.ordinal);
    }
}

// rth::parse_pixel_map's answer by chunks, on the host (the order of events of the kernels, sequentially): the chunks' maps, their
// exclusive scan in tiles of `tile` chunks, then every chunk's own records; a pixel named twice keeps the LATER record (`winner`: the
// ordinal + 1 of the last record per pixel, rows * cols words, zero on entry).  Returns the number of complete records, or -1 when one
// of them names a pixel outside the image -- and then nothing of rgb or present has been written.  starts (may be null) receives every
// complete record's first byte, by ordinal.
template <class Starts>
static inline int64_t parse_chunked(const uint8_t *data, size_t n, uint32_t rows, uint32_t cols, size_t chunk, size_t tile, uint32_t *winner, uint8_t *rgb,
                                    uint8_t *present, Starts *starts) {
    const size_t n_chunks = (n + chunk - 1u) / chunk, n_tiles = (n_chunks + tile - 1u) / tile;
    Map *maps = new Map[n_chunks + 1u];
    Map *tiles = new Map[n_tiles + 1u];
    Entry *entry = new Entry[n_chunks + 1u];
    for (size_t c = 0; c < n_chunks; ++c) maps[c] = run_map(data + c * chunk, (c + 1u) * chunk <= n ? chunk : n - c * chunk);
    for (size_t t = 0; t < n_tiles; ++t) { // a tile's map
        Map m = identity();
        for (size_t c = t * tile; c < (t + 1u) * tile && c < n_chunks; ++c) m = compose(m, maps[c]);
        tiles[t] = m;
    }
    Entry at{0u, 0u}; // the scan over the tiles, then inside each
    for (size_t t = 0; t < n_tiles; ++t) {
        Entry e = at;
        for (size_t c = t * tile; c < (t + 1u) * tile && c < n_chunks; ++c) { entry[c] = e; e = advance(e, maps[c]); }
        at = advance(at, tiles[t]);
    }
    const int64_t count = (int64_t) at.ordinal;
    bool bad = false;
    for (int pass = 0; pass < 2 && !bad; ++pass) // claim (and find a malformed record), then store
        for (size_t c = 0; c < n_chunks; ++c) {
            const size_t begin = c * chunk, end = begin + chunk <= n ? begin + chunk : n;
            for_owned_records(data + begin, begin, end, entry[c], [&](size_t start, uint32_t ordinal) {
                Record r;
                if (!read_record(data, n, start, r)) return;
                if (!in_image(r, rows, cols)) { bad = true; return; }
                const size_t o = (size_t) r.row * cols + r.col;
                if (pass == 0) {
                    if (winner[o] < ordinal + 1u) winner[o] = ordinal + 1u;
                    if (starts) (*starts)[ordinal] = start;
                } else if (winner[o] == ordinal + 1u) {
                    rgb[3u * o] = data[r.rgb_at]; rgb[3u * o + 1u] = data[r.rgb_at + 1u]; rgb[3u * o + 2u] = data[r.rgb_at + 2u];
                }
            });
        }
    if (!bad) for (size_t o = 0; o < (size_t) rows * cols; ++o) present[o] = winner[o] != 0u;
    delete[] maps; delete[] tiles; delete[] entry;
    return bad ? -1 : count;
}

} // namespace rpm
