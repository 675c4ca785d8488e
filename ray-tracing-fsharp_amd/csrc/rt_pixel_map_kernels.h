// rt_pixel_map_kernels.h -- ImageOutput.readPixelMap (ImageOutput.fs:46-113) on the device, the list of the pixels a presence map lacks,
// and the scatter of a rendered pixel list into a frame.  The automaton, its maps and who owns a record are rt_pixel_map.h's; the byte
// staging, the block scan of numbers and the one-workgroup scan of tile counts are rt_output.h's.  DESIGN.md "Resuming from a pixel map".
//
// The parse is five launches on the caller's stream, and NO workgroup ever waits for another:
//   parse_maps_kernel         one workgroup per tile of RPM_TILE_BYTES: every thread's chunk as a map, composed over the tile
//   parse_scan_kernel         ONE workgroup: the exclusive scan of the tile maps, in trips of RPM_SCAN_THREADS with the running (state,
//                             ordinal) in that workgroup's own registers; stores every tile's entry and the record count
//   parse_records_kernel<0>   one workgroup per tile: the chunk maps again, scanned inside the tile, so every thread knows the state and
//                             the record ordinal it enters its chunk with; it walks its chunk and reads the records it owns.  A record
//                             outside the image raises ParseHead::bad; every other one claims its pixel with atomicMax(ordinal + 1), so
//                             the LAST record in file order wins whatever the scheduling
//   parse_records_kernel<1>   the same walk; nothing at all when `bad` is set, else the record whose ordinal won stores its three bytes
//   parse_finish_kernel       present = (the pixel has a winner), in full, unless `bad`; d_count
// d_data, d_rgb and d_present may have any byte alignment.  Every store is indexed by a row and a column that were checked against the
// image (digit runs saturate, rpm::push_digit), and every read of the data by a position below n.
#pragma once

#include "rt_output.h"
#include "rt_pixel_map.h"

#include <hip/hip_runtime.h>

namespace rpm {

// Head of a parse's or a scatter's stream-ordered scratch, zeroed before the first launch; one word per pixel (`winner`) follows.
struct ParseHead {
    long long count;  // complete records, duplicates included
    unsigned int bad; // a complete record names a pixel outside the image (a scatter: a list entry outside the frame): nothing is written
    unsigned int pad;
    unsigned int pad2[4];
};
static_assert(sizeof(ParseHead) == RPM_HEAD_BYTES, "the winner words follow the head");

__device__ inline Map shfl_up_map(const Map &m, int d) {
    Map o;
    o.st = __shfl_up(m.st, d, 64);
    for (int s = 0; s < (int) STATES; ++s) o.cnt[s] = __shfl_up(m.cnt[s], d, 64);
    return o;
}
// Exclusive scan (by composition, in thread order) of one map per thread over the workgroup; `total` = all of them composed.
// wave_tot: LDS, BLOCK / 64 entries, free again on return.
template <int BLOCK> __device__ inline Map block_exclusive_scan_maps(const Map &v, Map *wave_tot, Map &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Map inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const Map o = shfl_up_map(inc, d);
        if (lane >= (uint32_t) d) inc = compose(o, inc);
    }
    if (lane == 63u) wave_tot[wave] = inc;
    __syncthreads();
    Map base = identity(), tot = identity();
    for (uint32_t w = 0; w < (uint32_t) (BLOCK / 64); ++w) {
        const Map x = wave_tot[w];
        if (w < wave) base = compose(base, x);
        tot = compose(tot, x);
    }
    total = tot;
    __syncthreads();
    const Map before = shfl_up_map(inc, 1);
    return lane == 0u ? base : compose(base, before);
}

// What the per-tile kernels start with: the tile's bytes staged into `in` (LDS), then this thread's chunk: where it is in LDS, its first
// byte's position in the data, and its length (0 behind the data's end).
__device__ inline const uint8_t *thread_chunk(const uint8_t *data, uint32_t n, uint32_t *in, uint32_t &begin, uint32_t &len) {
    const uint32_t t0 = blockIdx.x * (uint32_t) RPM_TILE_BYTES, cnt = n - t0 < (uint32_t) RPM_TILE_BYTES ? n - t0 : (uint32_t) RPM_TILE_BYTES;
    const uint8_t *src = data + t0;
    const uint32_t a = (uint32_t) ((uintptr_t) src & 3u);
    rto::stage_in((unsigned char *) in, src, cnt, a);
    __syncthreads();
    const uint32_t off = threadIdx.x * (uint32_t) RPM_CHUNK_BYTES;
    len = off < cnt ? (cnt - off < (uint32_t) RPM_CHUNK_BYTES ? cnt - off : (uint32_t) RPM_CHUNK_BYTES) : 0u;
    begin = t0 + off;
    return (const uint8_t *) in + a + off;
}

__global__ __launch_bounds__(RPM_BLOCK) void parse_maps_kernel(const uint8_t *data, uint32_t n, Map *tiles) {
    __shared__ uint32_t in[RPM_TILE_BYTES / 4 + 1];
    __shared__ Map wave_tot[RPM_BLOCK / 64];
    uint32_t begin, len;
    const uint8_t *chunk = thread_chunk(data, n, in, begin, len);
    Map total;
    (void) block_exclusive_scan_maps<RPM_BLOCK>(run_map(chunk, len), wave_tot, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// entries[i]: the (state, ordinal) in front of tile i's first byte.  ONE workgroup; more tiles than it has threads are walked in trips,
// where the walk stands in `carry` -- every thread keeps the same copy in registers.
__global__ __launch_bounds__(RPM_SCAN_THREADS) void parse_scan_kernel(const Map *tiles, uint32_t n_tiles, Entry *entries, ParseHead *head) {
    __shared__ Map wave_tot[RPM_SCAN_THREADS / 64];
    Entry carry{0u, 0u};
    for (uint32_t base = 0; base < n_tiles; base += (uint32_t) RPM_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const Map v = i < n_tiles ? tiles[i] : identity();
        Map trip;
        const Map before = block_exclusive_scan_maps<RPM_SCAN_THREADS>(v, wave_tot, trip);
        if (i < n_tiles) entries[i] = advance(carry, before);
        carry = advance(carry, trip);
    }
    if (threadIdx.x == 0) head->count = (long long) carry.ordinal;
}

template <bool STORE>
__global__ __launch_bounds__(RPM_BLOCK) void parse_records_kernel(const uint8_t *data, uint32_t n, uint32_t rows, uint32_t cols, const Entry *entries, ParseHead *head,
                                                                  unsigned int *winner, uint8_t *rgb) {
    __shared__ uint32_t in[RPM_TILE_BYTES / 4 + 1];
    __shared__ Map wave_tot[RPM_BLOCK / 64];
    if (STORE && head->bad) return; // the same word for every thread of every workgroup
    uint32_t begin, len;
    const uint8_t *chunk = thread_chunk(data, n, in, begin, len);
    Map total;
    const Map before = block_exclusive_scan_maps<RPM_BLOCK>(run_map(chunk, len), wave_tot, total);
    if (len == 0u) return;
    for_owned_records(chunk, (size_t) begin, (size_t) begin + len, advance(entries[blockIdx.x], before), [&](size_t start, uint32_t ordinal) {
        Record r;
        if (!read_record(data, (size_t) n, start, r)) return; // the truncated tail
        if (!in_image(r, rows, cols)) {
            if (!STORE) atomicOr(&head->bad, 1u);
            return;
        }
        const size_t o = (size_t) r.row * cols + r.col;
        if (!STORE) {
            atomicMax(&winner[o], ordinal + 1u);
        } else if (winner[o] == ordinal + 1u) {
            rgb[3u * o] = data[r.rgb_at]; rgb[3u * o + 1u] = data[r.rgb_at + 1u]; rgb[3u * o + 2u] = data[r.rgb_at + 2u];
        }
    });
}

// present in full (unless the map is malformed), and the count -- or the negated status -- for the caller on the device
__global__ __launch_bounds__(RPM_BLOCK) void parse_finish_kernel(const ParseHead *head, const unsigned int *winner, uint32_t npx, uint8_t *present, long long *d_count,
                                                                 long long bad_status) {
    const unsigned int bad = head->bad;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (tid == 0u && d_count) *d_count = bad ? bad_status : head->count;
    if (bad) return;
    for (uint32_t i = tid; i < npx; i += step) present[i] = winner[i] != 0u ? 1 : 0;
}

// ---- the pixels a presence map lacks: a compaction by the same three steps as rt_output.h's formats ----

// This thread's RPM_CHUNK_BYTES presence bytes as a mask of the ABSENT ones (bit k: pixel begin + k)
__device__ inline uint32_t absent_mask(const uint8_t *chunk, uint32_t len) {
    uint32_t m = 0u;
    for (uint32_t k = 0; k < len; ++k) m |= (chunk[k] == 0 ? 1u : 0u) << k;
    return m;
}
__global__ __launch_bounds__(RPM_BLOCK) void missing_sums_kernel(const uint8_t *present, uint32_t npx, unsigned long long *tiles) {
    __shared__ uint32_t in[RPM_TILE_BYTES / 4 + 1];
    __shared__ uint32_t wave_tot[RPM_BLOCK / 64];
    uint32_t begin, len, total;
    const uint8_t *chunk = thread_chunk(present, npx, in, begin, len);
    (void) rto::block_exclusive_scan<uint32_t, RPM_BLOCK>((uint32_t) __popc(absent_mask(chunk, len)), wave_tot, total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}
// tiles[i]: the list position of tile i's first absent pixel (rto::format_scan_kernel, which also decided whether the list fits)
__global__ __launch_bounds__(RPM_BLOCK) void missing_scatter_kernel(const uint8_t *present, uint32_t npx, const unsigned long long *tiles, const rto::FormatScratch *head,
                                                                    int32_t *pixels) {
    __shared__ uint32_t in[RPM_TILE_BYTES / 4 + 1];
    __shared__ uint32_t wave_tot[RPM_BLOCK / 64];
    if (!head->go) return;
    uint32_t begin, len, total;
    const uint8_t *chunk = thread_chunk(present, npx, in, begin, len);
    const uint32_t mask = absent_mask(chunk, len);
    int32_t *dst = pixels + tiles[blockIdx.x] + rto::block_exclusive_scan<uint32_t, RPM_BLOCK>((uint32_t) __popc(mask), wave_tot, total);
    for (uint32_t k = 0; k < len; ++k)
        if ((mask >> k) & 1u) *dst++ = (int32_t) (begin + k);
}

// ---- frame[pixels[i]] = list[i]: an entry outside the frame is found in front of the store; of duplicates the LAST in list order wins ----
__global__ __launch_bounds__(RPM_BLOCK) void scatter_claim_kernel(uint32_t n, const int32_t *pixels, uint32_t npx, ParseHead *head, unsigned int *winner) {
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t p = (uint32_t) pixels[i];
        if (p >= npx) atomicOr(&head->bad, 1u); // (a negative entry too)
        else atomicMax(&winner[p], i + 1u);
    }
}
__global__ __launch_bounds__(RPM_BLOCK) void scatter_store_kernel(uint32_t n, const int32_t *pixels, const uint8_t *list, const ParseHead *head, const unsigned int *winner,
                                                                  uint8_t *frame) {
    if (head->bad) return;
    const uint32_t step = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const size_t p = (size_t) (uint32_t) pixels[i];
        if (winner[p] != i + 1u) continue;
        frame[3u * p] = list[3u * (size_t) i]; frame[3u * p + 1u] = list[3u * (size_t) i + 1u]; frame[3u * p + 2u] = list[3u * (size_t) i + 2u];
    }
}

} // namespace rpm
