// rt_scene_kernels.h -- Scene.make (Scene.fs:15-28) from hittables in device memory: everything of build_scene and encode_image (rt_scene.h)
// that is proportional to the scene, as kernels (rt_scene_plan.h has the per-item rules, which the host code calls as well; DESIGN.md
// "Scene.make on the device").  The two trees are rt_tree_kernels.h' and rt_walk_kernels.h' own builds; here is what lies around them:
//   check      one pass over the records: the error word (min of index * 8 + reason) and the bounded flag of each
//   partition  Array.partition with order kept on both sides: an exclusive scan of the flags gives a bounded sphere its position, the
//              others theirs behind the bounded ones; Sphere.make's boxes go out by position, with a NaN and a non-finite flag
//   rank       the reference tree's `order` output (the depth-first leaf order) IS the rank table: objToOrig, rankOf, leafBoxes by rank,
//              then prim := rank in the tree
//   depth      every Branch j covers the pre-order range (j, skip[j]): diff[j + 1] += 1, diff[skip[j]] -= 1, and an inclusive scan of
//              diff is the depth of every node -- of any pre-order skip tree, the n-ary tuned ones included
//   place      the stable order by depth (breadth first, pre-order within a level): an LSD radix sort on the depth alone, 8 bits a pass,
//              as many passes as the largest depth needs; within a pass a histogram per tile, one scan over [digit][tile], and a stable
//              scatter (ballot ranks within a wave, wave offsets in LDS, tile offsets from the scan)
//   encode     one thread per node: the node and node32 records; one per object: geo, meta, mat through objToOrig; bmax, the largest
//              radius and the radius flag by integer max on order-preserving bits
//
// No kernel waits for another workgroup: every dependency is a launch boundary on the caller's stream.  Scans are three launches (tile
// sums, one workgroup over the sums, tiles again).  Atomics: integer add (diff, LDS histograms) and integer min / max on order-preserving
// keys, so every output is the same bytes on every run.
#pragma once
#include "rt_scene_plan.h"

#include <hip/hip_runtime.h>

#define RTSK_BLOCK 256
#define RTSK_ITEMS 4
#define RTSK_TILE (RTSK_BLOCK * RTSK_ITEMS) /* elements one workgroup scans, counts or scatters */
#define RTSK_RADIX 256

namespace rtsk {

struct Ctrl { // zeroed in front of a build, `err` to all ones and `bmax_bits` to the bits of 1e-30f
    unsigned long long err;      // min over the refused hittables of index * 8 + reason
    unsigned long long rmax_key; // max over the bounded radii > 0 of their bits (positive doubles order as their bits do)
    uint32_t nan_box, non_finite, bad_radius;
    uint32_t bmax_bits;          // max of the bits of |coordinate| over the node32 boxes (non-negative floats order as their bits do)
    uint32_t max_depth;
    uint32_t pad[7];
};
static_assert(sizeof(Ctrl) == 64, "one 64-byte block");

__device__ static inline uint32_t wave_max(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}
__device__ static inline unsigned long long wave_max64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}
// The exclusive scan of one value per thread over a workgroup of RTSK_BLOCK threads; `total`: the workgroup's sum.  sh: one word per wave.
__device__ static inline uint32_t block_scan(uint32_t v, uint32_t *sh, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off, 64); if ((int) lane >= off) inc += o; }
    __syncthreads(); // (sh may still be read from the call before)
    if (lane == 63u) sh[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (uint32_t k = 0; k < RTSK_BLOCK / 64u; ++k) { const uint32_t s = sh[k]; if (k < w) base += s; total += s; }
    return base + inc - v;
}

// ---- scan of m words, RTSK_TILE to a workgroup (arithmetic modulo 2^32: the depth's differences are signed) ----
__global__ __launch_bounds__(RTSK_BLOCK) void scan_sums_kernel(const uint32_t *a, uint32_t m, uint32_t *sums) {
    __shared__ uint32_t sh[RTSK_BLOCK / 64];
    const uint32_t first = blockIdx.x * RTSK_TILE + threadIdx.x * RTSK_ITEMS;
    uint32_t v = 0;
    for (uint32_t k = 0; k < RTSK_ITEMS; ++k) if (first + k < m) v += a[first + k];
    uint32_t total;
    (void) block_scan(v, sh, total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = total;
}
// one workgroup: sums[0 .. count) becomes its exclusive scan, sums[count] the sum of all
__global__ __launch_bounds__(RTSK_BLOCK) void scan_top_kernel(uint32_t *sums, uint32_t count) {
    __shared__ uint32_t sh[RTSK_BLOCK / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < count; base += RTSK_BLOCK) {
        const uint32_t i = base + threadIdx.x, v = i < count ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan(v, sh, total);
        if (i < count) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0u) sums[count] = carry;
}
// out may be a
__global__ __launch_bounds__(RTSK_BLOCK) void scan_apply_kernel(const uint32_t *a, uint32_t m, const uint32_t *sums, uint32_t *out, int inclusive) {
    __shared__ uint32_t sh[RTSK_BLOCK / 64];
    const uint32_t first = blockIdx.x * RTSK_TILE + threadIdx.x * RTSK_ITEMS;
    uint32_t x[RTSK_ITEMS], v = 0;
    for (uint32_t k = 0; k < RTSK_ITEMS; ++k) { x[k] = first + k < m ? a[first + k] : 0u; v += x[k]; }
    uint32_t total;
    uint32_t run = sums[blockIdx.x] + block_scan(v, sh, total);
    for (uint32_t k = 0; k < RTSK_ITEMS; ++k) {
        if (first + k < m) out[first + k] = inclusive ? run + x[k] : run;
        run += x[k];
    }
}

// ---- check and classify ----
__global__ __launch_bounds__(RTSK_BLOCK) void scene_check_kernel(const rt_hittable *h, uint64_t n, int64_t n_textures, Ctrl *ctrl, uint32_t *flag) {
    // (a grid-stride loop: the count is the caller's, and is refused as too large only after every record has been checked; flag is null then)
    for (uint64_t i = (uint64_t) blockIdx.x * RTSK_BLOCK + threadIdx.x; i < n; i += (uint64_t) gridDim.x * RTSK_BLOCK) {
        const rt_hittable &o = h[i];
        const int why = rts::check_hittable(o, n_textures);
        if (why) atomicMin(&ctrl->err, (unsigned long long) (i * 8u + (uint64_t) why));
        if (flag) flag[i] = rts::is_bounded(o) ? 1u : 0u;
    }
}
// pos: the exclusive scan of flag; n_bounded: its sum (scan_top_kernel's last word).  obj_to_orig gets its unbounded tail here.
__global__ __launch_bounds__(RTSK_BLOCK) void scene_partition_kernel(const rt_hittable *h, uint32_t n, const uint32_t *flag, const uint32_t *pos,
                                                                     const uint32_t *n_bounded, Ctrl *ctrl, int32_t *bounded, double *boxes,
                                                                     int32_t *obj_to_orig) {
    const uint32_t i = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = pos[i];
    if (!flag[i]) { obj_to_orig[*n_bounded + (i - j)] = (int32_t) i; return; }
    bounded[j] = (int32_t) i;
    const rtt::Box b = rts::sphere_box(h[i]);
    bool nan = false, finite = true;
    for (int a = 0; a < 3; ++a) {
        nan = nan || rts::is_nan(b.mn[a]) || rts::is_nan(b.mx[a]);
        finite = finite && rts::is_finite(b.mn[a]) && rts::is_finite(b.mx[a]);
    }
    rtt::store_box(boxes + (size_t) j * 6u, b);
    if (nan) atomicMax(&ctrl->nan_box, 1u);
    if (!finite) atomicMax(&ctrl->non_finite, 1u);
}

// ---- ranks: order[r] = position in `bounded` of the r-th Leaf of the reference tree in pre-order ----
__global__ __launch_bounds__(RTSK_BLOCK) void scene_rank_kernel(uint32_t nb, const int32_t *order, const int32_t *bounded, const double *boxes,
                                                                int32_t *obj_to_orig, int32_t *rank_of, double *leaf_boxes) {
    const uint32_t r = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    if (r >= nb) return;
    const uint32_t j = (uint32_t) order[r];
    obj_to_orig[r] = bounded[j];
    rank_of[j] = (int32_t) r;
    for (int k = 0; k < 6; ++k) leaf_boxes[(size_t) r * 6u + k] = boxes[(size_t) j * 6u + k];
}
// BoundingBoxTree.make over 1 or 2 boxes (BoundingBoxTree.fs:14-21), which sorts nothing: Leaf, or Branch (Leaf 0, Leaf 1, their union).  One thread.
__global__ void scene_small_tree_kernel(uint32_t nb, const double *boxes, int32_t *skip, int32_t *prim, double *node_boxes, int32_t *order) {
    if (blockIdx.x != 0u || threadIdx.x != 0u || nb == 0u || nb > 2u) return;
    const rtt::Box b0 = rtt::load_box(boxes);
    if (nb == 1u) {
        skip[0] = 1; prim[0] = 0; order[0] = 0;
        rtt::store_box(node_boxes, b0);
        return;
    }
    const rtt::Box b1 = rtt::load_box(boxes + 6);
    skip[0] = 3; skip[1] = 2; skip[2] = 3;
    prim[0] = -1; prim[1] = 0; prim[2] = 1;
    order[0] = 0; order[1] = 1;
    rtt::store_box(node_boxes, rtt::merge_two(b0, b1));
    rtt::store_box(node_boxes + 6, b0);
    rtt::store_box(node_boxes + 12, b1);
}
__global__ __launch_bounds__(RTSK_BLOCK) void scene_prim_kernel(uint32_t nn, int32_t *prim, const int32_t *rank_of) {
    const uint32_t i = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    if (i >= nn) return;
    const int32_t p = prim[i];
    if (p >= 0) prim[i] = rank_of[p];
}

// ---- depth: diff is nn + 1 zeroed words ----
__global__ __launch_bounds__(RTSK_BLOCK) void scene_diff_kernel(uint32_t nn, const int32_t *skip, const int32_t *prim, uint32_t *diff) {
    const uint32_t j = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    if (j >= nn || prim[j] >= 0) return;
    const uint32_t end = (uint32_t) skip[j];
    if (end > nn || end <= j) return; // (not a pre-order tree: leave the words alone rather than write outside them)
    atomicAdd(&diff[j + 1u], 1u);
    atomicAdd(&diff[end], 0xFFFFFFFFu);
}

// ---- the stable order by depth: one pass of an LSD radix sort on the digit (key >> shift) & mask, mask <= 255 (the product's passes are
// 8 bits wide; the test hook may ask for narrower ones, so that a tree of a few dozen levels takes several).  hist is [RTSK_RADIX][tiles]. ----
__global__ __launch_bounds__(RTSK_BLOCK) void sort_hist_kernel(const uint32_t *key, uint32_t m, uint32_t shift, uint32_t mask, uint32_t *hist, uint32_t tiles,
                                                               uint32_t *max_key) {
    __shared__ uint32_t cnt[RTSK_RADIX];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t mx = 0;
    for (uint32_t r = 0; r < RTSK_ITEMS; ++r) {
        const uint32_t i = blockIdx.x * RTSK_TILE + r * RTSK_BLOCK + threadIdx.x;
        if (i < m) { const uint32_t k = key[i]; atomicAdd(&cnt[(k >> shift) & mask], 1u); mx = k > mx ? k : mx; }
    }
    __syncthreads();
    hist[(size_t) threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
    if (max_key) {
        mx = wave_max(mx);
        if ((threadIdx.x & 63u) == 0u) atomicMax(max_key, mx);
    }
}
static_assert(RTSK_RADIX == RTSK_BLOCK, "one thread per digit");
// hist: scanned (exclusive, over the whole [digit][tile] array).  idx_in may be null: the identity.
__global__ __launch_bounds__(RTSK_BLOCK) void sort_scatter_kernel(const uint32_t *key_in, const uint32_t *idx_in, uint32_t m, uint32_t shift, uint32_t mask,
                                                                  const uint32_t *hist, uint32_t tiles, uint32_t *key_out, uint32_t *idx_out) {
    __shared__ uint32_t running[RTSK_RADIX];
    __shared__ uint32_t wave_cnt[RTSK_BLOCK / 64][RTSK_RADIX];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    running[threadIdx.x] = hist[(size_t) threadIdx.x * tiles + blockIdx.x];
    for (uint32_t r = 0; r < RTSK_ITEMS; ++r) {
        for (uint32_t k = 0; k < RTSK_BLOCK / 64u; ++k) wave_cnt[k][threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t i = blockIdx.x * RTSK_TILE + r * RTSK_BLOCK + threadIdx.x;
        const bool valid = i < m;
        const uint32_t key = valid ? key_in[i] : 0u, d = (key >> shift) & mask;
        unsigned long long same = __ballot(valid); // the valid lanes of this wave with the same digit
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = ((d >> b) & 1u) != 0u;
            const unsigned long long bal = __ballot(valid && bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t) __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wave_cnt[w][d] = (uint32_t) __popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t at = running[d] + rank;
            for (uint32_t k = 0; k < w; ++k) at += wave_cnt[k][d];
            if (at < m) { // (always, when hist is the scanned histogram of these keys)
                key_out[at] = key;
                idx_out[at] = idx_in ? idx_in[i] : i;
            }
        }
        __syncthreads();
        uint32_t add = 0;
        for (uint32_t k = 0; k < RTSK_BLOCK / 64u; ++k) add += wave_cnt[k][threadIdx.x];
        running[threadIdx.x] += add;
    }
}
// place[idx[k]] = k, place[nn] = nn ("tree exhausted")
__global__ __launch_bounds__(RTSK_BLOCK) void scene_place_kernel(uint32_t nn, const uint32_t *idx, uint32_t *place) {
    const uint32_t k = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    if (k < nn) { const uint32_t i = idx[k]; if (i < nn) place[i] = k; }
    if (k == nn) place[nn] = nn;
}

// ---- encode ----
struct alignas(16) Q16 { uint32_t w[4]; };
template <int N, class T> __device__ static inline void store16(unsigned char *dst, const T &rec) { // dst is 16-byte aligned
    static_assert(sizeof(T) == N * 16, "whole 16-byte words");
    Q16 q[N];
    __builtin_memcpy(q, &rec, sizeof(T));
    for (int k = 0; k < N; ++k) ((Q16 *) dst)[k] = q[k];
}
// box: nn * 6 doubles (minx, maxx, miny, maxy, minz, maxz); node and node32: the two sections of the image
__global__ __launch_bounds__(RTSK_BLOCK) void scene_nodes_kernel(uint32_t nn, uint64_t nobj, const int32_t *skip, const int32_t *prim, const double *box,
                                                                 const uint32_t *place, unsigned char *node, unsigned char *node32, Ctrl *ctrl) {
    const uint32_t i = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    float bm = 1e-30f;
    if (i < nn) {
        const rtt::Box b = rtt::load_box(box + (size_t) i * 6u);
        const int32_t p = prim[i];
        uint32_t end = (uint32_t) skip[i];
        if (end > nn) end = nn; // (place has nn + 1 words)
        const rts::Node32Rec fr = rts::node32_record(b, p, place[i + 1u], place[end], nobj);
        store16<7>(node + (size_t) i * RTD_NODE_BYTES, rts::node_record(b, i, skip[i], p));
        const uint32_t at = place[i];
        if (at < nn) store16<4>(node32 + (size_t) at * RTD_NODE32_BYTES, fr);
        bm = rts::bmax_with(bm, fr);
    }
    uint32_t bits;
    __builtin_memcpy(&bits, &bm, sizeof(bits));
    bits = wave_max(bits);
    if ((threadIdx.x & 63u) == 0u) atomicMax(&ctrl->bmax_bits, bits);
}
static_assert(sizeof(rts::NodeRec) == RTD_NODE_BYTES && sizeof(rts::Node32Rec) == RTD_NODE32_BYTES, "the records of the image");
struct Geo { double v[6]; };
struct Mat { double v[4]; };
__global__ __launch_bounds__(RTSK_BLOCK) void scene_objects_kernel(uint32_t nobj, uint32_t nb, uint64_t n_hittables, const rt_hittable *h, const int32_t *obj_to_orig,
                                                                   unsigned char *geo, unsigned char *meta, unsigned char *mat, Ctrl *ctrl) {
    const uint32_t j = blockIdx.x * RTSK_BLOCK + threadIdx.x;
    unsigned long long rkey = 0ull;
    uint32_t bad = 0u;
    if (j < nobj) {
        const uint64_t orig = (uint64_t) (uint32_t) obj_to_orig[j];
        if (orig < n_hittables) {
            const rt_hittable &o = h[orig];
            const rts::ObjectRec r = rts::object_record(o);
            Geo g; Mat m;
            for (int k = 0; k < 6; ++k) g.v[k] = r.geo[k];
            for (int k = 0; k < 4; ++k) m.v[k] = r.mat[k];
            store16<3>(geo + (size_t) j * 48u, g);
            *(int2 *) (meta + (size_t) j * 8u) = make_int2(r.meta[0], r.meta[1]);
            store16<2>(mat + (size_t) j * 32u, m);
            if (j < nb) {
                const double rad = o.radius;
                if (!rts::radius_ok(rad)) bad = 1u;
                if (rad > 0.0) __builtin_memcpy(&rkey, &rad, sizeof(rkey));
            }
        }
    }
    rkey = wave_max64(rkey);
    bad = wave_max(bad);
    if ((threadIdx.x & 63u) == 0u) {
        if (rkey) atomicMax(&ctrl->rmax_key, rkey);
        if (bad) atomicMax(&ctrl->bad_radius, 1u);
    }
}

} // namespace rtsk
