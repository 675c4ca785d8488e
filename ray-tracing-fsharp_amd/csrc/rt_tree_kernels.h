// rt_tree_kernels.h -- BoundingBoxTree.make's tree (BoundingBoxTree.fs:9-43) built on the device, level by level (rt_tree_plan.h has the
// shape, the key and the comparisons; DESIGN.md "The reference tree on the device").
//
// One array `ids` of box indices; a node is a contiguous segment of it, and `slot` says for every position which segment of the current
// level it is in.  A level with segments above RTT_S boxes is a set of launches over the whole array:
//   fill     one sort record (key of Min[axis], slot, position) per position and axis
//   sort     a bitonic sort of the records by (slot, key, position) -- unique, so any correct sort is the stable sortBy
//   parts    the ordered reduction of each segment's left and right half in each axis' order, RTT_PART boxes per workgroup
//   choose   per segment: the parts put together in order, the three costs, the first minimum, the two children's records
//   reorder  the winning axis' order becomes the next level's, and every position learns its child's slot
// and every segment of at most RTT_S boxes is then finished by ONE workgroup in LDS (tree_lds_kernel), all its remaining levels in one
// launch; for n <= RTT_S that launch is the whole build.
//
// No kernel waits for another workgroup: levels are separated by launch boundaries on the caller's stream, and every loop is bounded by
// the plan.  Every kernel returns at once when the check in front of the build found a NaN coordinate (*bad), so nothing is written then.
#pragma once
#include "rt_tree_plan.h"

#include <hip/hip_runtime.h>

#define RTK_BLOCK 256        /* fill, parts, reorder, steps */
#define RTK_TILE 2048        /* records one workgroup sorts in LDS (32 KiB; the compiler adds 16 KiB: it keeps the exchange's temporary there) */
#define RTK_TILE_THREADS 1024
#define RTK_LDS_THREADS 512  /* tree_lds_kernel: 8 waves, one segment per wave at a time */

namespace rtk {

struct alignas(16) Rec { uint64_t key; uint32_t slot, pos; };
__device__ static inline bool rec_less(const Rec &a, const Rec &b) {
    if (a.slot != b.slot) return a.slot < b.slot;
    if (a.key != b.key) return a.key < b.key;
    return a.pos < b.pos;
}

// ---- ordered reductions ------------------------------------------------------------------------------------------------
struct RBox { rtt::Box b; int has; };
__device__ static inline RBox comb(const RBox &a, const RBox &b) { // a: the earlier operand
    if (!a.has) return b;
    if (!b.has) return a;
    RBox o;
    o.b = rtt::merge_two(a.b, b.b);
    o.has = 1;
    return o;
}
// lane 0 ends with lanes 0..63 reduced in lane order (after the step `off`, lane i holds lanes [i, i + 2*off)); wave-uniform callers only
__device__ static inline RBox wave_reduce(RBox v) {
    const int lane = (int) (threadIdx.x & 63u);
    for (int off = 1; off < 64; off <<= 1) {
        RBox o;
        for (int a = 0; a < 3; ++a) { o.b.mn[a] = __shfl_down(v.b.mn[a], off, 64); o.b.mx[a] = __shfl_down(v.b.mx[a], off, 64); }
        o.has = __shfl_down(v.has, off, 64);
        if (lane + off >= 64) o.has = 0;
        v = comb(v, o);
    }
    return v;
}
// the boxes fetch(q), q in [lo, hi), reduced in order by one wave: each lane a contiguous run, then wave_reduce
template <class Fetch> __device__ static inline RBox wave_range(uint32_t lo, uint32_t hi, const double *boxes, Fetch fetch) {
    const uint32_t lane = threadIdx.x & 63u, len = hi > lo ? hi - lo : 0u, per = (len + 63u) / 64u;
    const uint32_t a = lo + lane * per, e = a + per < hi ? a + per : hi;
    RBox v;
    v.has = 0;
    for (uint32_t q = a; q < e; ++q) {
        const rtt::Box x = rtt::load_box(boxes + (size_t) fetch(q) * 6u);
        if (v.has) v.b = rtt::merge_two(v.b, x); else { v.b = x; v.has = 1; }
    }
    return wave_reduce(v);
}
// the same by a workgroup of `waves` waves (<= 16): wave w takes the w-th run; thread 0 returns the result (`sh`: `waves` RBox in LDS)
template <class Fetch> __device__ static inline RBox block_range(uint32_t lo, uint32_t hi, const double *boxes, Fetch fetch, RBox *sh) {
    const uint32_t waves = blockDim.x / 64u, w = threadIdx.x / 64u, len = hi > lo ? hi - lo : 0u, per = (len + waves - 1u) / waves;
    const uint32_t a = lo + w * per < hi ? lo + w * per : hi, e = a + per < hi ? a + per : hi;
    const RBox r = wave_range(a, e, boxes, fetch);
    if ((threadIdx.x & 63u) == 0u) sh[w] = r;
    __syncthreads();
    RBox acc;
    acc.has = 0;
    if (threadIdx.x == 0u) for (uint32_t k = 0; k < waves; ++k) acc = comb(acc, sh[k]);
    __syncthreads();
    return acc;
}

struct Outputs { int32_t *skip, *prim; double *boxes; int32_t *order; }; // any may be null
__device__ static inline void write_node(const Outputs &o, uint32_t node, uint32_t skip, int32_t prim, const rtt::Box &b) {
    if (o.skip) o.skip[node] = (int32_t) skip;
    if (o.prim) o.prim[node] = prim;
    if (o.boxes) rtt::store_box(o.boxes + (size_t) node * 6u, b);
}

// ---- the check in front of the build ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(RTK_BLOCK) void tree_check_kernel(const double *boxes, uint64_t count, int *bad) {
    int found = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * RTK_BLOCK + threadIdx.x; i < count; i += (uint64_t) gridDim.x * RTK_BLOCK) {
        const double v = boxes[i];
        if (v != v) found = 1;
    }
    if (found) atomicOr(bad, 1);
}

// ---- global levels ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RTK_BLOCK) void tree_init_kernel(uint32_t n, uint32_t *ids, uint32_t *slot, const int *bad) {
    if (*bad) return;
    const uint32_t p = blockIdx.x * RTK_BLOCK + threadIdx.x;
    if (p < n) { ids[p] = p; slot[p] = 0u; }
}
// the root's box: the input order reduced left to right, RTT_PART boxes per workgroup
__global__ __launch_bounds__(RTK_BLOCK) void tree_root_parts_kernel(uint32_t n, const double *boxes, rtt::Box *partial, const int *bad) {
    __shared__ RBox sh[RTK_BLOCK / 64];
    if (*bad) return;
    const uint32_t lo = blockIdx.x * (uint32_t) RTT_PART, hi = lo + RTT_PART < n ? lo + RTT_PART : n;
    const RBox r = block_range(lo, hi, boxes, [](uint32_t q) { return q; }, sh);
    if (threadIdx.x == 0u) partial[blockIdx.x] = r.b;
}
__global__ void tree_root_finish_kernel(uint32_t n, uint32_t nparts, const rtt::Box *partial, Outputs out, const int *bad) {
    if (*bad || threadIdx.x != 0u || blockIdx.x != 0u) return;
    rtt::Box acc = partial[0];
    for (uint32_t z = 1; z < nparts; ++z) acc = rtt::merge_two(acc, partial[z]);
    write_node(out, 0u, 2u * n - 1u, -1, acc);
}

__global__ __launch_bounds__(RTK_BLOCK) void tree_fill_kernel(uint32_t n, uint32_t P, const uint32_t *ids, const uint32_t *slot, const double *boxes, Rec *rec,
                                                              const int *bad) {
    if (*bad) return;
    const uint32_t i = blockIdx.x * RTK_BLOCK + threadIdx.x;
    if (i >= P) return;
    if (i < n) {
        const double *b = boxes + (size_t) ids[i] * 6u;
        const uint32_t s = slot[i];
        for (int a = 0; a < 3; ++a) rec[(size_t) a * P + i] = Rec{rtt::key_of(b[a * 2]), s, i};
    } else
        for (int a = 0; a < 3; ++a) rec[(size_t) a * P + i] = Rec{~0ull, 0xFFFFFFFFu, i}; // padding: behind every segment
}

// Bitonic sort, ascending, of P records (a power of two >= RTK_TILE) per axis (blockIdx.y).  The steps with a stride below the tile run in
// LDS: tree_sort_tile_kernel does every (k, j) with k in [k_lo, k_hi] and j < RTK_TILE; tree_sort_step_kernel is one (k, j) with j >= RTK_TILE.
__device__ static inline void cmp_swap(Rec &x, Rec &y, bool ascending) { // x at the lower index
    if (rec_less(y, x) == ascending) { const Rec t = x; x = y; y = t; }
}
__global__ __launch_bounds__(RTK_TILE_THREADS) void tree_sort_tile_kernel(Rec *rec, uint32_t P, uint32_t k_lo, uint32_t k_hi, const int *bad) {
    __shared__ Rec sh[RTK_TILE];
    if (*bad) return;
    Rec *base = rec + (size_t) blockIdx.y * P + (size_t) blockIdx.x * RTK_TILE;
    const uint32_t t = threadIdx.x, g0 = blockIdx.x * (uint32_t) RTK_TILE;
    sh[t] = base[t];
    sh[t + RTK_TILE_THREADS] = base[t + RTK_TILE_THREADS];
    __syncthreads();
    for (uint32_t k = k_lo; k <= k_hi; k <<= 1) {
        for (uint32_t j = (k >> 1) < (uint32_t) (RTK_TILE / 2) ? (k >> 1) : (uint32_t) (RTK_TILE / 2); j > 0u; j >>= 1) {
            const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
            cmp_swap(sh[i], sh[i | j], ((g0 + i) & k) == 0u);
            __syncthreads();
        }
    }
    base[t] = sh[t];
    base[t + RTK_TILE_THREADS] = sh[t + RTK_TILE_THREADS];
}
__global__ __launch_bounds__(RTK_BLOCK) void tree_sort_step_kernel(Rec *rec, uint32_t P, uint32_t k, uint32_t j, const int *bad) {
    if (*bad) return;
    const uint32_t t = blockIdx.x * RTK_BLOCK + threadIdx.x;
    if (t >= P / 2u) return;
    Rec *base = rec + (size_t) blockIdx.y * P;
    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
    Rec x = base[i], y = base[i | j];
    if (rec_less(y, x) == (((i & k) == 0u))) { base[i] = y; base[i | j] = x; }
}

// the box index at place q of an axis' sorted order (a record that is not a position -- padding -- cannot be there after a sort)
__device__ static inline uint32_t sorted_id(const uint32_t *ids, const Rec *rec, uint32_t q, uint32_t n) {
    const uint32_t p = rec[q].pos;
    return ids[p < n ? p : 0u];
}

// blockIdx.x = slot * nparts + part, blockIdx.y = axis * 2 + half
__global__ __launch_bounds__(RTK_BLOCK) void tree_parts_kernel(uint32_t n, uint32_t P, int32_t level, uint32_t nparts, const uint32_t *ids, const Rec *rec,
                                                               const double *boxes, rtt::Box *partial, const int *bad) {
    __shared__ RBox sh[RTK_BLOCK / 64];
    if (*bad) return;
    const uint32_t s = blockIdx.x / nparts, z = blockIdx.x % nparts, y = blockIdx.y;
    const rtt::Segment seg = rtt::segment(n, level, s);
    if (seg.count < 3u || seg.level != level) return;
    const uint32_t nl = rtt::left_count(seg.count);
    const uint32_t lo0 = (y & 1u) ? seg.start + nl : seg.start, hi0 = (y & 1u) ? seg.start + seg.count : seg.start + nl;
    const uint32_t lo = lo0 + z * (uint32_t) RTT_PART;
    if (lo >= hi0) return;
    const uint32_t hi = lo + RTT_PART < hi0 ? lo + RTT_PART : hi0;
    const Rec *r = rec + (size_t) (y >> 1) * P;
    const RBox v = block_range(lo, hi, boxes, [=](uint32_t q) { return sorted_id(ids, r, q, n); }, sh);
    if (threadIdx.x == 0u) partial[((size_t) s * 6u + y) * nparts + z] = v.b;
}

// one thread per slot of the level
__global__ __launch_bounds__(RTK_BLOCK) void tree_choose_kernel(uint32_t n, uint32_t P, int32_t level, uint32_t nparts, const uint32_t *ids, const Rec *rec,
                                                                const double *boxes, const rtt::Box *partial, uint32_t *slot_best, Outputs out, const int *bad) {
    if (*bad) return;
    const uint32_t s = blockIdx.x * RTK_BLOCK + threadIdx.x;
    if (s >= (1u << level)) return;
    const rtt::Segment seg = rtt::segment(n, level, s);
    if (seg.count < 2u || seg.level != level) return; // no such slot, or a Leaf (its record is its parent's to write)
    const uint32_t nl = rtt::left_count(seg.count), nr = seg.count - nl;
    const uint32_t ln = seg.node + 1u, rn = seg.node + 2u * nl;
    if (seg.count == 2u) { // Branch (Leaf boxes.[0], Leaf boxes.[1], boundAll): no sort
        const uint32_t a = ids[seg.start], b = ids[seg.start + 1u];
        write_node(out, ln, ln + 1u, (int32_t) a, rtt::load_box(boxes + (size_t) a * 6u));
        write_node(out, rn, rn + 1u, (int32_t) b, rtt::load_box(boxes + (size_t) b * 6u));
        return;
    }
    double c[3];
    rtt::Box L[3], R[3];
    for (uint32_t y = 0; y < 6u; ++y) {
        const uint32_t len = (y & 1u) ? nr : nl, parts = (len + RTT_PART - 1u) / RTT_PART;
        const rtt::Box *p = partial + ((size_t) s * 6u + y) * nparts;
        rtt::Box acc = p[0];
        for (uint32_t z = 1; z < parts; ++z) acc = rtt::merge_two(acc, p[z]);
        if (y & 1u) R[y >> 1] = acc; else L[y >> 1] = acc;
    }
    for (int a = 0; a < 3; ++a) c[a] = rtt::cost(L[a], R[a]);
    const int best = rtt::best_axis(c);
    slot_best[s] = (uint32_t) best;
    const Rec *r = rec + (size_t) best * P;
    write_node(out, ln, ln + 2u * nl - 1u, nl == 1u ? (int32_t) sorted_id(ids, r, seg.start, n) : -1, best == 0 ? L[0] : best == 1 ? L[1] : L[2]);
    write_node(out, rn, rn + 2u * nr - 1u, nr == 1u ? (int32_t) sorted_id(ids, r, seg.start + nl, n) : -1, best == 0 ? R[0] : best == 1 ? R[1] : R[2]);
}

__global__ __launch_bounds__(RTK_BLOCK) void tree_reorder_kernel(uint32_t n, uint32_t P, int32_t level, const uint32_t *ids_in, uint32_t *ids_out, uint32_t *slot,
                                                                 const Rec *rec, const uint32_t *slot_best, const int *bad) {
    if (*bad) return;
    const uint32_t p = blockIdx.x * RTK_BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = slot[p];
    const rtt::Segment seg = rtt::segment(n, level, s);
    uint32_t id = ids_in[p], child = 2u * s;
    if (seg.level == level && seg.count >= 2u) {
        const uint32_t nl = rtt::left_count(seg.count);
        if (seg.count >= 3u) id = sorted_id(ids_in, rec + (size_t) slot_best[s] * P, p, n);
        child += (p - seg.start >= nl) ? 1u : 0u;
    }
    ids_out[p] = id;
    slot[p] = child;
}

// ---- a segment of at most RTT_S boxes, all its levels, by one workgroup in LDS ---------------------------------------------------
// blockIdx.x: the slot of `level0` (0 and one workgroup when n <= RTT_S: the whole build, the root's record included; `ids` null then).
__global__ __launch_bounds__(RTK_LDS_THREADS) void tree_lds_kernel(uint32_t n, int32_t level0, const uint32_t *ids, const double *boxes, Outputs out, const int *bad) {
    __shared__ uint64_t key[RTT_S];
    __shared__ uint32_t tag[RTT_S]; // local slot << 11 | position
    __shared__ uint16_t ord[3][RTT_S];
    __shared__ uint32_t idbuf[2][RTT_S];
    __shared__ uint16_t lslot[RTT_S];
    __shared__ RBox wres[RTK_LDS_THREADS / 64];
    if (*bad) return;
    const rtt::Segment top = rtt::segment(n, level0, blockIdx.x);
    const uint32_t c0 = top.count, tid = threadIdx.x;
    if (c0 == 0u || c0 > (uint32_t) RTT_S) return; // (no such slot; the second cannot be: the host launches this at levels_above(n, RTT_S))
    uint32_t *cur = idbuf[0], *nxt = idbuf[1];
    for (uint32_t q = tid; q < c0; q += RTK_LDS_THREADS) { cur[q] = ids ? ids[top.start + q] : q; lslot[q] = 0; }
    __syncthreads();
    if (level0 == 0) {
        const RBox r = block_range(0u, c0, boxes, [=](uint32_t q) { return cur[q]; }, wres);
        if (tid == 0u) write_node(out, 0u, 2u * c0 - 1u, c0 == 1u ? (int32_t) cur[0] : -1, r.b);
    }
    uint32_t Pc = 2u;
    while (Pc < c0) Pc <<= 1;
    const int32_t D = top.level == level0 ? rtt::depth(c0) : 1; // (a Leaf that ended above level0 has nothing below it)
    for (int32_t l = 0; l + 1 < D; ++l) {
        for (int a = 0; a < 3; ++a) {
            for (uint32_t i = tid; i < Pc; i += RTK_LDS_THREADS) {
                if (i < c0) { key[i] = rtt::key_of(boxes[(size_t) cur[i] * 6u + (size_t) a * 2u]); tag[i] = ((uint32_t) lslot[i] << 11) | i; }
                else { key[i] = ~0ull; tag[i] = 0xFFFFF800u | i; }
            }
            __syncthreads();
            for (uint32_t k = 2u; k <= Pc; k <<= 1)
                for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
                    for (uint32_t t = tid; t < Pc / 2u; t += RTK_LDS_THREADS) {
                        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), m = i | j;
                        const uint32_t si = tag[i] >> 11, sm = tag[m] >> 11;
                        const bool less = sm != si ? sm < si : key[m] != key[i] ? key[m] < key[i] : tag[m] < tag[i]; // record m < record i
                        if (less == ((i & k) == 0u)) {
                            const uint64_t tk = key[i]; key[i] = key[m]; key[m] = tk;
                            const uint32_t tt = tag[i]; tag[i] = tag[m]; tag[m] = tt;
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t q = tid; q < c0; q += RTK_LDS_THREADS) { const uint32_t p = tag[q] & 2047u; ord[a][q] = (uint16_t) (p < c0 ? p : 0u); } // (padding sorts behind every position)
            __syncthreads();
        }
        // what no split touches keeps its place and goes left
        for (uint32_t q = tid; q < c0; q += RTK_LDS_THREADS) { nxt[q] = cur[q]; lslot[q] = (uint16_t) (2u * lslot[q]); }
        __syncthreads();
        const uint32_t lane = tid & 63u;
        for (uint32_t s = tid / 64u; s < (1u << l); s += RTK_LDS_THREADS / 64u) { // one wave per segment of the level
            const rtt::Segment seg = rtt::segment(c0, l, s);
            if (seg.count < 2u || seg.level != l) continue;
            const uint32_t nl = rtt::left_count(seg.count), nr = seg.count - nl;
            const uint32_t ln = top.node + seg.node + 1u, rn = top.node + seg.node + 2u * nl;
            if (seg.count == 2u) {
                if (lane < 2u) {
                    const uint32_t id = cur[seg.start + lane], node = lane ? rn : ln;
                    write_node(out, node, node + 1u, (int32_t) id, rtt::load_box(boxes + (size_t) id * 6u));
                    lslot[seg.start + lane] = (uint16_t) (2u * s + lane);
                }
                continue;
            }
            int best = 0;
            double bestCost = 0.0;
            rtt::Box bl{}, br{};
            for (int a = 0; a < 3; ++a) {
                const uint16_t *o = ord[a];
                const RBox L = wave_range(seg.start, seg.start + nl, boxes, [=](uint32_t q) { return cur[o[q]]; });
                const RBox R = wave_range(seg.start + nl, seg.start + seg.count, boxes, [=](uint32_t q) { return cur[o[q]]; });
                const double c = rtt::cost(L.b, R.b); // (lane 0's is the segment's)
                if (a == 0 || c < bestCost) { best = a; bestCost = c; bl = L.b; br = R.b; } // the first strict minimum; NaN is never `<`
            }
            best = __shfl(best, 0, 64);
            const uint16_t *o = ord[best];
            if (lane == 0u) {
                write_node(out, ln, ln + 2u * nl - 1u, nl == 1u ? (int32_t) cur[o[seg.start]] : -1, bl);
                write_node(out, rn, rn + 2u * nr - 1u, nr == 1u ? (int32_t) cur[o[seg.start + nl]] : -1, br);
            }
            for (uint32_t q = seg.start + lane; q < seg.start + seg.count; q += 64u) {
                nxt[q] = cur[o[q]];
                lslot[q] = (uint16_t) (2u * s + (q - seg.start >= nl ? 1u : 0u));
            }
        }
        __syncthreads();
        uint32_t *t = cur; cur = nxt; nxt = t;
    }
    if (out.order) for (uint32_t q = tid; q < c0; q += RTK_LDS_THREADS) out.order[top.start + q] = (int32_t) cur[q];
}

} // namespace rtk
