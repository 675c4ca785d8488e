// rt_walk_kernels.h -- the surface-area build of the tree the device walks (rt_scene.h SahBuilder without probe rays), on the device, node
// for node (rt_walk_plan.h has the rules; DESIGN.md "The walk tree on the device").
//
// One array `ids` of box indices, double-buffered; a node is a contiguous segment of it.  The shape depends on the boxes, so segments are
// records (start, count, node, depth) in lists the kernels append to:
//   segments above RTW_SWEEP boxes, level by level (the host reads two counters per level: how many there are and the largest):
//     bounds     per segment and axis the least and greatest centroid, as order-preserving keys (atomicMin / atomicMax are free of order)
//     bins       3 x RTW_BINS bin boxes and counts per segment: partials in LDS, combined with the same atomics
//     choose     one thread per segment: rtw::bin_choose, the very function SahBuilder calls; no winner or depth >= RTW_DEPTH: the median arm
//     select     the median arm only: the (key, id) of rank n/2 on axis 0 by an 11-digit radix select, one workgroup per such segment
//     partition  the two SETS into the other buffer (the order inside a set is not defined -- on the host it is std::nth_element's -- and
//                nothing below depends on it: the bins are order-free and a sweep sorts by the unique (key, id)); the children's boxes
//     emit       the two children's records; a child above RTW_SWEEP joins the next level, one of 2..RTW_SWEEP the list of subtrees
//   segments of at most RTW_SWEEP boxes: walk_subtree_kernel, ONE workgroup per segment with the whole subtree in LDS (144 KiB of the
//   CU's 160) for all its remaining levels: three sorts by (key, id) once, then per level and segment the suffix and prefix areas, the
//   costs and the first minimum in (axis, i) order by one wave, and a stable partition of the three orders by the whole workgroup.
// No arm is handed back to the host: the median arm above RTW_SWEEP is the select kernel.
//
// Branch boxes are written with +0.0 for either zero (keys canonicalise it), Leaf boxes as they came in: the sign of a zero in a union
// depends on the merge order, which the host leaves to std::nth_element above RTW_SWEEP; no cost, comparison or split depends on it.
// Two builds of one input therefore give the same bytes, whatever order the atomics land in.
//
// No kernel waits for another workgroup: levels are launch boundaries on the caller's stream, and every loop is bounded by the plan
// (rtw::levels_below).  Every kernel returns at once when the check in front found a non-finite coordinate (*bad): nothing is written then.
//
// Measured on one MI355X against the host builder (same section; profiles/r24/walk_tree_measure.json): 1.32 ms instead of 0.43 ms
// at 485 boxes, 6.8 instead of 13.4 ms at 1e4, 9.2 instead of 160 ms at 1e5 and 17.7 ms instead of 1.83 s at 1e6, where creating the scene
// goes from 1.98 s to 0.51 s.  The crossover is at about 8000 boxes: below it the host route is faster (at 4096 boxes ONE workgroup builds
// the whole tree in 10 ms against 5.9 ms on the host).  Nothing switches the defaults.
#pragma once
#include "rt_walk_plan.h"
#include "rt_tree_kernels.h"

#define RTWK_BLOCK 256
#define RTWK_PART 4096         /* positions of a segment one workgroup of a level kernel takes: 16 per thread */
#define RTWK_PER (RTWK_PART / RTWK_BLOCK)
#define RTWK_SUB_THREADS 1024  /* walk_subtree_kernel: 16 waves */
#define RTWK_SELECT_THREADS 1024

namespace rtwk {

typedef unsigned long long u64;
using rtk::Outputs;
using rtk::RBox;
using rtk::comb;
using rtk::write_node;

struct Seg { uint32_t start, count, node, dbuf; }; // dbuf: depth | (buffer of `ids` the segment is in) << 8
struct Ctrl { int bad; uint32_t nbig[2], maxcount[2], nsmall; uint32_t pad[2]; };
struct Dec { int32_t mode, axis, b; uint32_t k; double lo, scale; u64 pkey; uint32_t pid, pad; }; // mode 0: bins below b on axis; 1: (key, id) below the pivot

// Per segment of a level, set to all ones / to zero before the level (two memsets)
struct Ones { u64 lo[3]; u64 binmn[3][RTW_BINS][3]; u64 cmn[2][3]; };
struct Zeros { u64 hi[3]; u64 binmx[3][RTW_BINS][3]; u64 cmx[2][3]; uint32_t bincnt[3][RTW_BINS]; uint32_t cursor[2]; };

__device__ static inline rtt::Box canon(const rtt::Box &b) { // +0.0 for either zero
    rtt::Box o;
    for (int a = 0; a < 3; ++a) { o.mn[a] = b.mn[a] == 0.0 ? 0.0 : b.mn[a]; o.mx[a] = b.mx[a] == 0.0 ? 0.0 : b.mx[a]; }
    return o;
}

// ---- the check in front of the build: a scene never builds this tree over non-finite boxes ------------------------------------------
__global__ __launch_bounds__(RTWK_BLOCK) void walk_check_kernel(const double *boxes, uint64_t count, int *bad) {
    int found = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * RTWK_BLOCK + threadIdx.x; i < count; i += (uint64_t) gridDim.x * RTWK_BLOCK) {
        const double v = boxes[i];
        if (!(v - v == 0.0)) found = 1; // inf - inf and NaN - NaN are NaN
    }
    if (found) atomicOr(bad, 1);
}

// The record of a child over [start, start + count) of `ids`, and its place in the lists.  mn/mx: the keys of its box.
__device__ static inline void emit_child(const Outputs &out, const double *boxes, const uint32_t *ids, uint32_t start, uint32_t count, uint32_t node, uint32_t depth,
                                         uint32_t buf, const u64 *mn, const u64 *mx, Ctrl *c, uint32_t nextSel, Seg *bigNext, uint32_t capBig, Seg *small,
                                         uint32_t capSmall) {
    if (count == 1u) {
        const uint32_t id = ids[start];
        write_node(out, node, node + 1u, (int32_t) id, rtt::load_box(boxes + (size_t) id * 6u));
        return;
    }
    rtt::Box b;
    for (int a = 0; a < 3; ++a) { b.mn[a] = rtw::from_key(mn[a]); b.mx[a] = rtw::from_key(mx[a]); }
    write_node(out, node, rtw::skip_of(node, count), -1, b);
    const Seg s{start, count, node, depth | (buf << 8)};
    if (count > (uint32_t) RTW_SWEEP) {
        const uint32_t i = atomicAdd(&c->nbig[nextSel], 1u);
        if (i < capBig) bigNext[i] = s;
        atomicMax(&c->maxcount[nextSel], count);
    } else {
        const uint32_t i = atomicAdd(&c->nsmall, 1u);
        if (i < capSmall) small[i] = s;
    }
}

// ---- the root -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RTWK_BLOCK) void walk_root_box_kernel(uint32_t n, const double *boxes, uint32_t *ids, Ones *ones, Zeros *zeros, const int *bad) {
    __shared__ u64 sh[6];
    if (*bad) return;
    const uint32_t tid = threadIdx.x;
    if (tid < 3u) sh[tid] = ~0ull; else if (tid < 6u) sh[tid] = 0ull;
    __syncthreads();
    u64 mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    const uint32_t lo = blockIdx.x * (uint32_t) RTWK_PART, hi = lo + RTWK_PART < n ? lo + RTWK_PART : n;
    for (uint32_t q = lo + tid; q < hi; q += RTWK_BLOCK) {
        ids[q] = q;
        const double *b = boxes + (size_t) q * 6u;
        for (int a = 0; a < 3; ++a) {
            const u64 k0 = rtw::key_of(b[a * 2]), k1 = rtw::key_of(b[a * 2 + 1]);
            if (k0 < mn[a]) mn[a] = k0;
            if (k1 > mx[a]) mx[a] = k1;
        }
    }
    for (int a = 0; a < 3; ++a) { atomicMin(&sh[a], mn[a]); atomicMax(&sh[3 + a], mx[a]); }
    __syncthreads();
    if (tid < 3u) atomicMin(&ones[0].cmn[0][tid], sh[tid]); else if (tid < 6u) atomicMax(&zeros[0].cmx[0][tid - 3u], sh[tid]);
}
__global__ void walk_root_emit_kernel(uint32_t n, const double *boxes, const uint32_t *ids, const Ones *ones, const Zeros *zeros, Ctrl *c, Seg *big0, uint32_t capBig,
                                      Seg *small, uint32_t capSmall, Outputs out) {
    if (c->bad || threadIdx.x != 0u || blockIdx.x != 0u) return;
    emit_child(out, boxes, ids, 0u, n, 0u, 1u, 0u, ones[0].cmn[0], zeros[0].cmx[0], c, 0u, big0, capBig, small, capSmall);
}

// ---- a level of segments above RTW_SWEEP: blockIdx.x = segment of the level, blockIdx.y = part of RTWK_PART positions ------------------
__global__ __launch_bounds__(RTWK_BLOCK) void walk_bounds_kernel(const Seg *big, const uint32_t *ids0, const uint32_t *ids1, const double *boxes, Ones *ones, Zeros *zeros,
                                                                 Ctrl *c, uint32_t nextSel) {
    __shared__ u64 sh[6];
    if (c->bad) return;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x == 0u && blockIdx.y == 0u && tid == 0u) { c->nbig[nextSel] = 0u; c->maxcount[nextSel] = 0u; } // (emit, later on the stream, counts into them)
    const Seg seg = big[blockIdx.x];
    const uint32_t lo = blockIdx.y * (uint32_t) RTWK_PART;
    if (lo >= seg.count || (seg.dbuf & 255u) >= (uint32_t) RTW_DEPTH) return;
    const uint32_t hi = lo + RTWK_PART < seg.count ? lo + RTWK_PART : seg.count;
    const uint32_t *ids = ((seg.dbuf >> 8) ? ids1 : ids0) + seg.start;
    if (tid < 3u) sh[tid] = ~0ull; else if (tid < 6u) sh[tid] = 0ull;
    __syncthreads();
    u64 mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0ull, 0ull, 0ull};
    for (uint32_t q = lo + tid; q < hi; q += RTWK_BLOCK) {
        const double *b = boxes + (size_t) ids[q] * 6u;
        for (int a = 0; a < 3; ++a) {
            const u64 k = rtw::key_of(b[a * 2] + b[a * 2 + 1]);
            if (k < mn[a]) mn[a] = k;
            if (k > mx[a]) mx[a] = k;
        }
    }
    for (int a = 0; a < 3; ++a) { atomicMin(&sh[a], mn[a]); atomicMax(&sh[3 + a], mx[a]); }
    __syncthreads();
    if (tid < 3u) atomicMin(&ones[blockIdx.x].lo[tid], sh[tid]); else if (tid < 6u) atomicMax(&zeros[blockIdx.x].hi[tid - 3u], sh[tid]);
}

__global__ __launch_bounds__(RTWK_BLOCK) void walk_bins_kernel(const Seg *big, const uint32_t *ids0, const uint32_t *ids1, const double *boxes, Ones *ones, Zeros *zeros,
                                                               const Ctrl *c) {
    __shared__ u64 bmn[3][RTW_BINS][3], bmx[3][RTW_BINS][3];
    __shared__ uint32_t bc[3][RTW_BINS];
    if (c->bad) return;
    const uint32_t tid = threadIdx.x;
    const Seg seg = big[blockIdx.x];
    const uint32_t lo = blockIdx.y * (uint32_t) RTWK_PART;
    if (lo >= seg.count || (seg.dbuf & 255u) >= (uint32_t) RTW_DEPTH) return;
    const uint32_t hi = lo + RTWK_PART < seg.count ? lo + RTWK_PART : seg.count;
    const uint32_t *ids = ((seg.dbuf >> 8) ? ids1 : ids0) + seg.start;
    for (uint32_t i = tid; i < 3u * RTW_BINS * 3u; i += RTWK_BLOCK) { (&bmn[0][0][0])[i] = ~0ull; (&bmx[0][0][0])[i] = 0ull; }
    for (uint32_t i = tid; i < 3u * RTW_BINS; i += RTWK_BLOCK) (&bc[0][0])[i] = 0u;
    double clo[3], scale[3];
    bool use[3];
    for (int a = 0; a < 3; ++a) {
        clo[a] = rtw::from_key(ones[blockIdx.x].lo[a]);
        const double chi = rtw::from_key(zeros[blockIdx.x].hi[a]);
        use[a] = chi > clo[a];
        scale[a] = use[a] ? rtw::bin_scale(clo[a], chi) : 0.0;
    }
    __syncthreads();
    for (uint32_t q = lo + tid; q < hi; q += RTWK_BLOCK) {
        const rtt::Box x = rtt::load_box(boxes + (size_t) ids[q] * 6u);
        u64 kn[3], kx[3];
        for (int d = 0; d < 3; ++d) { kn[d] = rtw::key_of(x.mn[d]); kx[d] = rtw::key_of(x.mx[d]); }
        for (int a = 0; a < 3; ++a) {
            if (!use[a]) continue;
            const int b = rtw::bin_index(rtw::centroid2(x, a), clo[a], scale[a]);
            for (int d = 0; d < 3; ++d) { atomicMin(&bmn[a][b][d], kn[d]); atomicMax(&bmx[a][b][d], kx[d]); }
            atomicAdd(&bc[a][b], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 3u * RTW_BINS; i += RTWK_BLOCK) {
        const uint32_t a = i / RTW_BINS, b = i % RTW_BINS, cnt = bc[a][b];
        if (cnt == 0u) continue;
        for (int d = 0; d < 3; ++d) { atomicMin(&ones[blockIdx.x].binmn[a][b][d], bmn[a][b][d]); atomicMax(&zeros[blockIdx.x].binmx[a][b][d], bmx[a][b][d]); }
        atomicAdd(&zeros[blockIdx.x].bincnt[a][b], cnt);
    }
}

// one thread per segment of the level
__global__ __launch_bounds__(64) void walk_choose_kernel(uint32_t nbig, const Seg *big, const Ones *ones, const Zeros *zeros, Dec *dec, const Ctrl *c) {
    if (c->bad) return;
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s >= nbig) return;
    const Seg seg = big[s];
    Dec d{};
    d.mode = 1; d.axis = 0; d.k = seg.count / 2u;
    if ((seg.dbuf & 255u) < (uint32_t) RTW_DEPTH) {
        int bestAxis = -1, bestB = 0;
        double bestCost = 0.0;
        uint64_t k = 0;
        for (int a = 0; a < 3; ++a) {
            const double lo = rtw::from_key(ones[s].lo[a]), hi = rtw::from_key(zeros[s].hi[a]);
            if (!(hi > lo)) continue;
            rtt::Box bb[RTW_BINS];
            uint64_t cnt[RTW_BINS];
            for (int b = 0; b < RTW_BINS; ++b) {
                cnt[b] = zeros[s].bincnt[a][b];
                for (int x = 0; x < 3; ++x) { bb[b].mn[x] = rtw::from_key(ones[s].binmn[a][b][x]); bb[b].mx[x] = rtw::from_key(zeros[s].binmx[a][b][x]); }
            }
            rtw::bin_choose(a, bb, cnt, bestAxis, bestCost, k, bestB);
        }
        if (bestAxis >= 0) {
            const double lo = rtw::from_key(ones[s].lo[bestAxis]), hi = rtw::from_key(zeros[s].hi[bestAxis]);
            d.mode = 0; d.axis = bestAxis; d.b = bestB; d.k = (uint32_t) k; d.lo = lo; d.scale = rtw::bin_scale(lo, hi);
        }
    }
    dec[s] = d;
}

// The median arm above RTW_SWEEP: the (key of mn[0] + mx[0], id) of rank k = n/2 among the segment's boxes -- exactly k boxes are below it.
// Eleven 8-bit digits from the top (eight of the key, three of the id: ids are below 2^24), each a histogram of the boxes that agree with
// the digits chosen so far.
__device__ static inline uint32_t sel_digit(u64 key, uint32_t id, int j) { return j < 8 ? (uint32_t) (key >> (56 - 8 * j)) & 255u : (id >> (16 - 8 * (j - 8))) & 255u; }
__global__ __launch_bounds__(RTWK_SELECT_THREADS) void walk_select_kernel(const Seg *big, const uint32_t *ids0, const uint32_t *ids1, const double *boxes, Dec *dec,
                                                                          const Ctrl *c) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t chosen, rest;
    if (c->bad) return;
    if (dec[blockIdx.x].mode != 1) return;
    const Seg seg = big[blockIdx.x];
    const uint32_t *ids = ((seg.dbuf >> 8) ? ids1 : ids0) + seg.start;
    const uint32_t tid = threadIdx.x;
    u64 pk = 0ull;
    uint32_t pid = 0u;
    if (tid == 0u) rest = seg.count / 2u;
    for (int j = 0; j < 11; ++j) {
        if (tid < 256u) hist[tid] = 0u;
        __syncthreads();
        for (uint32_t q = tid; q < seg.count; q += RTWK_SELECT_THREADS) {
            const uint32_t id = ids[q];
            const double *b = boxes + (size_t) id * 6u;
            const u64 key = rtw::key_of(b[0] + b[1]);
            bool match = true;
            for (int t = 0; t < j; ++t) match = match && sel_digit(key, id, t) == sel_digit(pk, pid, t);
            if (match) atomicAdd(&hist[sel_digit(key, id, j)], 1u);
        }
        __syncthreads();
        if (tid == 0u) {
            uint32_t r = rest, b = 0u;
            for (; b < 255u; ++b) { if (r < hist[b]) break; r -= hist[b]; }
            chosen = b; rest = r;
        }
        __syncthreads();
        if (j < 8) pk |= (u64) chosen << (56 - 8 * j); else pid |= chosen << (16 - 8 * (j - 8));
    }
    if (tid == 0u) { dec[blockIdx.x].pkey = pk; dec[blockIdx.x].pid = pid; }
}

__global__ __launch_bounds__(RTWK_BLOCK) void walk_partition_kernel(const Seg *big, const uint32_t *ids0, const uint32_t *ids1, uint32_t *out0, uint32_t *out1,
                                                                    const double *boxes, const Dec *dec, Ones *ones, Zeros *zeros, const Ctrl *c) {
    __shared__ u64 smn[2][3], smx[2][3];
    __shared__ uint32_t cnt[2], base[2];
    if (c->bad) return;
    const uint32_t tid = threadIdx.x;
    const Seg seg = big[blockIdx.x];
    const uint32_t lo = blockIdx.y * (uint32_t) RTWK_PART;
    if (lo >= seg.count) return;
    const uint32_t hi = lo + RTWK_PART < seg.count ? lo + RTWK_PART : seg.count;
    const uint32_t buf = seg.dbuf >> 8;
    const uint32_t *ids = (buf ? ids1 : ids0) + seg.start;
    uint32_t *dst = (buf ? out0 : out1) + seg.start; // the other buffer
    const Dec d = dec[blockIdx.x];
    if (tid < 6u) { (&smn[0][0])[tid] = ~0ull; (&smx[0][0])[tid] = 0ull; }
    if (tid < 2u) cnt[tid] = 0u;
    __syncthreads();
    uint32_t my[RTWK_PER], right = 0u, have = 0u, nl = 0u, nr = 0u;
    u64 mn[2][3] = {{~0ull, ~0ull, ~0ull}, {~0ull, ~0ull, ~0ull}}, mx[2][3] = {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}};
    for (int e = 0; e < RTWK_PER; ++e) {
        const uint32_t q = lo + (uint32_t) e * RTWK_BLOCK + tid;
        my[e] = 0u;
        if (q >= hi) continue;
        const uint32_t id = ids[q];
        my[e] = id;
        have |= 1u << e;
        const rtt::Box x = rtt::load_box(boxes + (size_t) id * 6u);
        bool left;
        if (d.mode == 0) left = rtw::bin_index(rtw::centroid2(x, d.axis), d.lo, d.scale) < d.b;
        else { const u64 key = rtw::key_of(rtw::centroid2(x, 0)); left = key < d.pkey || (key == d.pkey && id < d.pid); }
        const int sd = left ? 0 : 1;
        if (left) ++nl; else { ++nr; right |= 1u << e; }
        for (int a = 0; a < 3; ++a) {
            const u64 k0 = rtw::key_of(x.mn[a]), k1 = rtw::key_of(x.mx[a]);
            if (k0 < mn[sd][a]) mn[sd][a] = k0;
            if (k1 > mx[sd][a]) mx[sd][a] = k1;
        }
    }
    const uint32_t offL = nl ? atomicAdd(&cnt[0], nl) : 0u, offR = nr ? atomicAdd(&cnt[1], nr) : 0u;
    for (int sd = 0; sd < 2; ++sd)
        if (sd == 0 ? nl : nr) for (int a = 0; a < 3; ++a) { atomicMin(&smn[sd][a], mn[sd][a]); atomicMax(&smx[sd][a], mx[sd][a]); }
    __syncthreads();
    if (tid < 2u) base[tid] = cnt[tid] ? atomicAdd(&zeros[blockIdx.x].cursor[tid], cnt[tid]) : 0u;
    if (tid < 6u) { atomicMin(&ones[blockIdx.x].cmn[tid / 3u][tid % 3u], (&smn[0][0])[tid]); atomicMax(&zeros[blockIdx.x].cmx[tid / 3u][tid % 3u], (&smx[0][0])[tid]); }
    __syncthreads();
    uint32_t pl = base[0] + offL, pr = d.k + base[1] + offR;
    for (int e = 0; e < RTWK_PER; ++e) {
        if (!(have >> e & 1u)) continue;
        if (right >> e & 1u) { if (pr < seg.count) dst[pr] = my[e]; ++pr; }
        else { if (pl < d.k) dst[pl] = my[e]; ++pl; }
    }
}

// one thread per segment of the level: the two children
__global__ __launch_bounds__(64) void walk_emit_kernel(uint32_t nbig, const Seg *big, const uint32_t *ids0, const uint32_t *ids1, const double *boxes, const Dec *dec,
                                                       const Ones *ones, const Zeros *zeros, Ctrl *c, uint32_t nextSel, Seg *bigNext, uint32_t capBig, Seg *small,
                                                       uint32_t capSmall, Outputs out) {
    if (c->bad) return;
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s >= nbig) return;
    const Seg seg = big[s];
    const uint32_t buf = (seg.dbuf >> 8) ^ 1u, depth = (seg.dbuf & 255u) + 1u, k = dec[s].k;
    const uint32_t *ids = buf ? ids1 : ids0;
    emit_child(out, boxes, ids, seg.start, k, rtw::left_node(seg.node), depth, buf, ones[s].cmn[0], zeros[s].cmx[0], c, nextSel, bigNext, capBig, small, capSmall);
    emit_child(out, boxes, ids, seg.start + k, seg.count - k, rtw::right_node(seg.node, k), depth, buf, ones[s].cmn[1], zeros[s].cmx[1], c, nextSel, bigNext, capBig, small,
               capSmall);
}

// ---- a segment of at most RTW_SWEEP boxes, all its levels, by one workgroup in LDS -----------------------------------------------------
__device__ static inline RBox shfl_box(const RBox &v, int src) {
    RBox o;
    for (int a = 0; a < 3; ++a) { o.b.mn[a] = __shfl(v.b.mn[a], src, 64); o.b.mx[a] = __shfl(v.b.mx[a], src, 64); }
    o.has = __shfl(v.has, src, 64);
    return o;
}
// what the lanes before / after this one hold, combined (has = 0 for the first / last lane); wave-uniform callers only
__device__ static inline RBox wave_before(RBox v) {
    const int lane = (int) (threadIdx.x & 63u);
    for (int off = 1; off < 64; off <<= 1) {
        RBox o = shfl_box(v, lane - off >= 0 ? lane - off : lane);
        if (lane - off < 0) o.has = 0;
        v = comb(o, v);
    }
    RBox e = shfl_box(v, lane > 0 ? lane - 1 : 0);
    if (lane == 0) e.has = 0;
    return e;
}
__device__ static inline RBox wave_after(RBox v) {
    const int lane = (int) (threadIdx.x & 63u);
    for (int off = 1; off < 64; off <<= 1) {
        RBox o = shfl_box(v, lane + off < 64 ? lane + off : lane);
        if (lane + off >= 64) o.has = 0;
        v = comb(v, o);
    }
    RBox e = shfl_box(v, lane < 63 ? lane + 1 : 63);
    if (lane == 63) e.has = 0;
    return e;
}

#define RTWK_KMASK 8191u /* segka: axis << 13 | k, k <= 4095; 0: the segment is not split on this level */

__global__ __launch_bounds__(RTWK_SUB_THREADS) void walk_subtree_kernel(const Seg *small, const uint32_t *ids0, const uint32_t *ids1, const double *boxes, Outputs out,
                                                                        const Ctrl *c) {
    __shared__ uint16_t ord[2][3][RTW_SWEEP]; // per axis the local elements in (key, id) order, segment by segment; double-buffered
    __shared__ uint32_t lid[RTW_SWEEP];       // box index of a local element
    __shared__ uint8_t side[RTW_SWEEP];       // per local element: 1 = it goes right on this level
    __shared__ uint16_t head[RTW_SWEEP];      // per position: the start of its segment
    __shared__ uint16_t segn[RTW_SWEEP], segka[RTW_SWEEP]; // per segment start: its count; the split chosen on this level
    __shared__ uint32_t segnode[RTW_SWEEP];   // per segment start: its node
    __shared__ double sufA[RTW_SWEEP];        // suffix areas of the axis being swept; the sort keys at the start; the scan of a partition
    __shared__ uint16_t act[RTW_SWEEP / 2];
    __shared__ uint32_t nact, wtot[RTWK_SUB_THREADS / 64];
    if (c->bad) return;
    const Seg top = small[blockIdx.x];
    const uint32_t c0 = top.count, tid = threadIdx.x, lane = tid & 63u, wave = tid / 64u;
    if (c0 < 2u || c0 > (uint32_t) RTW_SWEEP) return; // (cannot be: emit_child lists 2..RTW_SWEEP here)
    const uint32_t *ids = ((top.dbuf >> 8) ? ids1 : ids0) + top.start;
    const int32_t depth0 = (int32_t) (top.dbuf & 255u);
    for (uint32_t q = tid; q < c0; q += RTWK_SUB_THREADS) { lid[q] = ids[q]; head[q] = 0; }
    if (tid == 0u) { segn[0] = (uint16_t) c0; segnode[0] = top.node; }
    __syncthreads();
    // the three orders, once: a bitonic sort by (key, id); restricted to any subset it is that subset's order
    {
        u64 *skey = (u64 *) sufA;
        uint32_t Pc = 2u;
        while (Pc < c0) Pc <<= 1;
        for (int a = 0; a < 3; ++a) {
            uint16_t *pay = ord[0][a];
            for (uint32_t i = tid; i < Pc; i += RTWK_SUB_THREADS) {
                if (i < c0) { const double *b = boxes + (size_t) lid[i] * 6u; skey[i] = rtw::key_of(b[a * 2] + b[a * 2 + 1]); } else skey[i] = ~0ull;
                pay[i] = (uint16_t) i;
            }
            __syncthreads();
            for (uint32_t k = 2u; k <= Pc; k <<= 1)
                for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
                    for (uint32_t t = tid; t < Pc / 2u; t += RTWK_SUB_THREADS) {
                        const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), m = i | j;
                        const uint32_t pi = pay[i], pm = pay[m];
                        const uint32_t ii = pi < c0 ? lid[pi] : 0x80000000u + pi, im = pm < c0 ? lid[pm] : 0x80000000u + pm;
                        const bool less = skey[m] != skey[i] ? skey[m] < skey[i] : im < ii; // record m < record i
                        if (less == ((i & k) == 0u)) {
                            const u64 tk = skey[i]; skey[i] = skey[m]; skey[m] = tk;
                            pay[i] = (uint16_t) pm; pay[m] = (uint16_t) pi;
                        }
                    }
                    __syncthreads();
                }
        }
    }
    uint32_t cur = 0u;
    const int32_t bound = rtw::levels_below(c0, depth0);
    for (int32_t l = 0; l < bound; ++l) {
        const int32_t depth = depth0 + l;
        if (tid == 0u) nact = 0u;
        __syncthreads();
        for (uint32_t p = tid; p < c0; p += RTWK_SUB_THREADS)
            if (head[p] == p) {
                segka[p] = 0;
                if (segn[p] >= 2u) act[atomicAdd(&nact, 1u)] = (uint16_t) p;
            }
        __syncthreads();
        const uint32_t na = nact;
        if (na == 0u) break;
        // one wave per segment that splits: the choice and the two children's records
        for (uint32_t si = wave; si < na; si += RTWK_SUB_THREADS / 64u) {
            const uint32_t s = act[si], n = segn[s], me = segnode[s];
            uint32_t axis = 0u, k = n / 2u;
            if (depth < RTW_DEPTH) {
                bool bestHas = false, nanFirst = false;
                double bestCost = 0.0;
                const uint32_t per = (n + 63u) / 64u;
                const uint32_t ja = lane * per < n ? lane * per : n, je = ja + per < n ? ja + per : n;
                for (uint32_t a = 0; a < 3u; ++a) {
                    const uint16_t *o = ord[cur][a] + s;
                    RBox v;
                    v.has = 0;
                    for (uint32_t j = ja; j < je; ++j) {
                        const rtt::Box x = rtt::load_box(boxes + (size_t) lid[o[j]] * 6u);
                        if (v.has) v.b = rtt::merge_two(v.b, x); else { v.b = x; v.has = 1; }
                    }
                    RBox acc = wave_after(v);
                    for (uint32_t j = je; j-- > ja;) { // suffix areas: sufA[s + j] = the area of o[j..n)
                        RBox x;
                        x.b = rtt::load_box(boxes + (size_t) lid[o[j]] * 6u);
                        x.has = 1;
                        acc = comb(x, acc);
                        sufA[s + j] = rtw::half_area(acc.b);
                    }
                    acc = wave_before(v);
                    bool has = false;
                    double bc = 0.0;
                    uint32_t bi = 0u;
                    for (uint32_t j = ja; j < je; ++j) { // the split with the first j on the left: acc = o[0..j)
                        if (j >= 1u) {
                            const double cost = rtw::sweep_cost(rtw::half_area(acc.b), j, sufA[s + j], n);
                            if (a == 0u && j == 1u && cost != cost) nanFirst = true;
                            if (cost == cost && (!has || cost < bc)) { has = true; bc = cost; bi = j; }
                        }
                        RBox x;
                        x.b = rtt::load_box(boxes + (size_t) lid[o[j]] * 6u);
                        x.has = 1;
                        acc = comb(acc, x);
                    }
                    for (int off = 1; off < 64; off <<= 1) { // the first strict minimum: the lower lane keeps a tie
                        const int oh = __shfl_down((int) has, off, 64);
                        const double oc = __shfl_down(bc, off, 64);
                        const uint32_t oi = __shfl_down(bi, off, 64);
                        if (lane + off < 64u && oh && (!has || oc < bc)) { has = true; bc = oc; bi = oi; }
                    }
                    has = __shfl((int) has, 0, 64) != 0;
                    bc = __shfl(bc, 0, 64);
                    bi = __shfl(bi, 0, 64);
                    if (has && (!bestHas || bc < bestCost)) { bestHas = true; bestCost = bc; axis = a; k = bi; }
                }
                if (__any(nanFirst ? 1 : 0) || !bestHas) { axis = 0u; k = 1u; } // a first candidate is accepted whatever it costs, and nothing is < NaN
            }
            const uint16_t *o = ord[cur][axis];
            const RBox L = rtk::wave_range(s, s + k, boxes, [=](uint32_t q) { return lid[o[q]]; });
            const RBox R = rtk::wave_range(s + k, s + n, boxes, [=](uint32_t q) { return lid[o[q]]; });
            if (lane == 0u && k >= 1u && k < n && me >= top.node && rtw::skip_of(me, n) <= rtw::skip_of(top.node, c0)) { // (inside the subtree's own nodes, always)
                const uint32_t ln = rtw::left_node(me), rn = rtw::right_node(me, k), nr = n - k;
                write_node(out, ln, rtw::skip_of(ln, k), k == 1u ? (int32_t) lid[o[s]] : -1, k == 1u ? L.b : canon(L.b));
                write_node(out, rn, rtw::skip_of(rn, nr), nr == 1u ? (int32_t) lid[o[s + k]] : -1, nr == 1u ? R.b : canon(R.b));
                segka[s] = (uint16_t) ((axis << 13) | k);
            }
        }
        __syncthreads();
        for (uint32_t p = tid; p < c0; p += RTWK_SUB_THREADS) {
            const uint32_t s = head[p], ka = segka[s];
            if (ka) side[ord[cur][ka >> 13][p]] = (uint8_t) ((p - s) >= (ka & RTWK_KMASK) ? 1 : 0);
            else side[ord[cur][0][p]] = 0;
        }
        __syncthreads();
        // the three orders, each partitioned stably: position p = 4 * tid + j
        uint16_t *Ls = (uint16_t *) sufA; // Ls[p]: the elements that stay left among positions [0, p)
        for (int a = 0; a < 3; ++a) {
            const uint16_t *src = ord[cur][a];
            uint16_t *dst = ord[cur ^ 1u][a];
            uint32_t f[4], t = 0u;
            for (uint32_t j = 0; j < 4u; ++j) { const uint32_t p = tid * 4u + j; f[j] = p < c0 && side[src[p]] == 0 ? 1u : 0u; t += f[j]; }
            uint32_t incl = t;
            for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if ((int) lane >= off) incl += o; }
            if (lane == 63u) wtot[wave] = incl;
            __syncthreads();
            uint32_t run = incl - t;
            for (uint32_t w = 0; w < wave; ++w) run += wtot[w];
            for (uint32_t j = 0; j < 4u; ++j) { const uint32_t p = tid * 4u + j; if (p < c0) Ls[p] = (uint16_t) run; run += f[j]; }
            __syncthreads();
            for (uint32_t p = tid; p < c0; p += RTWK_SUB_THREADS) {
                const uint32_t s = head[p], ka = segka[s], kk = ka ? (ka & RTWK_KMASK) : (uint32_t) segn[s], e = src[p];
                const uint32_t r = (uint32_t) Ls[p] - (uint32_t) Ls[s];
                const uint32_t d = side[e] == 0 ? s + r : s + kk + ((p - s) - r);
                if (d < c0) dst[d] = (uint16_t) e;
            }
            __syncthreads();
        }
        // the next level's segments
        uint32_t hs[4], hk[4], hn[4], hnode[4];
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t p = tid + j * RTWK_SUB_THREADS;
            hk[j] = 0u;
            if (p >= c0) continue;
            hs[j] = head[p]; hk[j] = segka[hs[j]] & RTWK_KMASK; hn[j] = segn[hs[j]]; hnode[j] = segnode[hs[j]];
        }
        __syncthreads();
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t p = tid + j * RTWK_SUB_THREADS;
            if (p >= c0 || hk[j] == 0u) continue;
            const uint32_t s = hs[j], k = hk[j];
            head[p] = (uint16_t) (p - s < k ? s : s + k);
            if (p == s) {
                segn[s] = (uint16_t) k; segnode[s] = rtw::left_node(hnode[j]);
                segn[s + k] = (uint16_t) (hn[j] - k); segnode[s + k] = rtw::right_node(hnode[j], k);
            }
        }
        __syncthreads();
        cur ^= 1u;
    }
}

} // namespace rtwk
