// rt_walk_plan.h -- the rules of the surface-area build of the tree the device walks (rt_scene.h SahBuilder, the arms without probe
// rays), in one place.  Plain C++ for host and device (no HIP calls), in the manner of rt_tree_plan.h: SahBuilder, the kernels of
// rt_walk_kernels.h and tests/c/walk_plan_table.cpp all include this one definition.
//
// Layout.  A node over n boxes holds the union of its boxes; in pre-order node `me` has its left child at me + 1 over k boxes, its right
// child at me + 2k over n - k boxes, and skip[me] = me + 2n - 1: 2n - 1 nodes always.  Unlike BoundingBoxTree.make's tree the SHAPE depends
// on the boxes (k is chosen by cost), so a node index is known only once every split above it is.
//
// Split of a node over n boxes at `depth` (the root is at depth 1):
//   n <= RTW_SWEEP and depth < RTW_DEPTH   each axis swept in the order of (mn + mx, id); cost(i) = sweep_cost; the first strict minimum
//                                          over axis 0, 1, 2 and then i ascending; children: the first k of that order and the rest
//   n >  RTW_SWEEP and depth < RTW_DEPTH   RTW_BINS centroid bins per axis over [lo, hi] of mn + mx (an axis with !(hi > lo) is skipped);
//                                          candidates b = 1..31 with both sides non-empty, bin_choose; the left child is the SET of
//                                          boxes in bins below b
//   no winning axis, or depth >= RTW_DEPTH k = n / 2, the k smallest by (mn[0] + mx[0], id)
// Centroids compare as doubles (-0.0 == +0.0, then the id decides), so a sort key made from bits canonicalises the zero: key_of.
// Nothing here may be contracted (-ffp-contract=off holds for host and device); the cost expressions keep the association written here.
#pragma once
#include "rt_tree_plan.h"

#define RTW_SWEEP 4096 /* above this many boxes a node is split on centroid bins instead of a full sweep */
#define RTW_BINS 32
#define RTW_DEPTH 48   /* from this depth on a node is halved by centroid order on axis 0 */

namespace rtw {

template <class B> RTT_HD static inline double centroid2(const B &b, int axis) { return b.mn[axis] + b.mx[axis]; }
// half the surface area; non-positive extents are clamped to 0, so inverted (negative-radius) boxes count as empty
template <class B> RTT_HD static inline double half_area(const B &b) {
    double d[3];
    for (int a = 0; a < 3; ++a) { d[a] = b.mx[a] - b.mn[a]; if (!(d[a] > 0.0)) d[a] = 0.0; }
    return d[0] * d[1] + d[1] * d[2] + d[0] * d[2];
}
// a subtree of m leaves has 2m - 1 boxes.  Sweep: left = the first i of n in the axis' order.  Bins: left = nl boxes, right = nr.
RTT_HD static inline double sweep_cost(double area_left, uint64_t i, double area_right, uint64_t n) {
    return area_left * (double) (2 * i - 1) + area_right * (double) (2 * (n - i) - 1);
}
RTT_HD static inline double bin_cost(double area_left, uint64_t nl, double area_right, uint64_t nr) {
    return area_left * (double) (2 * nl - 1) + area_right * (double) (2 * nr - 1);
}
RTT_HD static inline double bin_scale(double lo, double hi) { return (double) RTW_BINS / (hi - lo); } // hi > lo
RTT_HD static inline int bin_index(double c, double lo, double scale) {
    int b = (int) ((c - lo) * scale);
    if (b >= RTW_BINS) b = RTW_BINS - 1;
    if (b < 0) b = 0;
    return b;
}

// The order-preserving key of a centroid under `<` with -0.0 mapped onto +0.0 (rt_tree_plan.h), and back: from_key(key_of(v)) == v, and is
// +0.0 for either zero.
RTT_HD static inline uint64_t key_of(double v) { return rtt::key_of(v); }
RTT_HD static inline double from_key(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    __builtin_memcpy(&v, &u, sizeof(v));
    return v;
}

// pre-order positions
RTT_HD static inline uint32_t left_node(uint32_t me) { return me + 1u; }
RTT_HD static inline uint32_t right_node(uint32_t me, uint32_t k) { return me + 2u * k; }
RTT_HD static inline uint32_t skip_of(uint32_t me, uint32_t n) { return me + 2u * n - 1u; }
// Levels a subtree over n boxes whose root is at `depth` can still have below its root: one box at least leaves a node per level until
// RTW_DEPTH, then the node is halved.  The bound of every level loop of the build.
RTT_HD static inline int32_t levels_below(uint32_t n, int32_t depth) {
    int32_t l = 0;
    uint32_t c = n;
    for (; depth + l < RTW_DEPTH && c > 1u; ++l) --c;        // the worst case: one box peeled per level
    for (; c > 1u; c = c - c / 2u) ++l;                       // halving: the larger child has c - c/2 boxes
    return l;
}

// BoundingBox.mergeTwo for any box type with mn[3], mx[3] (rt_tree_plan.h merge_two: min keeps the later operand on a tie, max the earlier)
template <class B> RTT_HD static inline B merge_two(const B &i, const B &j) {
    B o;
    for (int a = 0; a < 3; ++a) { o.mn[a] = i.mn[a] < j.mn[a] ? i.mn[a] : j.mn[a]; o.mx[a] = i.mx[a] < j.mx[a] ? j.mx[a] : i.mx[a]; }
    return o;
}

// The binned arm's choice on one axis, after the boxes and counts of the RTW_BINS bins are known (cnt[b] == 0: bin b is empty and bb[b]
// is not read).  Updates (bestAxis, bestCost, k) as the sweep does: the first strict minimum, a first candidate always accepted.
// bestB: the winning bin boundary (left = bins [0, b)).
template <class B> RTT_HD static inline void bin_choose(int axis, const B *bb, const uint64_t *cnt, int &bestAxis, double &bestCost, uint64_t &k, int &bestB) {
    double sufA[RTW_BINS + 1];
    uint64_t sufN[RTW_BINS + 1];
    B acc{};
    bool any = false;
    sufN[RTW_BINS] = 0; sufA[RTW_BINS] = 0.0;
    for (int b = RTW_BINS - 1; b >= 0; --b) {
        if (cnt[b]) { acc = any ? merge_two(acc, bb[b]) : bb[b]; any = true; }
        sufN[b] = sufN[b + 1] + cnt[b]; sufA[b] = any ? half_area(acc) : 0.0;
    }
    any = false;
    uint64_t nl = 0;
    for (int b = 1; b < RTW_BINS; ++b) { // left = bins [0, b)
        if (cnt[b - 1]) { acc = any ? merge_two(acc, bb[b - 1]) : bb[b - 1]; any = true; }
        nl += cnt[b - 1];
        if (nl == 0 || sufN[b] == 0) continue;
        const double cost = bin_cost(half_area(acc), nl, sufA[b], sufN[b]);
        if (bestAxis < 0 || cost < bestCost) { bestCost = cost; bestAxis = axis; k = nl; bestB = b; }
    }
}

} // namespace rtw
