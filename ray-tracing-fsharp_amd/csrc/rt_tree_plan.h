// rt_tree_plan.h -- the shape of BoundingBoxTree.make's tree (BoundingBoxTree.fs:9-43) as a function of the number of boxes alone, and the
// comparisons its build makes.  Plain C++ for host and device (no HIP calls), like rt_png.h and rt_pixel_map.h: the host side of the ABI,
// the kernels of rt_tree_kernels.h and tests/c/tree_plan_table.cpp all include this one definition.
//
// Shape.  A node over c boxes has children over c/2 + 1 and c - c/2 - 1 boxes (BoundingBoxTree.fs:28-29); c = 2 gives two Leaves without
// sorting, c = 1 is a Leaf.  A subtree over c boxes has 2c - 1 nodes, so in pre-order the left child of node `me` is me + 1, the right one
// me + 1 + (2*nl - 1), and skip[me] = me + 2c - 1.  Every segment boundary, node index and the number of levels are therefore known before a
// box is read, and the build can run level by level over ONE array of box indices in which a node is a contiguous segment.
//
// Order.  Array.sortBy is defined stable here (DESIGN.md "Tree shape"): a stable sort by Min[axis] is ANY sort by the unique key
// (Min[axis], position in the segment's current order).  The comparison is `<` on doubles, so -0.0 and +0.0 tie; NaN has no order and is
// refused by the callers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTT_HD __host__ __device__
#else
#define RTT_HD
#endif

// S: the largest segment one workgroup finishes in LDS (all its remaining levels in one launch).  Per leaf the workgroup keeps the sort
// record of the axis being sorted (8-byte key, 4-byte slot and position), three 2-byte sorted positions (one per axis), two 4-byte box
// indices (the order, double-buffered) and a 2-byte slot: 28 bytes, 56 KiB at S = 2048 -- two workgroups per CU in the 160 KiB LDS, so a CU
// that waits on one workgroup's box gathers has another to run.  S = 4096 (112 KiB) would leave one workgroup per CU and halve the number
// of subtrees in flight where the build hands over to LDS.  Boxes stay in global memory: 48 bytes each would be 96 KiB more at S = 2048.
#define RTT_S 2048
#define RTT_MAX_BOXES 4500000u /* the scene's own limit (rt_scene.h: (2n-1) * 112 B < 2^30) */
#define RTT_PART 4096          /* boxes one workgroup reduces of a global level's half segment */

namespace rtt {

struct Segment {
    uint32_t start; // first position of the segment in the order array
    uint32_t count; // boxes in it; 0: the slot does not exist
    uint32_t node;  // pre-order index of its node
    int32_t level;  // the level its node is on (0 = root); < the level asked for: a Leaf that ended above it
};

RTT_HD static inline uint32_t left_count(uint32_t c) { return c == 2u ? 1u : c / 2u + 1u; } // c >= 2
RTT_HD static inline int64_t node_count(uint64_t n) { return n == 0 ? 0 : (int64_t) (2 * n - 1); }
// levels of the tree (nodes on the longest root-to-leaf path): the left child is never the smaller one
RTT_HD static inline int32_t depth(uint64_t n) {
    if (n == 0) return 0;
    int32_t d = 1;
    for (uint32_t c = (uint32_t) n; c > 1u; c = left_count(c)) ++d;
    return d;
}
// the largest segment on `level` (the leftmost one)
RTT_HD static inline uint32_t max_count(uint32_t n, int32_t level) {
    uint32_t c = n;
    for (int32_t l = 0; l < level && c > 1u; ++l) c = left_count(c);
    return c;
}
// the first level on which every segment has at most `s` boxes
RTT_HD static inline int32_t levels_above(uint32_t n, uint32_t s) {
    int32_t l = 0;
    for (uint32_t c = n; c > s && c > 1u; c = left_count(c)) ++l;
    return l;
}
// Segment `slot` of `level` in a tree over n boxes: bit (level-1-k) of slot chooses the child at step k (0 left, 1 right).  A Leaf that
// ended above `level` is returned for the slots that keep going LEFT below it (so every position of the order array belongs to exactly
// one slot of every level, and slots are monotonic in the position); going right below a Leaf gives count 0.
RTT_HD static inline Segment segment(uint32_t n, int32_t level, uint32_t slot) {
    Segment s{0u, n, 0u, 0};
    for (int32_t k = 0; k < level; ++k) {
        const uint32_t right = (slot >> (level - 1 - k)) & 1u;
        if (s.count <= 1u) {
            if (right) { s.count = 0u; return s; }
            continue;
        }
        const uint32_t nl = left_count(s.count);
        if (right) { s.start += nl; s.node += 2u * nl; s.count -= nl; }
        else { s.node += 1u; s.count = nl; }
        s.level = k + 1;
    }
    return s;
}
RTT_HD static inline uint32_t skip_of(const Segment &s) { return s.node + 2u * s.count - 1u; }

// The order-preserving 64-bit key of a double under `<`, -0.0 mapped onto +0.0.  -inf and +inf are the ends; NaN is the caller's to refuse.
RTT_HD static inline uint64_t key_of(double v) {
    if (v == 0.0) v = 0.0; // -0.0 == 0.0: both become +0.0
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof(u)); // (the builtin: the same on the host and in device code, whatever was included before)
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

struct Box { double mn[3], mx[3]; };
// BoundingBox.mergeTwo (BoundingBox.fs:96-108), reduced left to right by BoundingBox.merge: `i` is the earlier operand.  min keeps the
// LATER operand on a tie, max the EARLIER one -- with both zeros present the sign of a zero in a Branch box depends on the order.  Both
// rules are associative, so an ordered tree reduction gives what the left-to-right one does.
RTT_HD static inline double merge_min(double i, double j) { return i < j ? i : j; }
RTT_HD static inline double merge_max(double i, double j) { return i < j ? j : i; }
RTT_HD static inline Box merge_two(const Box &i, const Box &j) {
    Box o;
    for (int a = 0; a < 3; ++a) { o.mn[a] = merge_min(i.mn[a], j.mn[a]); o.mx[a] = merge_max(i.mx[a], j.mx[a]); }
    return o;
}
// BoundingBox.volume (BoundingBox.fs:13-16) and the split's cost (BoundingBoxTree.fs:31); nothing may be contracted (-ffp-contract=off)
RTT_HD static inline double volume(const Box &b) { return (b.mx[0] - b.mn[0]) * (b.mx[1] - b.mn[1]) * (b.mx[2] - b.mn[2]); }
RTT_HD static inline double cost(const Box &l, const Box &r) { return volume(l) + volume(r); }
// Array.minBy: the first strict minimum; a NaN cost is never `<`
RTT_HD static inline int best_axis(const double c[3]) {
    int best = 0;
    for (int a = 1; a < 3; ++a) if (c[a] < c[best]) best = a;
    return best;
}
// a box of the ABI's form (minx, maxx, miny, maxy, minz, maxz)
RTT_HD static inline Box load_box(const double *b) { return Box{{b[0], b[2], b[4]}, {b[1], b[3], b[5]}}; }
RTT_HD static inline void store_box(double *b, const Box &x) { for (int a = 0; a < 3; ++a) { b[a * 2] = x.mn[a]; b[a * 2 + 1] = x.mx[a]; } }

} // namespace rtt
