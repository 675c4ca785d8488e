// csrc/rt_tree_plan.h against the plain recursion of BoundingBoxTree.make's shape (BoundingBoxTree.fs:14-41): for every n in 1..4100 and for
// 1e5, 1e6 and 4,500,000 the recursion visits every node once, and the plan must name the same segment, node index, skip link and level for
// it, cover every position of every level exactly once with slots that rise with the position, and agree on depth and node count.  Then the
// key: monotonic under `<`, both zeros equal, the infinities at the ends.  A stand-alone program (tests/test_tree_plan.py builds it plainly
// and under -fsanitize=address,undefined).
#include "../../ray-tracing-fsharp_amd/csrc/rt_tree_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static long g_nodes = 0;
static int g_depth = 0;
static uint32_t g_n = 0;
static std::vector<uint32_t> g_slots; // per level: the next slot expected (slots rise with the position)
static std::vector<uint32_t> g_covered;

#define CHECK(c) do { if (!(c)) { printf("FAIL %s (n=%u) line %d\n", #c, g_n, __LINE__); exit(1); } } while (0)

// the recursion as the reference writes it: returns the index after the subtree
static uint32_t go(uint32_t start, uint32_t c, uint32_t me, int level, uint32_t slot) {
    ++g_nodes;
    if (level + 1 > g_depth) g_depth = level + 1;
    const rtt::Segment s = rtt::segment(g_n, level, slot);
    CHECK(s.start == start && s.count == c && s.node == me && s.level == level);
    if ((size_t) level >= g_slots.size()) { g_slots.resize((size_t) level + 1, 0u); g_covered.resize((size_t) level + 1, 0u); }
    CHECK(slot >= g_slots[(size_t) level]);
    g_slots[(size_t) level] = slot + 1u;
    g_covered[(size_t) level] += c;
    uint32_t next;
    if (c == 1) {
        next = me + 1;
        // below a Leaf: going left keeps it (with its own level), going right is no slot
        const rtt::Segment l = rtt::segment(g_n, level + 2, slot << 2), r = rtt::segment(g_n, level + 1, (slot << 1) | 1u);
        CHECK(l.start == start && l.count == 1 && l.node == me && l.level == level && r.count == 0);
    } else {
        const uint32_t nl = c == 2 ? 1 : c / 2 + 1; // boxes.[0 .. n/2] and boxes.[n/2+1 ..]; two boxes: two Leaves
        CHECK(rtt::left_count(c) == nl);
        const uint32_t mid = go(start, nl, me + 1, level + 1, slot << 1);
        CHECK(mid == me + 1 + (2 * nl - 1));
        next = go(start + nl, c - nl, mid, level + 1, (slot << 1) | 1u);
    }
    CHECK(rtt::skip_of(s) == next && next == me + 2 * c - 1);
    return next;
}

static void one(uint32_t n) {
    g_n = n; g_nodes = 0; g_depth = 0; g_slots.clear(); g_covered.clear();
    const uint32_t end = go(0, n, 0, 0, 0);
    CHECK((int64_t) end == rtt::node_count(n) && g_nodes == rtt::node_count(n));
    CHECK(g_depth == rtt::depth(n));
    for (int l = 0; l < g_depth; ++l) CHECK(rtt::max_count(n, l) == rtt::segment(n, l, 0).count);
    const int lg = rtt::levels_above(n, RTT_S);
    CHECK(rtt::max_count(n, lg) <= (uint32_t) RTT_S || n <= 1);
    if (lg > 0) CHECK(rtt::max_count(n, lg - 1) > (uint32_t) RTT_S);
    if (lg > 0) CHECK(g_covered[(size_t) lg] == n); // no Leaf ends above the level that goes to LDS
}

static void keys() {
    const double v[] = {-HUGE_VAL, -1.7976931348623157e308, -2.5, -1.0, -4.9406564584124654e-324, -0.0, 0.0, 4.9406564584124654e-324, 1.0, 1.0000000000000002,
                        2.5, 1.7976931348623157e308, HUGE_VAL};
    const int m = (int) (sizeof(v) / sizeof(v[0]));
    g_n = 0;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            CHECK((v[i] < v[j]) == (rtt::key_of(v[i]) < rtt::key_of(v[j])));
            CHECK((v[i] == v[j]) == (rtt::key_of(v[i]) == rtt::key_of(v[j])));
        }
    CHECK(rtt::key_of(-0.0) == rtt::key_of(0.0));
    CHECK(rtt::key_of(-HUGE_VAL) == 0x000FFFFFFFFFFFFFull && rtt::key_of(HUGE_VAL) == 0xFFF0000000000000ull);
    // the merge rules: min keeps the later operand of a tie, max the earlier one
    CHECK(std::signbit(rtt::merge_min(0.0, -0.0)) && !std::signbit(rtt::merge_min(-0.0, 0.0)));
    CHECK(!std::signbit(rtt::merge_max(0.0, -0.0)) && std::signbit(rtt::merge_max(-0.0, 0.0)));
    const double nan = std::nan("");
    const double c1[3] = {nan, 1.0, 1.0}, c2[3] = {2.0, nan, 2.0}, c3[3] = {3.0, 2.0, 2.0}, c4[3] = {1.0, 1.0, 0.5};
    CHECK(rtt::best_axis(c1) == 0 && rtt::best_axis(c2) == 0 && rtt::best_axis(c3) == 1 && rtt::best_axis(c4) == 2);
}

int main() {
    for (uint32_t n = 1; n <= 4100; ++n) one(n);
    printf("shape 1..4100 ok\n");
    one(100000); one(1000000); one(4500000);
    CHECK(rtt::depth(485) == 11 && rtt::depth(100000) == 19 && rtt::depth(1000000) == 22 && rtt::depth(4500000) == 25);
    CHECK(rtt::node_count(0) == 0 && rtt::depth(0) == 0);
    printf("shape large ok\n");
    keys();
    printf("keys ok\n");
    return 0;
}
