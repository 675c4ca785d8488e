// csrc/rt_walk_plan.h alone: the order-preserving key (zeros included) and its inverse, the bin index at its edges, the pre-order positions
// against a plain recursion, the level bound, the cost expressions' association and half_area's clamp.  Prints one line per part.
#include "../../ray-tracing-fsharp_amd/csrc/rt_walk_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct B { double mn[3], mx[3]; };

// positions: a tree whose node over n boxes puts k(n, depth) on the left, laid out by recursion with a running counter
static uint32_t counter;
static uint32_t pick(uint32_t n, int depth) { return 1u + (uint32_t) ((n * 2654435761u + (uint32_t) depth * 40503u) % (n - 1u)); }
static void lay(uint32_t n, int depth, uint32_t expect_me, int &deepest) {
    const uint32_t me = counter++;
    CHECK(me == expect_me);
    if (depth > deepest) deepest = depth;
    if (n > 1u) {
        const uint32_t k = pick(n, depth);
        lay(k, depth + 1, rtw::left_node(me), deepest);
        lay(n - k, depth + 1, rtw::right_node(me, k), deepest);
    }
    CHECK(counter == rtw::skip_of(me, n));
}

int main() {
    // ---- keys ----
    const double inf = std::numeric_limits<double>::infinity(), tiny = std::numeric_limits<double>::denorm_min(), big = std::numeric_limits<double>::max();
    const double v[] = {-inf, -big, -1e300, -2.5, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, 2.5, 1e300, big, inf};
    const size_t nv = sizeof(v) / sizeof(v[0]);
    for (size_t i = 0; i < nv; ++i)
        for (size_t j = 0; j < nv; ++j) {
            CHECK((v[i] < v[j]) == (rtw::key_of(v[i]) < rtw::key_of(v[j])));
            CHECK((v[i] == v[j]) == (rtw::key_of(v[i]) == rtw::key_of(v[j])));
        }
    CHECK(rtw::key_of(-0.0) == rtw::key_of(0.0));
    for (size_t i = 0; i < nv; ++i) {
        const double back = rtw::from_key(rtw::key_of(v[i]));
        CHECK(back == v[i]);
        if (v[i] == 0.0) CHECK(!std::signbit(back)); // either zero comes back as +0.0
    }
    CHECK(rtw::key_of(-inf) > 0ull && rtw::key_of(inf) < ~0ull); // the all-zeros and all-ones words are free: "no maximum yet", "no minimum yet"
    std::printf("keys ok\n");

    // ---- bin index ----
    {
        const double lo = -3.0, hi = 5.0, s = rtw::bin_scale(lo, hi);
        CHECK(s == 4.0);
        CHECK(rtw::bin_index(lo, lo, s) == 0);
        CHECK(rtw::bin_index(hi, lo, s) == RTW_BINS - 1);              // (hi - lo) * scale == 32: clamped
        CHECK(rtw::bin_index(std::nextafter(hi, lo), lo, s) == RTW_BINS - 1);
        CHECK(rtw::bin_index(-2.75, lo, s) == 1 && rtw::bin_index(std::nextafter(-2.75, lo), lo, s) == 0);
        CHECK(rtw::bin_index(-4.0, lo, s) == 0);                        // below lo: clamped (cannot happen for a segment's own boxes)
        CHECK(rtw::bin_index(-0.0, 0.0, rtw::bin_scale(0.0, 1.0)) == 0 && rtw::bin_index(0.0, -0.0, rtw::bin_scale(-0.0, 1.0)) == 0);
        const double s2 = rtw::bin_scale(0.0, 64.0 * 64.0 * 64.0);      // an outlier: everything near 0 lands in bin 0
        CHECK(rtw::bin_index(1.0, 0.0, s2) == 0 && rtw::bin_index(64.0 * 64.0 * 64.0, 0.0, s2) == RTW_BINS - 1);
    }
    std::printf("bins ok\n");

    // ---- positions and the level bound ----
    for (uint32_t n = 1; n <= 300u; ++n) {
        counter = 0;
        int deepest = 0;
        lay(n, 1, 0u, deepest);
        CHECK(counter == 2u * n - 1u);
        CHECK(deepest - 1 <= (int) n - 1);
    }
    CHECK(rtw::levels_below(1u, 1) == 0 && rtw::levels_below(2u, 1) == 1 && rtw::levels_below(2u, 60) == 1);
    CHECK(rtw::levels_below(64u, 1) == 47 + 5);   // 47 peels leave 17 boxes at depth 48: 17 -> 9 -> 5 -> 3 -> 2 -> 1
    CHECK(rtw::levels_below(4096u, 48) == 12 && rtw::levels_below(4097u, 48) == 13);
    CHECK(rtw::levels_below(4500000u, 1) < 80);
    std::printf("positions ok\n");

    // ---- costs and half_area ----
    {
        const B inv = {{0, 0, 0}, {-1, 2, 3}}, flat = {{0, 0, 0}, {0, 2, 3}}, unit = {{0, 0, 0}, {1, 2, 3}};
        CHECK(rtw::half_area(inv) == 6.0 && rtw::half_area(flat) == 6.0 && rtw::half_area(unit) == 11.0);
        const B nan = {{0, 0, 0}, {std::nan(""), 2, 3}};
        CHECK(rtw::half_area(nan) == 6.0); // !(d > 0) clamps a NaN extent as well
        CHECK(rtw::sweep_cost(3.0, 1, 5.0, 10) == 3.0 * 1.0 + 5.0 * 17.0);
        CHECK(rtw::bin_cost(3.0, 4, 5.0, 6) == 3.0 * 7.0 + 5.0 * 11.0);
        const double a = 0.1, b = 0.7; // the association: (a * wl) + (b * wr), each product rounded on its own
        const double wl = 5.0, wr = 13.0, pl = a * wl, pr = b * wr;
        CHECK(rtw::sweep_cost(a, 3, b, 10) == pl + pr);
        CHECK(rtw::centroid2(unit, 1) == 2.0);
    }
    // bin_choose: the first strict minimum, empty sides skipped
    {
        B bb[RTW_BINS];
        uint64_t cnt[RTW_BINS];
        for (int i = 0; i < RTW_BINS; ++i) { cnt[i] = 0; bb[i] = B{{0, 0, 0}, {0, 0, 0}}; }
        cnt[0] = 2; bb[0] = B{{0, 0, 0}, {1, 1, 1}};
        cnt[10] = 2; bb[10] = B{{5, 0, 0}, {6, 1, 1}};
        cnt[31] = 2; bb[31] = B{{10, 0, 0}, {11, 1, 1}};
        int axis = -1, bestB = 0;
        double cost = 0.0;
        uint64_t k = 0;
        rtw::bin_choose(0, bb, cnt, axis, cost, k, bestB);
        CHECK(axis == 0 && k == 2 && bestB == 1); // b = 1..10 all cost the same: the first is kept; b = 11 costs the same by symmetry
        int axis2 = axis, b2 = bestB;
        double cost2 = cost;
        uint64_t k2 = k;
        rtw::bin_choose(1, bb, cnt, axis2, cost2, k2, b2); // the same cost on another axis does not win
        CHECK(axis2 == 0 && k2 == 2 && b2 == 1 && cost2 == cost);
    }
    std::printf("costs ok\n");
    return fails ? 1 : 0;
}
