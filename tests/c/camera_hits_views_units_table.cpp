// The work units of camera hits over a batch of views (rt_camera_hits_views) on a CPU: csrc/rt_views_plan.h's unit_of and first_slot, the
// very functions camera_hits_views_kernel inlines, and csrc/rt_launch_plan.h's unit count for the job.  For n list entries, units of
// `chunk` entries, n_views views and n_samples samples per entry it checks that
//   - the units cover every (view, entry) exactly once, in order, and none spans two views (the last unit of a view is short);
//   - the slot ranges [first_slot, first_slot + npx * n_samples) of successive units partition [0, n_views * n * n_samples) in order;
//   - the planner's unit count for the job is n_views * ceil(n / chunk);
//   - at the refusal bound (n_views * n * n_samples <= INT32_MAX, the most the entry points admit) the largest slot, formed in 32 bits
//     as the kernel forms it, stays below 2^31.
// No input; prints "camera hits views units: ok" and returns 0, or says what failed and returns 1.  tests/test_camera_hits_views_plan.py
// builds and runs it (plain, and once with -fsanitize=address,undefined).
#include "../../ray-tracing-fsharp_amd/csrc/rt_launch_plan.h"
#include "../../ray-tracing-fsharp_amd/csrc/rt_views_plan.h"

#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(cond)                                                                                                                        \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            fprintf(stderr, "FAILED %s (line %d): n=%u chunk=%u n_views=%u n_samples=%u\n", #cond, __LINE__, n, chunk, n_views, n_samples); \
            return 1;                                                                                                                      \
        }                                                                                                                                  \
    } while (0)

static int check_case(uint32_t n, uint32_t chunk, uint32_t n_views, uint32_t n_samples) {
    const rtviews::Plan pl{n, chunk, n_views};
    const uint32_t upv = rtviews::units_per_view(pl);
    const uint64_t units = rtviews::units_of(pl);
    CHECK(upv == (n + chunk - 1u) / chunk && units == (uint64_t) n_views * upv);
    rtp::Job job;
    job.kind = rtp::Job::CAMERA_HITS;
    job.n = n; job.n_views = n_views; job.spp = (int32_t) n_samples;
    CHECK(job.unit_count((int) chunk) == units);
    CHECK(job.ray_count() == (uint64_t) n_views * n * n_samples);
    std::vector<uint8_t> seen((size_t) n_views * n, 0);
    uint64_t nextSlot = 0, nextEntry = 0; // what the next unit must start with: the units come in (view, entry) order
    for (uint64_t u = 0; u < units; ++u) {
        const rtviews::Unit r = rtviews::unit_of(pl, upv, (uint32_t) u);
        CHECK(r.view < n_views && r.npx >= 1u && r.npx <= chunk);
        CHECK((uint64_t) r.first + r.npx <= n);                                  // inside ONE view
        CHECK(r.npx == chunk || r.first + r.npx == n);                           // only a view's last unit is short
        CHECK((uint64_t) r.view * n + r.first == nextEntry);
        for (uint32_t i = 0; i < r.npx; ++i) {
            CHECK(seen[(size_t) r.view * n + r.first + i] == 0);
            seen[(size_t) r.view * n + r.first + i] = 1;
        }
        const uint32_t slot = rtviews::first_slot(pl, r.view, r.first, n_samples);
        CHECK((uint64_t) slot == nextSlot);
        CHECK(rtviews::batch_pixel(pl, r.view, r.first) * n_samples == (uint64_t) slot);
        nextSlot += (uint64_t) r.npx * n_samples;
        nextEntry += r.npx;
    }
    CHECK(nextEntry == (uint64_t) n_views * n && nextSlot == (uint64_t) n_views * n * n_samples);
    for (uint8_t s : seen) CHECK(s == 1);
    return 0;
}

// The refusal bound: the largest n with n_views * n * n_samples <= INT32_MAX; the last unit of the last view, and its last item's slot.
static int check_bound(uint32_t chunk, uint32_t n_views, uint32_t n_samples) {
    const uint32_t n = (uint32_t) ((uint64_t) INT32_MAX / ((uint64_t) n_views * n_samples));
    CHECK(n >= 1u && (uint64_t) n_views * n * n_samples <= (uint64_t) INT32_MAX);
    CHECK((uint64_t) n_views * ((uint64_t) n + 1u) * n_samples > (uint64_t) INT32_MAX); // (one more entry would be refused)
    const rtviews::Plan pl{n, chunk, n_views};
    const uint32_t upv = rtviews::units_per_view(pl);
    const uint64_t units = rtviews::units_of(pl);
    CHECK(units <= (uint64_t) INT32_MAX); // (below the poisoned unit counter, 2^31: every wave leaves at its first reservation)
    const rtviews::Unit r = rtviews::unit_of(pl, upv, (uint32_t) (units - 1u));
    CHECK(r.view == n_views - 1u && r.first + r.npx == n);
    const uint32_t last = rtviews::first_slot(pl, r.view, r.first, n_samples) + r.npx * n_samples - 1u; // as the kernel: slot0 + item
    CHECK((uint64_t) last == (uint64_t) n_views * n * n_samples - 1u && last < (1u << 31));
    const rtviews::Unit f = rtviews::unit_of(pl, upv, (uint32_t) (units - upv)); // the last view's first unit
    CHECK(f.view == n_views - 1u && f.first == 0u);
    CHECK((uint64_t) rtviews::first_slot(pl, f.view, f.first, n_samples) == (uint64_t) (n_views - 1u) * n * n_samples);
    return 0;
}

int main() {
    const uint32_t ns[] = {1, 5, 9, 63, 64, 65}, chunks[] = {1, 3, 10, 64}, views[] = {1, 2, 70, 4097}, samples[] = {1, 7};
    int cases = 0;
    for (uint32_t n : ns)
        for (uint32_t chunk : chunks)
            for (uint32_t v : views)
                for (uint32_t s : samples) {
                    if (check_case(n, chunk, v, s)) return 1;
                    ++cases;
                }
    for (uint32_t chunk : chunks)
        for (uint32_t v : views)
            for (uint32_t s : samples) {
                if (check_bound(chunk, v, s)) return 1;
                ++cases;
            }
    printf("camera hits views units: ok (%d cases)\n", cases);
    return 0;
}
