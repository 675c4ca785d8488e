// The item -> (pixel, offset) lookup of an extension by map (csrc/rt_extend_map.h: the function pass B's map variant inlines),
// driven exhaustively on a CPU for tests/test_extend_map_host.py.  One line in, one line out:
//   lookup npx n2_0 .. n2_{npx-1}
// Every item 0 .. total-1 is mapped with rtm::map_find_pixel over the starts of rtm::map_starts and held to the pixel and offset a
// plain walk over the counts gives; the line printed is
//   npx=<npx> total=<total> wrong=<items mapped to another (pixel, offset)> uncovered=<(pixel, offset) pairs not hit exactly once> reads=<most reads of `start` by one search>
#include "../../ray-tracing-fsharp_amd/csrc/rt_extend_map.h"

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

struct CountingStarts { // counts the reads a search makes; refuses one outside the range's pixels
    const uint32_t *v; uint32_t n; mutable uint32_t reads = 0, outside = 0;
    uint32_t operator[](uint32_t i) const { ++reads; if (i >= n) { ++outside; return 0u; } return v[i]; }
};

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what != "lookup") return 2;
        uint32_t npx = 0;
        std::cin >> npx;
        if (!std::cin || npx < 1 || npx > RTM_MAX_PIXELS) return 2;
        std::vector<uint32_t> n2(npx), start(npx);
        for (auto &v : n2) std::cin >> v;
        if (!std::cin) return 2;
        const uint32_t total = rtm::map_starts(n2.data(), npx, start.data());
        std::vector<std::vector<uint32_t>> hits(npx);
        for (uint32_t j = 0; j < npx; ++j) hits[j].assign(n2[j], 0u);
        unsigned long long wrong = 0, uncovered = 0;
        uint32_t mostReads = 0, outside = 0;
        uint32_t wantPx = 0, wantOff = 0; // the plain walk
        for (uint32_t item = 0; item < total; ++item) {
            while (wantOff >= n2[wantPx]) { ++wantPx; wantOff = 0; }
            CountingStarts cs{start.data(), npx};
            const uint32_t j = rtm::map_find_pixel<const CountingStarts &>(cs, npx, item);
            const uint32_t off = j < npx ? item - start[j] : 0u;
            if (j != wantPx || off != wantOff) ++wrong;
            if (j < npx && off < n2[j]) hits[j][off]++;
            if (cs.reads > mostReads) mostReads = cs.reads;
            outside += cs.outside;
            ++wantOff;
        }
        for (uint32_t j = 0; j < npx; ++j)
            for (uint32_t h : hits[j]) uncovered += h != 1u;
        printf("npx=%u total=%u wrong=%llu uncovered=%llu reads=%u outside=%u\n", npx, total, wrong, uncovered, mostReads, outside);
    }
    return 0;
}
