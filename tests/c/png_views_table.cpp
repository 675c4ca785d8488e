// The batch layout of csrc/rt_png.h ("a batch of equal-sized images") driven alone on a CPU, for tests/test_png_views_host.py: the scan the
// kernels run is done here in a plain loop over the entry counts the layout charges, and everything the kernels read off the scanned
// array is printed for the test to hold against its own straightforward arithmetic.
//   stdin:   one line per batch:  K rows cols b(0,0) b(0,1) ... b(K-1,tiles-1)    (the byte count of every tile, image by image)
//   stdout:  one line per batch:  tiles=<per image> entries=<n> total=<bytes> entry=<K*tiles indices> start=<K+1 offsets> end=<K> idat=<K>
//            tile=<K*tiles offsets> go=<capacity total-1, total, total+1, and total without a buffer>     (lists are comma separated)
// -DRTP_VIEWS_MUTANT=1..3 builds one of rt_png.h's three wrong layouts: the test expects each to be caught.
// Build: g++ -std=c++17 -Wall -Werror -O1 [-fsanitize=address,undefined] -o png_views_table tests/c/png_views_table.cpp
#include "../../ray-tracing-fsharp_amd/csrc/rt_png.h"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

template <class T> static void print_list(const char *name, const std::vector<T> &v) {
    printf(" %s=", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long) v[i]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint64_t K, rows, cols;
        if (!(in >> K >> rows >> cols)) continue;
        const uint64_t tiles = rtp::tile_count(rows, cols), n = rtp::views_entry_count(K, tiles);
        std::vector<uint64_t> entries((size_t) n + 2u, 0u), entry; // (two spare words: a wrong layout must not leave the array)
        for (uint64_t v = 0; v < K; ++v) {
            for (uint64_t t = 0; t < tiles; ++t) {
                uint64_t bytes;
                if (!(in >> bytes)) { fprintf(stderr, "too few tile byte counts\n"); return 2; }
                entries[(size_t) rtp::views_entry(v, t, tiles)] = bytes;
                entry.push_back(rtp::views_entry(v, t, tiles));
            }
            entries[(size_t) rtp::views_entry(v, tiles, tiles)] = rtp::views_tail_entry_bytes(v, K); // as png_views_sums_kernel's tile 0 does
        }
        uint64_t carry = rtp::views_first_bytes(); // png_views_scan_kernel, one entry at a time
        for (uint64_t i = 0; i < n; ++i) { const uint64_t c = entries[(size_t) i]; entries[(size_t) i] = carry; carry += c; }
        std::vector<uint64_t> start, end, idat, tile, go;
        for (uint64_t v = 0; v < K; ++v) {
            start.push_back(rtp::views_file_start(entries.data(), v, tiles));
            end.push_back(rtp::views_file_end(entries.data(), v, tiles));
            idat.push_back(rtp::views_idat_length(entries.data(), v, tiles, carry));
            for (uint64_t t = 0; t < tiles; ++t) tile.push_back(entries[(size_t) rtp::views_entry(v, t, tiles)]);
        }
        start.push_back(carry);
        for (uint64_t cap : {carry - 1u, carry, carry + 1u}) go.push_back(rtp::views_go(carry, cap, true) ? 1u : 0u);
        go.push_back(rtp::views_go(carry, carry, false) ? 1u : 0u);
        printf("tiles=%llu entries=%llu total=%llu", (unsigned long long) tiles, (unsigned long long) n, (unsigned long long) carry);
        print_list("entry", entry); print_list("start", start); print_list("end", end); print_list("idat", idat); print_list("tile", tile); print_list("go", go);
        printf("\n");
    }
    return 0;
}
