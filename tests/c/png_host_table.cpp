// csrc/rt_png.h alone, driven on a CPU for tests/test_png_host.py (built with -fsanitize=address,undefined): the checksum combiners against
// straight-line CRC-32 and Adler-32 over split buffers, the code builder's Kraft sums and length limits, the canonical codes, the token
// rule and the length symbols.  Every check prints one line "<name> ok" or "<name> FAILED ..."; the exit status is the count of failures.
#include "../../ray-tracing-fsharp_amd/csrc/rt_png.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(name, cond)                                                        \
    do {                                                                          \
        if (!(cond)) { printf("%s FAILED: %s (line %d)\n", name, #cond, __LINE__); ++failures; return; } \
    } while (0)

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static void checksums() {
    const char *check = "123456789"; // the catalogued check values of both sums
    EXPECT("checksums", rtp::crc32_of((const uint8_t *) check, 9) == 0xCBF43926u);
    EXPECT("checksums", rtp::adler32_of((const uint8_t *) check, 9) == 0x091E01DEu);
    EXPECT("checksums", rtp::crc32_of(nullptr, 0) == 0u && rtp::adler32_of(nullptr, 0) == 1u);
    std::vector<uint8_t> buf(70000);
    for (auto &b : buf) b = (uint8_t) rnd();
    for (size_t i = 30000; i < 36000; ++i) buf[i] = 255; // Adler's sums pass the modulus many times
    const size_t sizes[] = {0, 1, 2, 255, 256, 4096, 16384, 16385, 65520, 65521, 65522, 70000};
    for (size_t n : sizes) {
        const uint32_t crc = rtp::crc32_of(buf.data(), n), adler = rtp::adler32_of(buf.data(), n);
        const size_t cuts[] = {0, 1, n / 3, n / 2, n > 0 ? n - 1 : 0, n};
        for (size_t c : cuts) {
            if (c > n) continue;
            EXPECT("checksums", rtp::crc_combine(rtp::crc32_of(buf.data(), c), rtp::crc32_of(buf.data() + c, n - c), n - c) == crc);
            EXPECT("checksums", rtp::adler_combine(rtp::adler32_of(buf.data(), c), rtp::adler32_of(buf.data() + c, n - c), n - c) == adler);
            EXPECT("checksums", rtp::crc32_of(buf.data() + c, n - c, rtp::crc32_of(buf.data(), c)) == crc); // the running form
        }
        // many pieces, combined left to right and as a tree
        uint32_t crc_run = 0u, adler_run = 1u;
        std::vector<uint32_t> pc, pa;
        std::vector<uint64_t> pl;
        for (size_t at = 0; at < n;) {
            const size_t want = 1 + rnd() % 5000, len = want < n - at ? want : n - at;
            crc_run = rtp::crc_combine(crc_run, rtp::crc32_of(buf.data() + at, len), len);
            adler_run = rtp::adler_combine(adler_run, rtp::adler32_of(buf.data() + at, len), len);
            pc.push_back(rtp::crc32_of(buf.data() + at, len)); pa.push_back(rtp::adler32_of(buf.data() + at, len)); pl.push_back(len);
            at += len;
        }
        EXPECT("checksums", crc_run == crc && adler_run == adler);
        for (size_t d = 1; d < pc.size(); d <<= 1)
            for (size_t i = 0; i + d < pc.size(); i += 2 * d) {
                pc[i] = rtp::crc_combine(pc[i], pc[i + d], pl[i + d]); pa[i] = rtp::adler_combine(pa[i], pa[i + d], pl[i + d]); pl[i] += pl[i + d];
            }
        if (!pc.empty()) EXPECT("checksums", pc[0] == crc && pa[0] == adler && pl[0] == n);
    }
    printf("checksums ok\n");
}

// Lengths for `freq`: within the limit, zero exactly where the count is zero, Kraft sum exactly 1, and no rarer symbol with a shorter code.
static bool lengths_hold(const std::vector<uint32_t> &freq, uint32_t max_bits, uint32_t *longest, bool *optimal) {
    const uint32_t n = (uint32_t) freq.size();
    rtp::BuildScratch s;
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (freq[i]) { s.order[rtp::rank_of(freq.data(), n, i)] = (uint16_t) i; ++m; }
    for (uint32_t i = 1; i < m; ++i)
        if (freq[s.order[i - 1]] > freq[s.order[i]] || (freq[s.order[i - 1]] == freq[s.order[i]] && s.order[i - 1] >= s.order[i])) return false;
    std::vector<uint8_t> len(n, 0xEE);
    rtp::build_lengths(freq.data(), n, m, max_bits, s, len.data());
    unsigned long long kraft = 0, cost = 0;
    *longest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if ((len[i] != 0) != (freq[i] != 0) && m != 1) return false;
        if (len[i] > max_bits) return false;
        if (len[i]) kraft += 1ull << (max_bits - len[i]);
        if (len[i] > *longest) *longest = len[i];
        cost += (unsigned long long) freq[i] * len[i];
        for (uint32_t j = 0; j < n; ++j)
            if (freq[i] && freq[j] && freq[i] < freq[j] && len[i] < len[j]) return false;
    }
    if (m >= 1 && kraft != 1ull << max_bits) return false;
    // canonical codes: prefix-free -- reversed back, the codes of equal length rise by one with the symbol, and no code is a prefix of a longer one
    std::vector<uint32_t> code(n);
    rtp::assign_codes(len.data(), n, max_bits, code.data());
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < n; ++j) {
            if (i == j || !len[i] || !len[j] || len[i] > len[j]) continue;
            if ((code[j] & ((1u << len[i]) - 1u)) == code[i]) return false; // stored reversed: a prefix is the low bits
        }
    if (optimal) { // against a plain O(n^2) Huffman cost
        std::vector<unsigned long long> w;
        for (uint32_t f : freq) if (f) w.push_back(f);
        unsigned long long best = 0;
        while (w.size() > 1) {
            size_t a = 0, b = 1;
            if (w[b] < w[a]) std::swap(a, b);
            for (size_t k = 2; k < w.size(); ++k) { if (w[k] < w[a]) { b = a; a = k; } else if (w[k] < w[b]) b = k; }
            const unsigned long long sum = w[a] + w[b];
            best += sum;
            w[a] = sum; w.erase(w.begin() + (long) b);
        }
        *optimal = cost == best || m == 1;
    }
    return true;
}

static void code_builder() {
    uint32_t longest = 0;
    bool optimal = false;
    for (int trial = 0; trial < 300; ++trial) { // random counts, sparse and dense: the limit is not reached, so the code is Huffman's
        std::vector<uint32_t> f(rtp::LL_SYMS, 0u);
        const uint32_t used = 2 + rnd() % 285;
        for (uint32_t k = 0; k < used; ++k) f[rnd() % rtp::LL_USED] = 1 + rnd() % (trial % 2 ? 4000 : 20);
        f[rtp::EOB] = 1;
        EXPECT("code_builder", lengths_hold(f, rtp::LL_MAX_BITS, &longest, &optimal));
        if (longest < rtp::LL_MAX_BITS) EXPECT("code_builder", optimal);
    }
    { // Fibonacci counts 1 (end of block), 1, 2, 3, 5 ...: Huffman's own tree is a chain, 23 symbols -> depth 22
        std::vector<uint32_t> f(rtp::LL_SYMS, 0u);
        uint32_t a = 1, b = 2;
        for (uint32_t i = 0; i < 22; ++i) { f[i * 11] = a; const uint32_t c = a + b; a = b; b = c; }
        f[rtp::EOB] = 1;
        EXPECT("code_builder", lengths_hold(f, rtp::LL_MAX_BITS, &longest, nullptr) && longest == rtp::LL_MAX_BITS);
    }
    { // powers of two: depth 30 without the limit
        std::vector<uint32_t> f(rtp::LL_SYMS, 0u);
        for (uint32_t i = 0; i < 30; ++i) f[i] = 1u << i;
        EXPECT("code_builder", lengths_hold(f, rtp::LL_MAX_BITS, &longest, nullptr) && longest == rtp::LL_MAX_BITS);
    }
    { // all 286 symbols with chain-like counts on top of equal ones
        std::vector<uint32_t> f(rtp::LL_SYMS, 0u);
        for (uint32_t i = 0; i < rtp::LL_USED; ++i) f[i] = 1;
        uint32_t a = 1, b = 2;
        for (uint32_t i = 0; i < 24; ++i) { f[i] = a; const uint32_t c = a + b; a = b; b = c; }
        EXPECT("code_builder", lengths_hold(f, rtp::LL_MAX_BITS, &longest, nullptr) && longest == rtp::LL_MAX_BITS);
    }
    for (int trial = 0; trial < 2000; ++trial) { // the code-length code: 19 symbols, 7 bits, counts skewed enough to pass it often
        std::vector<uint32_t> f(rtp::CL_SYMS, 0u);
        const uint32_t used = 1 + rnd() % 19;
        for (uint32_t k = 0; k < used; ++k) f[rnd() % rtp::CL_SYMS] = 1u << (rnd() % 9);
        if (trial % 3 == 0) { uint32_t a = 1, b = 1; for (uint32_t i = 0; i < 19; ++i) { f[(i * 7) % 19] = a; const uint32_t c = a + b; a = b; b = c; } }
        EXPECT("code_builder", lengths_hold(f, rtp::CL_MAX_BITS, &longest, &optimal));
        if (longest < rtp::CL_MAX_BITS) EXPECT("code_builder", optimal);
    }
    { // one symbol: two codes of length 1, so that the code is complete
        std::vector<uint32_t> f(rtp::CL_SYMS, 0u);
        f[0] = 5;
        rtp::BuildScratch s;
        s.order[0] = 0;
        uint8_t len[rtp::CL_SYMS];
        rtp::build_lengths(f.data(), rtp::CL_SYMS, 1, rtp::CL_MAX_BITS, s, len);
        EXPECT("code_builder", len[0] == 1 && len[1] == 1 && len[2] == 0);
    }
    { // the fixed code is the canonical code of its lengths (RFC 1951 3.2.6)
        uint8_t len[rtp::LL_SYMS];
        uint16_t code[rtp::LL_SYMS];
        for (uint32_t i = 0; i < rtp::LL_SYMS; ++i) len[i] = (uint8_t) rtp::fixed_length(i);
        rtp::assign_codes(len, rtp::LL_SYMS, rtp::LL_MAX_BITS, code);
        auto rev = [](uint32_t c, uint32_t l) { uint32_t r = 0; for (uint32_t k = 0; k < l; ++k) { r = (r << 1) | (c & 1); c >>= 1; } return r; };
        EXPECT("code_builder", rev(code[0], 8) == 0x30 && rev(code[143], 8) == 0xBF && rev(code[144], 9) == 0x190 && rev(code[255], 9) == 0x1FF);
        EXPECT("code_builder", rev(code[256], 7) == 0 && rev(code[279], 7) == 0x17 && rev(code[280], 8) == 0xC0 && rev(code[287], 8) == 0xC7);
    }
    printf("code_builder ok\n");
}

static void token_rule() {
    const uint32_t base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint32_t extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0}; // RFC 1951 3.2.5
    for (uint32_t len = 3; len <= 258; ++len) {
        uint32_t sym, eb, ev;
        rtp::length_symbol(len, sym, eb, ev);
        EXPECT("token_rule", sym >= 257 && sym <= 285 && eb == extra[sym - 257] && base[sym - 257] + ev == len && ev < (1u << eb) + (eb == 0));
        EXPECT("token_rule", rtp::length_extra_bits(sym) == eb);
    }
    for (uint32_t L = 1; L <= 1600; ++L) { // every run: the tokens cover it exactly, greedily, and only a remainder below 3 is literals
        uint32_t covered = 0, k = 0, literals = 0, matches = 0;
        while (k < L) {
            const uint32_t t = rtp::token_at(k, L);
            EXPECT("token_rule", t == 1 || (t >= 3 && t <= 258));
            EXPECT("token_rule", !(t != 1 && k == 0));
            if (t == 1) ++literals; else { ++matches; for (uint32_t q = 1; q < t; ++q) EXPECT("token_rule", rtp::token_at(k + q, L) == 0); }
            covered += t; k += t;
        }
        const uint32_t rest = L - 1, rem = rest % 258;
        EXPECT("token_rule", covered == L && matches == rest / 258 + (rem >= 3) && literals == 1 + (rem < 3 ? rem : 0));
    }
    const uint32_t named[][3] = {{1, 1, 0}, {2, 2, 0}, {3, 3, 0}, {4, 1, 1}, {258, 1, 1}, {259, 1, 1}, {260, 2, 1}, {261, 3, 1}, {262, 1, 2}, {517, 1, 2}}; // L, literals, matches
    for (auto &c : named) {
        uint32_t lit = 0, mat = 0;
        for (uint32_t k = 0; k < c[0]; ++k) { const uint32_t t = rtp::token_at(k, c[0]); lit += t == 1; mat += t >= 3; }
        EXPECT("token_rule", lit == c[1] && mat == c[2]);
    }
    printf("token_rule ok\n");
}

static void sizes_and_container() {
    const uint64_t T = RTO_PNG_TILE_BYTES;
    EXPECT("sizes", rtp::filtered_bytes(2, 3) == 20 && rtp::tile_count(2, 3) == 1 && rtp::max_bytes(2, 3) == 43 + 20 + 5 + 25);
    EXPECT("sizes", rtp::tile_count(1, (T - 1) / 3) == 1 && rtp::tile_count(2, (T - 1) / 3) == 2);
    EXPECT("sizes", rtp::supported(1601, 2401) && rtp::supported(23000, 31000) && !rtp::supported(27000, 27000) && !rtp::supported(1, 0x7fffffffull));
    // one whole file, all stored (random bytes, no gamma): the length is max_bytes, the sums are the straight-line ones
    const uint32_t rows = 37, cols = 211;
    std::vector<uint8_t> rgb(rows * cols * 3), gamma(256), out(rtp::max_bytes(rows, cols) + 8, 0xA5);
    for (auto &b : rgb) b = (uint8_t) rnd();
    for (uint32_t i = 0; i < 256; ++i) gamma[i] = (uint8_t) i;
    const uint64_t len = rtp::format_png(rgb.data(), rows, cols, gamma.data(), out.data());
    EXPECT("sizes", len == rtp::max_bytes(rows, cols) && out[len] == 0xA5);
    const uint64_t idat = len - 43 - 25 + 11;
    EXPECT("sizes", (((uint64_t) out[33] << 24) | (out[34] << 16) | (out[35] << 8) | out[36]) == idat);
    const uint32_t crc = rtp::crc32_of(out.data() + 37, 4 + idat);
    EXPECT("sizes", (((uint32_t) out[37 + 4 + idat] << 24) | (out[38 + 4 + idat] << 16) | (out[39 + 4 + idat] << 8) | out[40 + 4 + idat]) == crc);
    // a flat image: every row a literal, the filter byte and runs of zeros
    std::vector<uint8_t> flat(64 * 64 * 3, 0);
    const uint64_t flat_len = rtp::format_png(flat.data(), 64, 64, gamma.data(), out.data());
    EXPECT("sizes", flat_len * 20 <= 64 * 64 * 3);
    printf("sizes ok\n");
}

int main() {
    checksums();
    code_builder();
    token_rule();
    sizes_and_container();
    return failures;
}
