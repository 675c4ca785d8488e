// csrc/rt_jpeg.h alone, on a CPU: hand-computed tables of the sample arithmetic, then the WHOLE subsequence algorithm of the device route
// (rtj::decode_host with S > 0: the synchronising rounds as a loop over subsequences, the same step function, the placing run behind its
// checks) over every case of a case file, against the sequential decode and the fixture.  Built plainly and with
// -fsanitize=address,undefined by tests/test_jpeg_host.py: the memory-safety check of the device code's logic.
//
// Case file (written by the test from tests/golden/jpeg_cases.npz): u32 count, then per case u32 name length, name, u32 kind (0: decodes,
// 1: refused, 2: decodes, and is cut at every length), u32 jpeg length, jpeg, u32 rgb length, rgb.
#include "../../ray-tracing-fsharp_amd/csrc/rt_jpeg.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static const uint32_t SIZES[] = {0u, 4u, 8u, 64u, (uint32_t) RTJ_DEFAULT_SUBSEQUENCE};

static uint8_t dc_only_sample(int32_t dc_times_q) {
    int16_t coef[64] = {0};
    uint16_t q[64];
    for (int k = 0; k < 64; ++k) q[k] = 1;
    uint8_t out[64];
    rtj::idct_block(coef, dc_times_q, q, out, 8);
    for (int i = 1; i < 64; ++i) CHECK(out[i] == out[0]); // a flat block
    return out[0];
}

static void tables() {
    // a DC-only block: pass 1 gives 4 * dc down column 0 .. 7, pass 2 (dc + 4) >> 3; the sample is that + 128, clamped
    CHECK(dc_only_sample(0) == 128 && dc_only_sample(8) == 129 && dc_only_sample(-8) == 127 && dc_only_sample(3) == 128 && dc_only_sample(4) == 129);
    CHECK(dc_only_sample(-5) == 127 && dc_only_sample(1016) == 255 && dc_only_sample(1008) == 254 && dc_only_sample(-1024) == 0 && dc_only_sample(-1016) == 1);
    CHECK(dc_only_sample(2047 * 16) == 255 && dc_only_sample(-2047 * 16) == 0); // the extremes of a DC sum at quantiser 16, through the clamp
    { // every coefficient at the extremes of its 16 bits times the largest quantiser: the arithmetic wraps, nothing else
        int16_t coef[64];
        uint16_t q[64];
        uint8_t out[64];
        for (int sign = -1; sign <= 1; sign += 2) {
            for (int k = 0; k < 64; ++k) { coef[k] = (int16_t) (sign * 32767); q[k] = 255; }
            rtj::idct_block(coef, sign * 32767, q, out, 8); // (nothing to hold it to: libjpeg's int wraps the same way)
        }
    }
    { // the largest AC coefficient that does not wrap, at row 0, column 1: a half cosine along every row, through both clamps
        int16_t coef[64] = {0};
        uint16_t q[64];
        for (int k = 0; k < 64; ++k) q[k] = 1;
        uint8_t out[64];
        for (int sign = -1; sign <= 1; sign += 2) {
            coef[1] = (int16_t) (sign * 2047); // 2047 * 1.387 / 8 = 355 at column 0, its negative at column 7
            rtj::idct_block(coef, 0, q, out, 8);
            for (int r = 0; r < 8; ++r) {
                CHECK(out[8 * r] == (sign > 0 ? 255 : 0) && out[8 * r + 7] == (sign > 0 ? 0 : 255));
                for (int c = 1; c < 8; ++c) CHECK(sign > 0 ? out[8 * r + c] <= out[8 * r + c - 1] : out[8 * r + c] >= out[8 * r + c - 1]);
            }
        }
    }
    { // one AC coefficient: zig-zag index 1 is row 0, column 1 -- the block varies along a row and not down a column
        int16_t coef[64] = {0};
        uint16_t q[64];
        for (int k = 0; k < 64; ++k) q[k] = 1;
        coef[1] = 100;
        uint8_t out[64];
        rtj::idct_block(coef, 0, q, out, 8);
        for (int r = 1; r < 8; ++r) CHECK(std::memcmp(out, out + 8 * r, 8) == 0);
        CHECK(out[0] > 128 && out[3] > 128 && out[4] < 128 && out[7] < 128 && out[0] > out[3]);
    }
    // the colour formulas at corners of the (Y, Cb, Cr) cube, by hand
    rtj::Frame f{};
    f.W = f.H = 1; f.ncomp = 3; f.cls = rtj::S444;
    for (int c = 0; c < 3; ++c) { f.pw[c] = 8; f.cw[c] = f.ch[c] = 1; f.plane_at[c] = 64u * (uint32_t) c; }
    // x = Cb - 128, y = Cr - 128 are -128 or 127: (91881 y + 32768) >> 16 = -179 / 178, (116130 x + 32768) >> 16 = -227 / 225,
    // (-22554 x - 46802 y + 32768) >> 16 = 135 (x, y low), -47 (x low, y high), 48 (x high, y low), -134 (both high)
    static const uint8_t ycc[9][3] = {{0, 0, 0}, {0, 0, 255}, {0, 255, 0}, {0, 255, 255}, {255, 0, 0}, {255, 0, 255}, {255, 255, 0}, {255, 255, 255}, {128, 128, 128}};
    static const uint8_t want[9][3] = {{0, 135, 0}, {178, 0, 0}, {0, 48, 225}, {178, 0, 225}, {76, 255, 28}, {255, 208, 28}, {76, 255, 255}, {255, 121, 255}, {128, 128, 128}};
    for (int i = 0; i < 9; ++i) {
        uint8_t planes[192] = {0}, rgb[3];
        for (int c = 0; c < 3; ++c) planes[64 * c] = ycc[i][c];
        rtj::pixel_rgb(f, planes, 0, 0, rgb);
        CHECK(rgb[0] == want[i][0] && rgb[1] == want[i][1] && rgb[2] == want[i][2]);
    }
    f.ncomp = 1; // greyscale: R = G = B = Y
    { uint8_t planes[64] = {201}, rgb[3]; rtj::pixel_rgb(f, planes, 0, 0, rgb); CHECK(rgb[0] == 201 && rgb[1] == 201 && rgb[2] == 201); }
    // the triangle filters on planes 1 and 2 samples wide, by hand
    rtj::Frame g{};
    g.pw[1] = 8;
    const uint8_t one[64] = {77}, two[64] = {10, 50, 0, 0, 0, 0, 0, 0, 90, 130};
    g.cls = rtj::S422; g.cw[1] = 1; g.ch[1] = 1;
    CHECK(rtj::chroma_at(g, one, 1, 0, 0) == 77 && rtj::chroma_at(g, one, 1, 1, 0) == 77);
    g.cw[1] = 2;
    { const uint32_t w[4] = {10, 20, 40, 50}; for (uint32_t x = 0; x < 4; ++x) CHECK(rtj::chroma_at(g, two, 1, x, 0) == w[x]); }
    g.cls = rtj::S420; g.cw[1] = 1; g.ch[1] = 1;
    for (uint32_t y = 0; y < 2; ++y) for (uint32_t x = 0; x < 2; ++x) CHECK(rtj::chroma_at(g, one, 1, x, y) == 77);
    g.cw[1] = 2; g.ch[1] = 2;
    {
        const uint32_t w[4][4] = {{10, 20, 40, 50}, {30, 40, 60, 70}, {70, 80, 100, 110}, {90, 100, 120, 130}};
        for (uint32_t y = 0; y < 4; ++y) for (uint32_t x = 0; x < 4; ++x) CHECK(rtj::chroma_at(g, two, 1, x, y) == w[y][x]);
    }
    // extra bits, and the 32 bits at a bit position with the end of the data inside them
    CHECK(rtj::extend(0, 0) == 0 && rtj::extend(1, 1) == 1 && rtj::extend(0, 1) == -1 && rtj::extend(5, 3) == 5 && rtj::extend(2, 3) == -5 && rtj::extend(0, 11) == -2047);
    const uint8_t bytes[3] = {0x12, 0x34, 0x56};
    CHECK(rtj::window(bytes, 3, 0) == 0x123456FFu && rtj::window(bytes, 3, 4) == 0x23456FFFu && rtj::window(bytes, 3, 23) == 0x7FFFFFFFu && rtj::window(bytes, 3, 24) == 0xFFFFFFFFu);
    std::printf("tables ok\n");
}

struct Case { std::string name; uint32_t kind; std::vector<uint8_t> jpeg, rgb; };

static uint32_t read_u32(FILE *f) { uint32_t v = 0; CHECK(std::fread(&v, 4, 1, f) == 1); return v; }
static std::vector<uint8_t> read_bytes(FILE *f) {
    std::vector<uint8_t> v(read_u32(f));
    if (!v.empty()) CHECK(std::fread(v.data(), 1, v.size(), f) == v.size());
    return v;
}

// One file under every subsequence size: the same status, the same text, the same bitmap -- and an untouched buffer when refused.  The
// file is handed over in an allocation of exactly its length, so a read behind it is the sanitizer's to report.
static int all_sizes(const uint8_t *data, size_t n, size_t cap, std::vector<uint8_t> &rgb, std::string &text) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(exact.get(), data, n);
    int status = -1;
    for (uint32_t S : SIZES) {
        std::vector<uint8_t> out(cap, (uint8_t) 0xA5);
        std::string err;
        int64_t plan[8] = {0};
        const int rc = rtj::decode_host(exact.get(), n, out.data(), cap, S, plan, err);
        if (rc != rtj::OK) for (uint8_t b : out) CHECK(b == 0xA5);
        if (rc == rtj::OK || plan[1]) CHECK(plan[2] <= plan[1] && (plan[1] == 0 || plan[2] >= 1)); // rounds <= subsequences, always
        if (status < 0) { status = rc; rgb = out; text = err; }
        else CHECK(rc == status && out == rgb && err == text);
    }
    return status;
}

int main(int argc, char **argv) {
    tables();
    if (argc < 2) return 0;
    FILE *f = std::fopen(argv[1], "rb");
    CHECK(f != nullptr);
    std::vector<Case> cases(read_u32(f));
    for (Case &c : cases) {
        const std::vector<uint8_t> name = read_bytes(f);
        c.name.assign(name.begin(), name.end());
        c.kind = read_u32(f);
        c.jpeg = read_bytes(f);
        c.rgb = read_bytes(f);
    }
    std::fclose(f);
    std::vector<uint8_t> rgb;
    std::string text;
    size_t decoded = 0, refused = 0, prefixes = 0, most_rounds = 0;
    for (const Case &c : cases) {
        if (c.kind == 1u) {
            const int rc = all_sizes(c.jpeg.data(), c.jpeg.size(), 40 * 56 * 3, rgb, text);
            CHECK(rc == rtj::INVALID || rc == rtj::UNSUPPORTED);
            std::printf("refused %s %d %s\n", c.name.c_str(), rc, text.c_str());
            ++refused;
            continue;
        }
        CHECK(all_sizes(c.jpeg.data(), c.jpeg.size(), c.rgb.size(), rgb, text) == rtj::OK);
        if (rgb != c.rgb) { std::fprintf(stderr, "%s: the decode differs from the fixture\n", c.name.c_str()); return 1; }
        { // how many rounds the loop took at 64 bytes
            std::string err;
            int64_t plan[8];
            CHECK(rtj::decode_host(c.jpeg.data(), c.jpeg.size(), rgb.data(), rgb.size(), 64u, plan, err) == rtj::OK);
            if ((size_t) plan[2] > most_rounds) most_rounds = (size_t) plan[2];
            if (c.name == "noise-40x56-444-q95-r0") std::printf("rounds %s %lld of %lld\n", c.name.c_str(), (long long) plan[2], (long long) plan[1]);
        }
        ++decoded;
        if (c.kind == 2u)
            for (size_t n = 0; n < c.jpeg.size(); ++n, ++prefixes) (void) all_sizes(c.jpeg.data(), n, c.rgb.size(), rgb, text);
    }
    std::printf("most rounds at 64 bytes: %zu\n", most_rounds);
    std::printf("cases ok %zu refusals ok %zu prefixes ok %zu\n", decoded, refused, prefixes);
    return 0;
}
