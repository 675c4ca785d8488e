// csrc/rt_texture_plan.h alone, on a CPU: the layout of the texel blob against a literal restatement of the loop the host texture half
// used to run, rtt::source_index (and its stepped form) over EVERY destination byte against rows copied one by one, and the per-lane
// function of of_image_kernel (rtt::place_unit, the same inline function the kernel calls) over whole blobs against the blob
// rth::build_textures makes from the host's reversed rows.  Every source bitmap and every blob is a heap block of exactly its size, so
// under -fsanitize=address a read or a write one byte outside is a report.  Built plainly, with the sanitizers, and once per
// RTX_MUTANT_* (which must make it fail) by tests/test_texture_plan_cpp.py.
#include "../../ray-tracing-fsharp_amd/csrc/rt_scene.h"
#include "../../ray-tracing-fsharp_amd/csrc/rt_texture_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Size { int32_t w, h; };
static const Size SIZES[] = {{1, 1}, {1, 5}, {5, 1}, {17, 9}, {64, 33}};
static const int NSIZES = 5;

static uint8_t noise(uint64_t i, uint64_t salt) { // every row differs
    uint64_t x = (i + 1u) * 0x9E3779B97F4A7C15ull + salt * 0xD1B54A32D192ED03ull;
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
    return (uint8_t) x;
}

// a table of n records: every third one an image (sizes in turn), the others Colour / UvRamp / Checkered over smaller indices
static void make_table(size_t n, std::vector<int32_t> &kind, std::vector<int32_t> &w, std::vector<int32_t> &h) {
    kind.assign(n, RT_TEXTURE_COLOUR); w.assign(n, 0); h.assign(n, 0);
    int next = 0;
    for (size_t i = 0; i < n; ++i) {
        if (n == 1 || i % 3 == 0) { kind[i] = RT_TEXTURE_IMAGE; w[i] = SIZES[next % NSIZES].w; h[i] = SIZES[next % NSIZES].h; ++next; }
        else if (i % 3 == 1) kind[i] = RT_TEXTURE_UV_RAMP;
        else kind[i] = i >= 2 ? RT_TEXTURE_CHECKERED : RT_TEXTURE_COLOUR;
    }
}

static void layout_tables() {
    const size_t counts[] = {0, 1, 254};
    for (size_t n : counts) {
        std::vector<int32_t> kind, w, h;
        make_table(n, kind, w, h);
        // the old loop, literally: texel_off = blob.size(); append width*height*3 bytes; pad with 0 to a multiple of 16
        std::vector<uint8_t> blob;
        std::vector<uint64_t> want(n, rtt::NO_BYTE);
        for (size_t i = 0; i < n; ++i) {
            if (kind[i] != RT_TEXTURE_IMAGE) continue;
            const size_t bytes = (size_t) w[i] * (size_t) h[i] * 3u;
            want[i] = blob.size();
            blob.insert(blob.end(), bytes, (uint8_t) 1);
            while (blob.size() % 16u) blob.push_back(0);
        }
        std::vector<uint64_t> off(n ? n : 1);
        CHECK(rtt::texel_layout(kind.data(), w.data(), h.data(), n, RT_TEXTURE_IMAGE, off.data()) == blob.size());
        for (size_t i = 0; i < n; ++i) CHECK(off[i] == want[i]);
    }
    std::puts("layout ok");
}

static void source_index_tables() {
    for (const Size &sz : SIZES)
        for (int top = 0; top < 2; ++top) {
            const size_t row = (size_t) sz.w * 3u, bytes = row * (size_t) sz.h, padded = (size_t) rtt::padded_bytes(sz.w, sz.h);
            CHECK(padded % 16u == 0 && padded >= bytes && padded - bytes < 16u);
            std::vector<uint64_t> iota(bytes), ref(bytes);
            for (size_t i = 0; i < bytes; ++i) iota[i] = i;
            for (int32_t y = 0; y < sz.h; ++y) // the reference: row y of the texels is the bitmap's row h-1-y (top first) or y
                memcpy(&ref[(size_t) y * row], &iota[(size_t) (top ? sz.h - 1 - y : y) * row], row * sizeof(uint64_t));
            for (size_t b = 0; b < padded; ++b) {
                const uint64_t got = rtt::source_index(sz.w, sz.h, top != 0, b);
                if (b < bytes) CHECK(got == ref[b] && got < bytes);
                else CHECK(got == rtt::NO_BYTE);
            }
            for (size_t start = 0; start < padded; start += 16u) { // the stepped form from every unit boundary
                rtt::SourceCursor c = rtt::cursor_at(sz.w, sz.h, top != 0, start);
                for (size_t b = start; b < start + 16u; ++b) {
                    if (b < bytes) CHECK(c.left == bytes - b && c.src == ref[b]);
                    else CHECK(c.left == 0u);
                    rtt::cursor_next(c);
                }
            }
        }
    std::puts("source_index ok");
}

static void find_image_tables() {
    const uint64_t offs[] = {0, 16, 32, 96, 560};
    CHECK(rtt::find_image(offs, 5, 0) == 0 && rtt::find_image(offs, 5, 15) == 0 && rtt::find_image(offs, 5, 16) == 1 && rtt::find_image(offs, 5, 31) == 1);
    CHECK(rtt::find_image(offs, 5, 32) == 2 && rtt::find_image(offs, 5, 95) == 2 && rtt::find_image(offs, 5, 96) == 3 && rtt::find_image(offs, 5, 559) == 3);
    CHECK(rtt::find_image(offs, 5, 560) == 4 && rtt::find_image(offs, 5, 1u << 30) == 4 && rtt::find_image(offs + 1, 4, 15) == -1 && rtt::find_image(offs, 0, 7) == -1);
    std::puts("find_image ok");
}

// The whole blob through place_unit, lane by lane, against rth::build_textures' blob.  Image k of the table: k % 3 == 0 from a "device"
// bitmap top first, == 1 from one that is already reversed, == 2 host-sourced (its range is not the kernel's: prefilled, must stay).
static void blob_tables() {
    const size_t counts[] = {0, 1, 254};
    for (size_t n : counts) {
        std::vector<int32_t> kind, w, h;
        make_table(n, kind, w, h);
        std::vector<rt_texture> tex(n ? n : 1);
        std::vector<std::unique_ptr<uint8_t[]>> bitmaps(n), texels(n); // exact-size heap blocks
        for (size_t i = 0; i < n; ++i) {
            rt_texture &t = tex[i];
            memset(&t, 0, sizeof(t));
            t.kind = (uint32_t) kind[i]; t.even = t.odd = -1; t.map_radius = 1.0;
            if (kind[i] == RT_TEXTURE_CHECKERED) { t.even = (int32_t) i - 1; t.odd = (int32_t) i - 2; t.grid_size = 3.0; }
            if (kind[i] != RT_TEXTURE_IMAGE) continue;
            t.width = w[i]; t.height = h[i];
            const size_t row = (size_t) w[i] * 3u, bytes = row * (size_t) h[i];
            bitmaps[i].reset(new uint8_t[bytes]);
            texels[i].reset(new uint8_t[bytes]);
            for (size_t b = 0; b < bytes; ++b) bitmaps[i][b] = noise(b, i);
            for (int32_t y = 0; y < h[i]; ++y) memcpy(&texels[i][(size_t) y * row], &bitmaps[i][(size_t) (h[i] - 1 - y) * row], row); // ofImage on the host
            t.texels = texels[i].get();
        }
        rth::HostScene host;
        int status = -1;
        const std::string msg = rth::build_textures(n ? tex.data() : nullptr, n, host, status);
        CHECK(status == RT_OK && msg.empty() && host.texelBytes == host.texelBlob.size());
        {   // the texture half itself against the loop it used to run: the same bytes, the same offsets
            std::vector<uint8_t> old;
            for (size_t i = 0; i < n; ++i) {
                if (kind[i] != RT_TEXTURE_IMAGE) { CHECK(host.texRecs[i].texel_off == 0u); continue; }
                CHECK(host.texRecs[i].texel_off == (uint32_t) old.size());
                old.insert(old.end(), tex[i].texels, tex[i].texels + (size_t) w[i] * (size_t) h[i] * 3u);
                while (old.size() % 16u) old.push_back(0);
            }
            CHECK(old == host.texelBlob);
        }
        // the table as the create calls build it
        std::vector<rtt::ImageEntry> entries;
        std::vector<uint64_t> offsets;
        const size_t total = host.texelBlob.size();
        std::unique_ptr<uint8_t[]> blob(new uint8_t[total ? total : 1]);
        memset(blob.get(), 0xA5, total ? total : 1);
        size_t k = 0;
        for (size_t i = 0; i < n; ++i) {
            if (kind[i] != RT_TEXTURE_IMAGE) continue;
            rtt::ImageEntry e{};
            e.off = host.texRecs[i].texel_off; e.width = w[i]; e.height = h[i];
            if (k % 3 == 0) { e.src = bitmaps[i].get(); e.flags = RTX_FROM_DEVICE | RTX_TOP_FIRST; }
            else if (k % 3 == 1) { e.src = texels[i].get(); e.flags = RTX_FROM_DEVICE; }
            else memcpy(blob.get() + e.off, host.texelBlob.data() + e.off, (size_t) rtt::padded_bytes(w[i], h[i])); // host-sourced: uploaded
            entries.push_back(e);
            offsets.push_back(e.off);
            ++k;
        }
        for (size_t at = 0; at < total; at += 16u) { // one lane per unit
            uint8_t out[16];
            uint32_t valid = 99u;
            const bool mine = rtt::place_unit(offsets.data(), entries.data(), (uint32_t) entries.size(), at, out, &valid);
            const int32_t img = rtt::find_image(offsets.data(), (uint32_t) offsets.size(), at);
            CHECK(img >= 0 && mine == ((entries[(size_t) img].flags & RTX_FROM_DEVICE) != 0u));
            if (!mine) continue;
            const uint64_t end = entries[(size_t) img].off + rtt::image_bytes(entries[(size_t) img].width, entries[(size_t) img].height);
            CHECK(valid == (at + 16u <= end ? 16u : (uint32_t) (end > at ? end - at : 0u)));
            memcpy(blob.get() + at, out, 16);
        }
        CHECK(total == 0 || memcmp(blob.get(), host.texelBlob.data(), total) == 0);
        uint8_t out[16];
        uint32_t valid = 0;
        CHECK(!rtt::place_unit(offsets.data(), entries.data(), (uint32_t) entries.size(), total, out, &valid) || entries.empty()); // beyond the blob
    }
    std::puts("blob ok");
}

int main() {
    layout_tables();
    source_index_tables();
    find_image_tables();
    blob_tables();
    return 0;
}
