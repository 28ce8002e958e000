// gif_mixed_plan_test.cpp -- the host side of a mixed-size gif.Encode's per-frame records (imageprocessor_amd/csrc/ipx_gif_mixed_plan.h:
// gif_mix_build, gif_stream_bound, gif_rows_in_flight) held to their rules, the uniform core's arithmetic transcribed beside them, as a
// program of its own: plain g++, no GPU, no runtime.
//   g++ -std=c++17 -fsanitize=address,undefined -o gif_mixed_plan_test tools/gif_mixed_plan_test.cpp && ./gif_mixed_plan_test
// Prints "gif mixed plan ok" and exits 0, or says what broke and exits 1.  tests/test_gif_mixed_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_gif_mixed_plan.h"

using namespace ipx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 50) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the uniform arithmetic, transcribed (ipx_gif.hip before the records: gif_rows_in_flight and gif_encode_core) ----
static int u_rows(int h, int n, bool has_knob, int knob)
{
    int waves = 16;
    if ((h + 63) / 64 < waves) waves = (h + 63) / 64;
    if (2048 / (n > 1 ? n : 1) < waves) waves = 2048 / (n > 1 ? n : 1);
    if (has_knob) waves = knob;
    if (waves > 16) waves = 16;
    if (waves < 1) waves = 1;
    return 64 * waves;
}
static unsigned long long u_bound(int w, int h)
{
    const unsigned long long npix = (unsigned long long)w * h, codes = npix + 3 + npix / 3838 + 1, data = (codes * 12 + 7) / 8;
    return 792 + data + (data + 254) / 255 + 2;   // 13 + 768 + 10 + 1 = 792 header bytes
}

struct Span { unsigned long long lo, hi; };
static void disjoint(const char *name, const char *what, std::vector<Span> v)
{
    std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    for (size_t i = 1; i < v.size(); i++) CHECK(v[i - 1].hi <= v[i].lo, "%s: two %s overlap", name, what);
}

static void check_plan(const char *name, const std::vector<int> &w, const std::vector<int> &h, bool has_knob = false, int knob = 0, int pad = 0)
{
    const int n = (int)w.size();
    std::vector<GifMixSrc> in((size_t)n);
    for (int i = 0; i < n; i++) in[(size_t)i] = GifMixSrc{(const uint8_t *)(uintptr_t)(0x10000 + 4096ull * i + (i % 3) * 4), w[i], h[i], 4 * w[i] + pad};
    GifMixPlan p;
    const bool ok = gif_mix_build(in.data(), n, has_knob, knob, &p);
    CHECK(ok, "%s: refused", name);
    if (!ok) return;
    CHECK((int)p.frames.size() == n && (int)p.dither_order.size() == n && (int)p.lzw_order.size() == n, "%s: sizes", name);
    std::vector<Span> idx, car, reg;
    unsigned long long carry = 0, max_region = 0;
    for (int i = 0; i < n; i++) {
        const GifMixFrame &f = p.frames[(size_t)i];
        CHECK(f.src == in[(size_t)i].src && f.w == w[i] && f.h == h[i] && f.stride == 4 * w[i] + pad, "%s: frame %d is not the caller's", name, i);
        CHECK(f.index_off % 256 == 0 && f.region_off % 256 == 0 && f.region % 256 == 0, "%s: frame %d is not aligned", name, i);
        CHECK(f.region >= u_bound(w[i], h[i]) && f.region < u_bound(w[i], h[i]) + 256, "%s: frame %d region %llu, bound %llu", name, i, f.region, u_bound(w[i], h[i]));
        CHECK(gif_stream_bound(w[i], h[i]) == u_bound(w[i], h[i]), "%s: gif_stream_bound(%d, %d)", name, w[i], h[i]);
        CHECK(f.carry_off == carry, "%s: frame %d carry at %llu, expected %llu", name, i, f.carry_off, carry);   // shares of w each, back to back
        carry += (unsigned long long)w[i];
        CHECK(f.rows == u_rows(h[i], n, has_knob, knob), "%s: frame %d has %d rows in flight, the rule says %d", name, i, f.rows, u_rows(h[i], n, has_knob, knob));
        CHECK(f.rows >= 64 && f.rows <= 1024 && f.rows % 64 == 0, "%s: frame %d rows %d", name, i, f.rows);
        idx.push_back(Span{f.index_off, f.index_off + (unsigned long long)w[i] * h[i]});
        car.push_back(Span{f.carry_off, f.carry_off + (unsigned long long)w[i]});
        reg.push_back(Span{f.region_off, f.region_off + f.region});
        CHECK(idx.back().hi <= p.index_bytes && car.back().hi <= p.carry_int4s && reg.back().hi <= p.region_bytes, "%s: frame %d beyond an arena", name, i);
        if (f.region > max_region) max_region = f.region;
    }
    CHECK(p.carry_int4s == carry && p.max_region == max_region, "%s: totals", name);
    disjoint(name, "index shares", idx);
    disjoint(name, "carry shares", car);
    disjoint(name, "regions", reg);
    // the launch orders are permutations
    for (const std::vector<uint32_t> *o : {&p.dither_order, &p.lzw_order}) {
        std::vector<int> seen((size_t)n, 0);
        for (uint32_t f : *o) { CHECK(f < (uint32_t)n, "%s: order names frame %u", name, f); if (f < (uint32_t)n) seen[f]++; }
        for (int i = 0; i < n; i++) CHECK(seen[(size_t)i] == 1, "%s: frame %d is in an order %d times", name, i, seen[(size_t)i]);
    }
    // the buckets partition the dither order: consecutive, ascending rows, every frame of a bucket with the bucket's rows, costliest first
    int at = 0, last_rows = 0;
    CHECK(p.buckets.size() <= 16, "%s: %zu buckets", name, p.buckets.size());
    for (const GifMixBucket &b : p.buckets) {
        CHECK(b.first == at && b.n >= 1 && b.rows > last_rows, "%s: bucket of %d rows at %d (expected %d), %d frames", name, b.rows, b.first, at, b.n);
        for (int q = b.first; q < b.first + b.n && q < n; q++) {
            const GifMixFrame &f = p.frames[p.dither_order[(size_t)q]];
            CHECK(f.rows == b.rows, "%s: frame of %d rows in the bucket of %d", name, f.rows, b.rows);
            if (q > b.first) CHECK(gif_mix_dither_steps(p.frames[p.dither_order[(size_t)q - 1]]) >= gif_mix_dither_steps(f), "%s: bucket of %d rows is not costliest first", name, b.rows);
        }
        at += b.n;
        last_rows = b.rows;
    }
    CHECK(at == n, "%s: the buckets hold %d of %d frames", name, at, n);
    for (int q = 1; q < n; q++) {
        const GifMixFrame &a = p.frames[p.lzw_order[(size_t)q - 1]], &b = p.frames[p.lzw_order[(size_t)q]];
        CHECK((unsigned long long)a.w * a.h >= (unsigned long long)b.w * b.h, "%s: the LZW order is not longest first at %d", name, q);
    }
}

int main()
{
    // the named edges
    check_plan("one pixel", {1}, {1});
    check_plan("test sizes", {1, 2, 1, 3, 64, 17, 257, 3, 5, 3, 5, 3, 97}, {1, 1, 2, 3, 64, 241, 1, 63, 64, 65, 129, 1025, 131});
    check_plan("test sizes, padded", {1, 2, 1, 3, 64, 17, 257, 3, 5, 3, 5, 3, 97}, {1, 1, 2, 3, 64, 241, 1, 63, 64, 65, 129, 1025, 131}, false, 0, 12);
    check_plan("one wave each", {7, 9, 11, 13, 15}, {63, 64, 65, 129, 130}, true, 1);
    check_plan("knob 0", {7, 9}, {63, 2000}, true, 0);
    check_plan("knob 99", {7, 9}, {63, 2000}, true, 99);
    check_plan("knob -3", {7, 9}, {63, 2000}, true, -3);
    check_plan("largest sides", {65535, 1, 65535}, {1, 65535, 2});
    check_plan("every bucket", {3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3}, {1, 65, 129, 193, 257, 321, 385, 449, 513, 577, 641, 705, 769, 833, 897, 961, 5000});
    {   // 65535 frames of 65535 x 1: the totals stay exact in 64 bits
        const int n = 65535;
        std::vector<int> w((size_t)n, 65535), h((size_t)n, 1);
        check_plan("65535 x (65535 x 1)", w, h);
        std::vector<GifMixSrc> in((size_t)n, GifMixSrc{(const uint8_t *)(uintptr_t)0x10000, 65535, 1, 4 * 65535});
        GifMixPlan p;
        CHECK(gif_mix_build(in.data(), n, false, 0, &p), "65535 frames refused");
        CHECK(p.carry_int4s == 65535ull * 65535ull, "carry total %llu", p.carry_int4s);
        CHECK(p.index_bytes == 65535ull * 65536ull, "index total %llu", p.index_bytes);
        CHECK(p.region_bytes == 65535ull * ((u_bound(65535, 1) + 255) / 256 * 256) && p.region_bytes > 0xffffffffull, "region total %llu", p.region_bytes);
        CHECK(p.buckets.size() == 1 && p.buckets[0].rows == 64 && p.buckets[0].n == n, "65535 frames: buckets");
    }
    {   // refusals, and n == 0
        GifMixPlan p;
        const uint8_t *s = (const uint8_t *)(uintptr_t)0x10000;
        const GifMixSrc bad[] = {{s, 0, 4, 16}, {s, 4, 0, 16}, {s, 65536, 1, 4 * 65536}, {s, 1, 65536, 4}, {s, 4, 4, 12}, {s, -1, 4, 16}};
        for (const GifMixSrc &b : bad) {
            const GifMixSrc two[2] = {{s, 4, 4, 16}, b};
            CHECK(!gif_mix_build(two, 2, false, 0, &p), "a %d x %d frame of stride %d was taken", b.w, b.h, b.stride);
        }
        CHECK(gif_mix_build(nullptr, 0, false, 0, &p) && p.frames.empty() && p.buckets.empty(), "n == 0");
    }
    // seeded lists
    std::mt19937 rng(20240917);
    for (int t = 0; t < 3000; t++) {
        const int n = 1 + (int)(rng() % (t % 10 == 0 ? 300 : 24));
        std::vector<int> w((size_t)n), h((size_t)n);
        for (int i = 0; i < n; i++) {
            const int kind = (int)(rng() % 8);
            w[(size_t)i] = kind == 0 ? 1 : kind == 1 ? 1 + (int)(rng() % 65535) / (1 + (int)(rng() % 64)) : 1 + (int)(rng() % 1500);
            h[(size_t)i] = kind == 2 ? 1 : kind == 3 ? 1 + (int)(rng() % 65535) / (1 + (int)(rng() % 64)) : 1 + (int)(rng() % 1500);
        }
        const bool has_knob = t % 7 == 3;
        char name[32];
        snprintf(name, sizeof name, "seeded %d", t);
        check_plan(name, w, h, has_knob, has_knob ? (int)(rng() % 20) - 2 : 0, t % 5 == 0 ? 12 : 0);
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("gif mixed plan ok\n");
    return 0;
}
