// jpeg_enc_mixed_plan_test.cpp -- the host side of a mixed-size jpeg.Encode's per-frame records (imageprocessor_amd/csrc/
// ipx_jpeg_enc_mixed_plan.h: jpeg_enc_build, jpeg_enc_place_scans, jpeg_enc_place_streams, jpeg_enc_find) held to a transcription of the
// uniform encoder's arithmetic (jpeg_encode_sets, launch_jpeg_fdct and the entropy launches), and the scan-length rule of both encode
// cores (jpeg_scan_limit, jpeg_scan_too_long) and the rounding rules (ipx_align.h) held to theirs, as a program of its own: plain g++,
// no GPU, no runtime.
//   g++ -std=c++17 -fsanitize=address,undefined -o jpeg_enc_mixed_plan_test tools/jpeg_enc_mixed_plan_test.cpp && ./jpeg_enc_mixed_plan_test
// Prints "jpeg enc mixed plan ok" and exits 0, or says what broke and exits 1.  tests/test_jpeg_enc_mixed_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_jpeg_enc_mixed_plan.h"

using namespace ipx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 50) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the uniform arithmetic, transcribed ----
// fdct_rgba8: a.mcus_per_frame; jpeg_encode_sets: nblk = ipx_jpeg_coef_count * 2 / 128, coef_count = mcus * 384
static long long u_mcus(int w, int h) { return (long long)((w + 15) / 16) * ((h + 15) / 16); }
static long long u_nblk(int w, int h) { return u_mcus(w, h) * 384 * 2 / 128; }
// launch_jpeg_fdct: grid((mw + 8 - 1) / 8, mh, n)
static long long u_fdct_x(int w) { return (((w + 15) >> 4) + 8 - 1) / 8; }
static long long u_fdct_y(int h) { return (h + 15) >> 4; }
// launch_jpeg_dclen / launch_jpeg_bits: grid((nblk + 255) / 256, n)
static long long u_blk_wgs(int w, int h) { return (u_nblk(w, h) + 255) / 256; }
// fdct_rgba8's aligned16 for one frame
static int u_aligned(const uint8_t *src, int stride) { return ((((uintptr_t)src) | (uintptr_t)stride) & 15) == 0; }

static std::vector<JpegEncSrc> frames_of(const std::vector<int> &w, const std::vector<int> &h, int pad = 0, uintptr_t base = 0x10000)
{
    std::vector<JpegEncSrc> f(w.size());
    for (size_t i = 0; i < w.size(); i++) f[i] = JpegEncSrc{(const uint8_t *)(base + 4096 * i), (int16_t *)(uintptr_t)(0x40000000 + 256 * i), w[i], h[i], 4 * w[i] + pad};
    return f;
}

struct Probe { const char *name; uint32_t JpegEncFrame::*first; };
static const Probe kGrids[] = {{"transform", &JpegEncFrame::wg_fdct}, {"block", &JpegEncFrame::wg_blk}, {"chunk", &JpegEncFrame::wg_chunk}};

// every rule of the records, for any sizes; every_wg: walk every workgroup of every grid through the search (else the ends of each frame)
static void check_records(const char *name, const std::vector<int> &w, const std::vector<int> &h, bool every_wg, unsigned seed = 1)
{
    const int n = (int)w.size();
    const std::vector<JpegEncSrc> in = frames_of(w, h, seed % 3 == 0 ? 4 : 0, seed % 2 ? 0x10000 : 0x10004);
    std::vector<JpegEncFrame> g;
    JpegEncTotals t;
    const bool ok = jpeg_enc_build(in.data(), n, &g, &t);
    CHECK(ok, "%s: refused", name);
    if (!ok) return;
    CHECK((int)g.size() == n, "%s: %zu records for %d frames", name, g.size(), n);
    unsigned long long mcus = 0, fw = 0, bw = 0;
    for (int i = 0; i < n; i++) {
        const JpegEncFrame &r = g[i];
        CHECK(r.src == in[i].src && r.coefs == in[i].coefs && r.w == w[i] && r.h == h[i] && r.stride == in[i].stride, "%s: frame %d is not the caller's", name, i);
        CHECK(r.aligned16 == u_aligned(in[i].src, in[i].stride), "%s: frame %d aligned16 is %d", name, i, r.aligned16);
        CHECK(r.mw == (w[i] + 15) / 16 && r.mcus == u_mcus(w[i], h[i]) && (long long)r.mcus * 6 == u_nblk(w[i], h[i]), "%s: frame %d has %d MCUs", name, i, r.mcus);
        CHECK(r.wgs_per_row == u_fdct_x(w[i]) && r.wgs_per_row >= 1, "%s: frame %d workgroups per row", name, i);
        CHECK(r.mcu_base == mcus, "%s: frame %d starts at MCU %llu, expected %llu", name, i, r.mcu_base, mcus);
        CHECK(r.wg_fdct == fw && r.wg_blk == bw, "%s: frame %d starts at workgroups %u and %u, expected %llu and %llu", name, i, r.wg_fdct, r.wg_blk, fw, bw);
        mcus += (unsigned long long)u_mcus(w[i], h[i]);
        fw += (unsigned long long)(u_fdct_x(w[i]) * u_fdct_y(h[i]));
        bw += (unsigned long long)u_blk_wgs(w[i], h[i]);
    }
    CHECK(t.mcus == mcus && t.fdct_wgs == fw && t.blk_wgs == bw, "%s: totals", name);
    // scans of seeded lengths: a frame's bytes, chunks and places, as jpeg_encode_sets computes them for that frame
    std::mt19937_64 rng(seed);
    std::vector<unsigned long long> bits(n);
    for (int i = 0; i < n; i++) bits[i] = i % 5 == 0 ? 8 * 64 * (1 + rng() % 600) : 1 + rng() % (200ull * g[i].mcus * 6);   // (whole chunks every fifth)
    CHECK(jpeg_enc_place_scans(bits.data(), n, &g, &t), "%s: scans refused", name);
    unsigned long long ub = 0, ch = 0, cw = 0;
    for (int i = 0; i < n; i++) {
        const JpegEncFrame &r = g[i];
        const uint32_t ubytes = (uint32_t)((bits[i] + 7) / 8);
        const uint32_t max_chunks = (ubytes + 64 - 1) / 64;           // jpeg_encode_sets: (umax + chunk - 1) / chunk, of this frame alone
        CHECK(r.ubytes == ubytes && r.nchunks == max_chunks, "%s: frame %d has %u bytes in %u chunks", name, i, r.ubytes, r.nchunks);
        CHECK(r.ubase == ub && r.ubase % 256 == 0 && r.ff0 == ch && r.wg_chunk == cw, "%s: frame %d scan placement", name, i);
        ub += ((unsigned long long)ubytes + 8 + 255) & ~255ull;       // align256(ubytes + 8)
        ch += max_chunks;
        cw += (max_chunks + 255) / 256;                               // launch_jpeg_ffcount: grid((max_chunks + 255) / 256, n)
    }
    CHECK(t.ubytes == ub && t.chunks == ch && t.chunk_wgs == cw, "%s: scan totals", name);
    // streams: header + scan + 0xff count + EOI, every stream 16-byte aligned
    std::vector<uint32_t> ff(n);
    std::vector<size_t> offs(n), lens(n);
    for (int i = 0; i < n; i++) ff[i] = (uint32_t)(rng() % (g[i].ubytes + 1));
    const unsigned long long total = jpeg_enc_place_streams(ff.data(), n, 589, &g, offs.data(), lens.data());
    unsigned long long at = 0;
    for (int i = 0; i < n; i++) {
        CHECK(lens[i] == 589 + (size_t)g[i].ubytes + ff[i] + 2 && offs[i] == at && g[i].obase == at && at % 16 == 0, "%s: frame %d stream placement", name, i);
        // the next stream starts at the first multiple of 16 that is not inside this one: no overlap, and less than 16 bytes between them
        const unsigned long long end = offs[i] + lens[i], next = i + 1 < n ? offs[i + 1] : total;
        CHECK(next >= end && next - end < 16 && next % 16 == 0, "%s: stream %d ends at %llu, the next starts at %llu", name, i, end, next);
        at += (lens[i] + 15) & ~(size_t)15;
    }
    CHECK(total == at, "%s: block of %llu bytes, expected %llu", name, total, at);
    // the search finds every workgroup's frame in every grid: the last one whose first workgroup is not behind it, and the workgroup lies inside it
    for (const Probe &p : kGrids) {
        auto count = [&](int i) -> unsigned long long {
            if (p.first == &JpegEncFrame::wg_fdct) return (unsigned long long)(u_fdct_x(w[i]) * u_fdct_y(h[i]));
            if (p.first == &JpegEncFrame::wg_blk) return (unsigned long long)u_blk_wgs(w[i], h[i]);
            return (g[i].nchunks + 255ull) / 256;
        };
        auto probe = [&](unsigned long long wg, int want) {
            const int got = jpeg_enc_find(g.data(), n, (uint32_t)wg, p.first);
            CHECK(got == want, "%s: %s workgroup %llu found frame %d, expected %d", name, p.name, wg, got, want);
            if (got >= 0 && got < n) CHECK(wg >= g[got].*(p.first) && wg - g[got].*(p.first) < count(got), "%s: %s workgroup %llu is outside frame %d", name, p.name, wg, got);
        };
        for (int i = 0; i < n; i++) {
            const unsigned long long first = g[i].*(p.first), c = count(i);
            CHECK(c >= 1, "%s: frame %d has no %s workgroup", name, i, p.name);
            if (every_wg) for (unsigned long long k = 0; k < c; k++) probe(first + k, i);
            else { probe(first, i); probe(first + c - 1, i); probe(first + c / 2, i); }
        }
    }
}

int main()
{
    // the shapes of the GPU tests, forward and reversed
    const int sizes[][2] = {{1, 1}, {16, 16}, {17, 15}, {128, 16}, {129, 16}, {1040, 16}, {16, 129}, {176, 64}, {256, 256}, {64, 48}, {1024, 768}};
    {
        std::vector<int> w, h;
        for (auto &s : sizes) { w.push_back(s[0]); h.push_back(s[1]); }
        for (unsigned seed = 1; seed <= 6; seed++) {
            check_records("the edge sizes", w, h, true, seed);
            check_records("the edge sizes reversed", std::vector<int>(w.rbegin(), w.rend()), std::vector<int>(h.rbegin(), h.rend()), true, seed);
        }
        // one workgroup exactly, and one more: 128 and 129 pixels of width; 1040 is nine workgroups, the last of one MCU
        std::vector<JpegEncFrame> g;
        JpegEncTotals t;
        const std::vector<JpegEncSrc> in = frames_of(w, h);
        CHECK(jpeg_enc_build(in.data(), (int)in.size(), &g, &t), "the edge sizes refused");
        CHECK(g[3].wgs_per_row == 1 && g[4].wgs_per_row == 2 && g[5].wgs_per_row == 9 && g[5].mw == 65 && g[6].mcus == 9 && g[6].wgs_per_row == 1, "workgroups per row of the edge sizes");
        CHECK(g[7].mcus == 44 && u_blk_wgs(176, 64) == 2 && g[8].wg_blk - g[7].wg_blk == 2, "176 x 64: 264 blocks are two block workgroups");
    }
    // the search's ends: a one-workgroup frame between two large ones, n = 1, small then large and the reverse
    check_records("one workgroup between two large", {1024, 16, 1024}, {768, 16, 768}, true);
    check_records("large between 1x1", {1, 1024, 1}, {1, 768, 1}, true);
    check_records("one frame", {1024}, {768}, true);
    check_records("one frame of one pixel", {1}, {1}, true);
    check_records("no frame", {}, {}, true);
    {
        std::vector<int> sw(300, 8), sh(300, 8);
        sw.push_back(400); sh.push_back(300);
        check_records("small then large", sw, sh, true);
        check_records("large then small", std::vector<int>(sw.rbegin(), sw.rend()), std::vector<int>(sh.rbegin(), sh.rend()), true);
    }
    // 65535 frames, of one workgroup each and of random sizes
    {
        std::mt19937 rng(20261021);
        std::vector<int> w(65535, 1), h(65535, 1);
        check_records("65535 frames of one workgroup", w, h, true);
        for (int i = 0; i < 65535; i++) { w[i] = 1 + (int)(rng() % 300); h[i] = 1 + (int)(rng() % 200); }
        check_records("65535 random frames", w, h, false, 2);
        check_records("2000 random frames, every workgroup", std::vector<int>(w.begin(), w.begin() + 2000), std::vector<int>(h.begin(), h.begin() + 2000), true, 3);
    }
    // sums beyond 32 bits: 65535 frames of 65535 x 65535 are 2^16 * 2^21 transform workgroups, more than one launch takes: refused, not
    // wrapped; 1000 of them are within a launch, and their prefix sums pass 2^32
    {
        std::vector<int> w(65535, 65535), h(65535, 65535);
        std::vector<JpegEncFrame> g;
        JpegEncTotals t;
        const std::vector<JpegEncSrc> in = frames_of(w, h);
        CHECK(!jpeg_enc_build(in.data(), 65535, &g, &t), "2^37 workgroups were taken as one launch");
        CHECK(jpeg_enc_build(in.data(), 1000, &g, &t), "1000 frames of 2^32 pixels refused");
        const unsigned long long m = 4096ull * 4096, fw = 512ull * 4096, bw = (m * 6 + 255) / 256;
        CHECK(t.mcus == 1000 * m && t.fdct_wgs == 1000 * fw && t.blk_wgs == 1000 * bw, "64-bit totals: %llu MCUs, %llu and %llu workgroups", t.mcus, t.fdct_wgs, t.blk_wgs);
        CHECK(g[999].mcu_base == 999 * m && g[999].mcu_base * 6 * 4 > 0xffffffffull && g[999].wg_fdct == (uint32_t)(999 * fw) && 999 * fw < 0x7fffffffull, "64-bit offsets of the last frame");
        CHECK(jpeg_enc_find(g.data(), 1000, (uint32_t)(999 * fw - 1), &JpegEncFrame::wg_fdct) == 998 && jpeg_enc_find(g.data(), 1000, (uint32_t)(999 * fw), &JpegEncFrame::wg_fdct) == 999, "search at 2^31");
        // scans just below the limit: 1000 * 2^29 bytes of unstuffed scan, 1000 * 2^23 chunks
        std::vector<unsigned long long> bits(1000, 0xfffffffeull);
        CHECK(jpeg_enc_place_scans(bits.data(), 1000, &g, &t), "scans below the limit refused");
        CHECK(g[999].ubytes == 0x20000000u && g[999].ubase == 999ull * (0x20000000ull + 256) && g[999].ff0 == 999ull << 23 && t.chunk_wgs == 1000ull << 15, "64-bit scan offsets");
        bits[500] = 0xffffffffull;
        CHECK(!jpeg_enc_place_scans(bits.data(), 1000, &g, &t), "a scan of 2^32 - 1 bits was placed");
        // the builder's refusals
        auto one = [&](int fw_, int fh_, int stride) { const JpegEncSrc f{(const uint8_t *)0x1000, nullptr, fw_, fh_, stride}; return jpeg_enc_build(&f, 1, &g, &t); };
        CHECK(!one(0, 1, 4) && !one(1, 0, 4) && !one(65536, 1, 4 * 65536) && !one(1, 65536, 4) && !one(2, 1, 7) && one(2, 1, 8) && one(65535, 1, 4 * 65535), "the builder's refusals");
    }
    // the two rounding rules
    for (size_t v : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, (size_t)255, (size_t)256, (size_t)257, (size_t)0xfffffff1u}) {
        CHECK(align16(v) % 16 == 0 && align16(v) >= v && align16(v) - v < 16, "align16(%zu) is %zu", v, align16(v));
        CHECK(align256(v) % 256 == 0 && align256(v) >= v && align256(v) - v < 256, "align256(%zu) is %zu", v, align256(v));
    }
    // the scan-length rule of both cores: the limit is 2^32 - 1 bits, the knob can only lower it, a scan AT the limit is refused and one
    // below it passes, and the first offender is the one named
    {
        const unsigned long long top = 0xffffffffull;
        CHECK(kJpegScanBitsTop == top && jpeg_scan_limit(0) == top && jpeg_scan_limit(-1) == top && jpeg_scan_limit(-2147483647 - 1) == top, "no knob: the limit is 2^32 - 1");
        CHECK(jpeg_scan_limit(1) == 1 && jpeg_scan_limit(4000) == 4000 && jpeg_scan_limit(2147483647) == 2147483647ull, "the knob lowers the limit");
        for (int knob : {-5, 0, 1, 2, 4000, 65536, 2147483647}) CHECK(jpeg_scan_limit(knob) <= top && jpeg_scan_limit(knob) >= 1, "knob %d: limit %llu", knob, jpeg_scan_limit(knob));
        for (unsigned long long limit : {1ull, 4000ull, 2147483647ull, top}) {
            const unsigned long long below[] = {0, limit - 1, limit / 2}, at[] = {limit - 1, limit, 0}, over[] = {limit - 1, 0, limit + 1, limit};
            CHECK(jpeg_scan_too_long(below, 3, limit) == -1, "limit %llu: a scan below it was refused", limit);
            CHECK(jpeg_scan_too_long(at, 3, limit) == 1, "limit %llu: a scan at it passed, or another was named", limit);
            CHECK(jpeg_scan_too_long(over, 4, limit) == 2, "limit %llu: the first offender is frame 2", limit);
            CHECK(jpeg_scan_too_long(over, 2, limit) == -1 && jpeg_scan_too_long(over, 0, limit) == -1, "limit %llu: scans beyond n were read", limit);
        }
        // what passes the rule at its top is what jpeg_enc_place_scans takes
        std::vector<JpegEncFrame> g(1);
        JpegEncTotals t;
        const unsigned long long last_ok = top - 1;
        CHECK(jpeg_scan_too_long(&last_ok, 1, jpeg_scan_limit(0)) == -1 && jpeg_enc_place_scans(&last_ok, 1, &g, &t), "2^32 - 2 bits pass both");
        CHECK(jpeg_scan_too_long(&top, 1, jpeg_scan_limit(0)) == 0 && !jpeg_enc_place_scans(&top, 1, &g, &t), "2^32 - 1 bits pass neither");
    }
    // the SOF0 dimensions lie where jpeg_write_header puts them: SOI, DQT with two tables, the SOF0 marker, length and precision
    CHECK(kJpegSofDims == 141, "SOF0 dimensions at %d", kJpegSofDims);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("jpeg enc mixed plan ok\n");
    return 0;
}
