// jpeg_mixed_plan_test.cpp -- the host side of a mixed-size JPEG decode's per-image records (imageprocessor_amd/csrc/
// ipx_jpeg_mixed_plan.h: jpeg_mix_build, jpeg_mix_find) and the cut the mixed-size JPEG leg makes with the sampling class as the kind
// (ipx_mixed_cut.h), held to their rules as a program of its own: plain g++, no GPU, no runtime.
//   g++ -std=c++17 -fsanitize=address,undefined -o jpeg_mixed_plan_test tools/jpeg_mixed_plan_test.cpp && ./jpeg_mixed_plan_test
// Prints "jpeg mixed plan ok" and exits 0, or says what broke and exits 1.  tests/test_jpeg_mixed_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_jpeg_mixed_plan.h"
#include "../imageprocessor_amd/csrc/ipx_mixed_cut.h"

using namespace ipx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 50) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const JpegMixClass kClasses[] = {{1, 1, 0}, {2, 1, 0}, {2, 2, 0}, {1, 2, 0}, {1, 1, 1}};   // 4:4:4, 4:2:2, 4:2:0, 4:4:0, Gray

// every rule of the records, for any sizes; every_wg: walk every workgroup of the launch through the search (else the ends of each image)
static void check_records(const char *name, const JpegMixClass &c, const std::vector<int> &w, const std::vector<int> &h, bool every_wg)
{
    const int n = (int)w.size();
    std::vector<JpegMixGeom> g;
    JpegMixTotals t;
    const bool ok = jpeg_mix_build(c, w.data(), h.data(), n, &g, &t);
    CHECK(ok, "%s: refused", name);
    if (!ok) return;
    CHECK((int)g.size() == n, "%s: %zu records for %d images", name, g.size(), n);
    unsigned long long blocks = 0, wgs = 0, yb = 0, cb = 0;
    int max_nblk = 0;
    for (int i = 0; i < n; i++) {
        const JpegMixGeom &r = g[i];
        const int mxx = (w[i] + 8 * c.h0 - 1) / (8 * c.h0), myy = (h[i] + 8 * c.v0 - 1) / (8 * c.v0);
        CHECK(r.w == w[i] && r.h == h[i] && r.mxx == mxx && r.myy == myy, "%s: image %d geometry", name, i);
        CHECK(r.nblk == mxx * myy * c.bpm(), "%s: image %d has %d blocks", name, i, r.nblk);
        CHECK(r.ystride == 8 * c.h0 * mxx && r.cstride == 8 * mxx, "%s: image %d strides", name, i);
        CHECK(r.wgs_per_row == (mxx + c.mcus_per_wg() - 1) / c.mcus_per_wg() && r.wgs_per_row >= 1, "%s: image %d workgroups per row", name, i);
        // the prefix sums: monotone, each image starts where the one before ended
        CHECK(r.blk0 == blocks, "%s: image %d starts at block %llu, expected %llu", name, i, r.blk0, blocks);
        CHECK((unsigned long long)r.wg0 == wgs, "%s: image %d starts at workgroup %u, expected %llu", name, i, r.wg0, wgs);
        CHECK(r.yoff == yb && r.coff == cb, "%s: image %d plane offsets", name, i);
        CHECK(r.yoff % 256 == 0 && r.coff % 256 == 0, "%s: image %d planes are not 256-byte aligned", name, i);
        blocks += (unsigned long long)r.nblk;
        wgs += (unsigned long long)r.wgs_per_row * myy;
        const unsigned long long ysz = (unsigned long long)r.ystride * 8 * c.v0 * myy, csz = (unsigned long long)r.cstride * 8 * myy;
        yb += (ysz + 255) & ~255ull;
        cb += c.gray ? 0 : (csz + 255) & ~255ull;
        if (r.nblk > max_nblk) max_nblk = r.nblk;
    }
    // the last image's end equals the total
    CHECK(t.blocks == blocks && t.wgs == wgs && t.ybytes == yb && t.cbytes == cb && t.max_nblk == max_nblk, "%s: totals", name);
    CHECK(t.wgs <= 0x7fffffffull, "%s: %llu workgroups", name, t.wgs);
    // the search finds every workgroup's image: the last one whose first workgroup is not behind it, and the workgroup lies inside it
    auto probe = [&](unsigned long long wg, int want) {
        const int got = jpeg_mix_find(g.data(), n, (uint32_t)wg);
        CHECK(got == want, "%s: workgroup %llu found image %d, expected %d", name, wg, got, want);
        if (got >= 0 && got < n) {
            const unsigned long long in = wg - g[got].wg0;
            CHECK(wg >= g[got].wg0 && in < (unsigned long long)g[got].wgs_per_row * g[got].myy, "%s: workgroup %llu is outside image %d", name, wg, got);
        }
    };
    for (int i = 0; i < n; i++) {
        const unsigned long long first = g[i].wg0, count = (unsigned long long)g[i].wgs_per_row * g[i].myy;
        if (every_wg) for (unsigned long long k = 0; k < count; k++) probe(first + k, i);
        else { probe(first, i); probe(first + count - 1, i); probe(first + count / 2, i); }
    }
}

int main()
{
    // the shapes of the GPU tests: ten sizes in every class, in file order and reversed
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 7}, {16, 16}, {17, 17}, {33, 15}, {64, 48}, {129, 65}, {257, 40}, {200, 120}};
    for (const JpegMixClass &c : kClasses) {
        std::vector<int> w, h;
        for (auto &s : sizes) { w.push_back(s[0]); h.push_back(s[1]); }
        check_records("ten sizes", c, w, h, true);
        check_records("ten sizes reversed", c, std::vector<int>(w.rbegin(), w.rend()), std::vector<int>(h.rbegin(), h.rend()), true);
        // the search's ends: thirty one-workgroup images before one of hundreds, the same reversed, a large one between two of 1 x 1, one image
        std::vector<int> sw(30, 8), sh(30, 8);
        sw.push_back(400); sh.push_back(300);
        check_records("small then large", c, sw, sh, true);
        check_records("large then small", c, std::vector<int>(sw.rbegin(), sw.rend()), std::vector<int>(sh.rbegin(), sh.rend()), true);
        check_records("large between 1x1", c, {1, 400, 1}, {1, 300, 1}, true);
        check_records("one image", c, {400}, {300}, true);
        check_records("one image of one pixel", c, {1}, {1}, true);
        check_records("no image", c, {}, {}, true);
    }
    // 257 x 40 at 4:2:0: 17 MCUs per row are two full workgroups and a tail of one MCU, three MCU rows
    {
        std::vector<JpegMixGeom> g;
        JpegMixTotals t;
        const int w = 257, h = 40;
        CHECK(jpeg_mix_build(kClasses[2], &w, &h, 1, &g, &t) && g[0].mxx == 17 && g[0].myy == 3 && g[0].wgs_per_row == 3 && t.wgs == 9 && t.blocks == 17 * 3 * 6,
              "257 x 40 at 4:2:0");
    }
    // 65535 images, of one workgroup each and of random sizes
    {
        std::mt19937 rng(20261021);
        std::vector<int> w(65535, 1), h(65535, 1);
        check_records("65535 images of one workgroup", kClasses[2], w, h, true);
        for (int i = 0; i < 65535; i++) { w[i] = 1 + (int)(rng() % 300); h[i] = 1 + (int)(rng() % 200); }
        for (const JpegMixClass &c : kClasses) check_records("65535 random images", c, w, h, false);
        for (int i = 0; i < 2000; i++) { w[i] = 1 + (int)(rng() % 300); h[i] = 1 + (int)(rng() % 200); }
        check_records("2000 random images, every workgroup", kClasses[0], std::vector<int>(w.begin(), w.begin() + 2000), std::vector<int>(h.begin(), h.begin() + 2000), true);
    }
    // sums beyond 32 bits: 65535 images of 16384 x 16384 (2^28 pixels, the parser's limit) at 4:4:4 are 2^44 bytes of luma and 2^34
    // blocks -- the offsets hold them -- and 2^35 workgroups, more than one launch takes: refused, not wrapped
    {
        std::vector<int> w(65535, 16384), h(65535, 16384);
        std::vector<JpegMixGeom> g;
        JpegMixTotals t;
        CHECK(!jpeg_mix_build(kClasses[0], w.data(), h.data(), 65535, &g, &t), "2^35 workgroups were taken as one launch");
        // 3000 of them are within a launch: 3000 * 2^19 workgroups, 3000 * 2^28 luma bytes, 3000 * 3 * 2^22 blocks
        CHECK(jpeg_mix_build(kClasses[0], w.data(), h.data(), 3000, &g, &t), "3000 images of 2^28 pixels refused");
        CHECK(t.wgs == 3000ull << 19 && t.ybytes == 3000ull << 28 && t.blocks == (3000ull * 3) << 22, "64-bit totals: %llu workgroups, %llu bytes, %llu blocks", t.wgs, t.ybytes, t.blocks);
        CHECK(g[2999].blk0 == (2999ull * 3) << 22 && g[2999].yoff == 2999ull << 28 && g[2999].wg0 == (uint32_t)(2999ull << 19), "64-bit offsets of the last image");
        CHECK(g[2999].yoff > 0xffffffffull && g[2999].blk0 * 128 > 0xffffffffull, "the offsets did not pass 2^32");
        CHECK(jpeg_mix_find(g.data(), 3000, (uint32_t)((2999ull << 19) - 1)) == 2998 && jpeg_mix_find(g.data(), 3000, (uint32_t)(2999ull << 19)) == 2999, "search at 2^30");
        const int zero = 0, one = 1;
        CHECK(!jpeg_mix_build(kClasses[0], &zero, &one, 1, &g, &t) && !jpeg_mix_build(kClasses[0], &one, &zero, 1, &g, &t), "an empty image was taken");
    }
    // the leg's cut with the class as the kind: runs are one size and one class, every OK file is in exactly one run
    {
        std::mt19937 rng(7);
        for (int round = 0; round < 200; round++) {
            const int n = 1 + (int)(rng() % 60);
            std::vector<MixItem> items(n);
            for (MixItem &it : items) {
                const int s = (int)(rng() % 4), k = (int)(rng() % 5);
                it = MixItem{rng() % 7 != 0, sizes[s][0], sizes[s][1], kClasses[k].gray ? 0 : kClasses[k].h0 * 4 + kClasses[k].v0, 1000 + rng() % 5000, 500 + rng() % 3000};
            }
            const MixCut c = mixed_cut(items.data(), n, 1 + (int)(rng() % 8), 2000 + rng() % 20000, rng() % 10000);
            std::vector<int> in_run(n, 0);
            size_t at = 0;
            for (const MixGroup &grp : c.groups)
                for (int ci = grp.chunk0; ci < grp.chunk0 + grp.nchunks; ci++)
                    for (int r = c.chunks[ci].run0; r < c.chunks[ci].run0 + c.chunks[ci].nruns; r++) {
                        const MixRun &run = c.runs[r];
                        CHECK((size_t)run.first == at && run.n >= 1, "cut %d: run %d starts at %d, expected %zu", round, r, run.first, at);
                        CHECK(run.first >= c.chunks[ci].first && run.first + run.n <= c.chunks[ci].first + c.chunks[ci].n, "cut %d: run %d leaves its chunk", round, r);
                        CHECK(c.chunks[ci].first >= grp.first && c.chunks[ci].first + c.chunks[ci].n <= grp.first + grp.n, "cut %d: chunk %d leaves its group", round, ci);
                        for (int p = run.first; p < run.first + run.n; p++) {
                            const MixItem &a = items[c.order[run.first]], &b = items[c.order[p]];
                            CHECK(b.ok && a.w == b.w && a.h == b.h && a.kind == b.kind, "cut %d: run %d mixes sizes or classes", round, r);
                            in_run[c.order[p]]++;
                        }
                        at += (size_t)run.n;
                    }
            for (int i = 0; i < n; i++) CHECK(in_run[i] == (items[i].ok ? 1 : 0), "cut %d: file %d is in %d runs", round, i, in_run[i]);
        }
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("jpeg mixed plan ok\n");
    return 0;
}
