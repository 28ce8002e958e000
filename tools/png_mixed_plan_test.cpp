// png_mixed_plan_test.cpp -- the mixed-size PNG leg's ordering and cutting (imageprocessor_amd/csrc/ipx_png_mixed_plan.h: files ->
// decode groups -> chunks -> runs) held to its rules as a program of its own: plain g++, no GPU, no runtime.
//   g++ -std=c++17 -fsanitize=address,undefined -o png_mixed_plan_test tools/png_mixed_plan_test.cpp && ./png_mixed_plan_test
// Prints "png mixed plan ok" and exits 0, or says what broke and exits 1.  tests/test_png_mixed_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_png_mixed_plan.h"

using namespace ipx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// every rule of the cut, for any input
static void check_cut(const char *name, const std::vector<MixItem> &items, int group_files, size_t group_bytes, size_t chunk_bytes)
{
    const int n = (int)items.size();
    const MixCut c = png_mixed_cut(items.data(), n, group_files, group_bytes, chunk_bytes);
    const int gf = group_files < 1 ? 1 : group_files;
    // the order: every OK file once, no other, sorted by (w, h, kind) with ties by index
    std::vector<int> seen(n, 0);
    for (int i : c.order) { CHECK(i >= 0 && i < n && items[i].ok, "%s: order names file %d", name, i); if (i >= 0 && i < n) seen[i]++; }
    for (int i = 0; i < n; i++) CHECK(seen[i] == (items[i].ok ? 1 : 0), "%s: file %d is in the order %d times", name, i, seen[i]);
    for (size_t p = 1; p < c.order.size(); p++) {
        const MixItem &a = items[c.order[p - 1]], &b = items[c.order[p]];
        const bool le = std::make_tuple(a.w, a.h, a.kind, c.order[p - 1]) < std::make_tuple(b.w, b.h, b.kind, c.order[p]);
        CHECK(le, "%s: order not sorted at %zu", name, p);
    }
    // groups tile the order; chunks tile their group; runs tile their chunk
    int at = 0, chunk_at = 0, run_at = 0;
    std::vector<int> in_run(n, 0);
    for (const MixGroup &g : c.groups) {
        CHECK(g.first == at && g.n >= 1, "%s: group at %d starts at %d with %d files", name, at, g.first, g.n);
        CHECK(g.n <= gf, "%s: group of %d files, the limit is %d", name, g.n, gf);
        size_t fb = 0;
        for (int p = g.first; p < g.first + g.n; p++) fb += items[c.order[p]].frame_bytes;
        CHECK(g.n == 1 || fb <= group_bytes, "%s: group of %zu frame bytes, the budget is %zu", name, fb, group_bytes);
        // (a group ends only for a reason: the next file would break a limit)
        if (g.first + g.n < (int)c.order.size())
            CHECK(g.n == gf || fb + items[c.order[g.first + g.n]].frame_bytes > group_bytes, "%s: group at %d ended early", name, g.first);
        CHECK(g.chunk0 == chunk_at && g.nchunks >= 1, "%s: group's chunks start at %d, expected %d", name, g.chunk0, chunk_at);
        int cat = g.first;
        for (int k = g.chunk0; k < g.chunk0 + g.nchunks; k++) {
            const MixChunk &ch = c.chunks[k];
            CHECK(ch.first == cat && ch.n >= 1, "%s: chunk %d starts at %d, expected %d", name, k, ch.first, cat);
            size_t cb = 0;
            for (int p = ch.first; p < ch.first + ch.n; p++) cb += items[c.order[p]].chunk_bytes;
            CHECK(ch.n == 1 || cb <= chunk_bytes, "%s: chunk of %zu bytes, the budget is %zu", name, cb, chunk_bytes);
            if (ch.first + ch.n < g.first + g.n)
                CHECK(cb + items[c.order[ch.first + ch.n]].chunk_bytes > chunk_bytes, "%s: chunk %d ended early", name, k);
            CHECK(ch.run0 == run_at && ch.nruns >= 1, "%s: chunk's runs start at %d, expected %d", name, ch.run0, run_at);
            int rat = ch.first;
            for (int r = ch.run0; r < ch.run0 + ch.nruns; r++) {
                const MixRun &run = c.runs[r];
                CHECK(run.first == rat && run.n >= 1, "%s: run %d starts at %d, expected %d", name, r, run.first, rat);
                const MixItem &a = items[c.order[run.first]];
                for (int p = run.first; p < run.first + run.n; p++) {
                    const MixItem &b = items[c.order[p]];
                    CHECK(a.w == b.w && a.h == b.h && a.kind == b.kind, "%s: run %d mixes sizes or kinds", name, r);
                    in_run[c.order[p]]++;
                }
                // (a run ends only at another size or kind, or at its chunk's end)
                if (run.first + run.n < ch.first + ch.n) {
                    const MixItem &b = items[c.order[run.first + run.n]];
                    CHECK(!(a.w == b.w && a.h == b.h && a.kind == b.kind), "%s: run %d ended inside a size", name, r);
                }
                rat += run.n;
            }
            CHECK(rat == ch.first + ch.n, "%s: chunk %d's runs cover %d of %d files", name, k, rat - ch.first, ch.n);
            run_at += ch.nruns;
            cat += ch.n;
        }
        CHECK(cat == g.first + g.n, "%s: group's chunks cover %d of %d files", name, cat - g.first, g.n);
        chunk_at += g.nchunks;
        at += g.n;
    }
    CHECK(at == (int)c.order.size(), "%s: the groups cover %d of %zu files", name, at, c.order.size());
    CHECK(chunk_at == (int)c.chunks.size() && run_at == (int)c.runs.size(), "%s: stray chunks or runs", name);
    for (int i = 0; i < n; i++) CHECK(in_run[i] == (items[i].ok ? 1 : 0), "%s: file %d is in %d runs", name, i, in_run[i]);
}

int main()
{
    // n = 0, and nothing but failed files
    {
        const MixCut c = png_mixed_cut(nullptr, 0, 1024, 1u << 30, 1u << 30);
        CHECK(c.order.empty() && c.groups.empty() && c.chunks.empty() && c.runs.empty(), "n = 0 makes something");
        std::vector<MixItem> bad(5, MixItem{false, 4, 4, 0, 100, 100});
        const MixCut d = png_mixed_cut(bad.data(), 5, 1024, 1u << 30, 1u << 30);
        CHECK(d.order.empty() && d.groups.empty() && d.chunks.empty() && d.runs.empty(), "failed files make something");
        check_cut("all failed", bad, 1024, 1u << 30, 1u << 30);
    }
    // a known case: sizes interleaved, one failed file, everything within the budgets -> one group, one chunk, a run per size and kind
    {
        std::vector<MixItem> it;
        const int sizes[4][2] = {{64, 48}, {48, 64}, {200, 150}, {5, 1}};
        for (int i = 0; i < 24; i++) it.push_back(MixItem{true, sizes[i % 4][0], sizes[i % 4][1], (i / 4) % 3, 1000, 5000});
        it[7].ok = false;
        const MixCut c = png_mixed_cut(it.data(), (int)it.size(), 1024, 1u << 30, 1u << 30);
        CHECK(c.order.size() == 23 && c.groups.size() == 1 && c.chunks.size() == 1 && c.runs.size() == 12, "known case: %zu files, %zu groups, %zu chunks, %zu runs",
              c.order.size(), c.groups.size(), c.chunks.size(), c.runs.size());
        CHECK(it[c.order[0]].w == 5 && it[c.order.back()].w == 200, "known case: the order does not start at the narrowest size");
        check_cut("known", it, 1024, 1u << 30, 1u << 30);
        // the same with budgets that split inside a size run: two files per chunk, five per group
        check_cut("known, split", it, 5, 1u << 30, 10000);
        const MixCut s = png_mixed_cut(it.data(), (int)it.size(), 5, 1u << 30, 10000);
        CHECK(s.groups.size() == 5 && s.chunks.size() == 14, "known case, split: %zu groups, %zu chunks", s.groups.size(), s.chunks.size());
    }
    // a single file larger than both budgets still gets a group and a chunk of its own
    {
        std::vector<MixItem> it = {MixItem{true, 10, 10, 2, 100, 100}, MixItem{true, 9000, 9000, 2, (size_t)5 << 30, (size_t)9 << 30},
                                   MixItem{true, 10, 10, 2, 100, 100}};
        const MixCut c = png_mixed_cut(it.data(), 3, 1024, (size_t)4 << 30, (size_t)1 << 30);
        CHECK(c.groups.size() == 2 && c.chunks.size() == 2 && c.runs.size() == 2, "big file: %zu groups, %zu chunks, %zu runs", c.groups.size(),
              c.chunks.size(), c.runs.size());
        CHECK(c.groups[1].n == 1 && c.order[c.groups[1].first] == 1 && c.chunks[1].n == 1, "big file: not alone");
        check_cut("big file", it, 1024, (size_t)4 << 30, (size_t)1 << 30);
        check_cut("zero budgets", it, 0, 0, 0);
    }
    // random batches under random budgets
    std::mt19937 rng(20240607);
    for (int round = 0; round < 300; round++) {
        const int n = (int)(rng() % 70);
        std::vector<MixItem> it(n);
        for (MixItem &m : it) {
            m.ok = rng() % 8 != 0;
            m.w = 1 + (int)(rng() % 4);
            m.h = 1 + (int)(rng() % 3);
            m.kind = (int)(rng() % 7);
            m.frame_bytes = 256 * (1 + rng() % 40);
            m.chunk_bytes = 256 * (1 + rng() % 200);
        }
        check_cut("random", it, (int)(rng() % 12), 256 * (size_t)(rng() % 200), 256 * (size_t)(rng() % 600));
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("png mixed plan ok\n");
    return 0;
}
