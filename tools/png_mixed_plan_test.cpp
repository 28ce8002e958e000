// png_mixed_plan_test.cpp -- the mixed-size PNG leg's ordering and cutting (imageprocessor_amd/csrc/ipx_mixed_cut.h: files ->
// decode groups -> chunks -> runs) and the two layouts of decoded frames and palettes (ipx_png_layout.h: strided, packed), compared
// with the four loops they replaced, held to their rules as a program of its own: plain g++, no GPU, no runtime.
//   g++ -std=c++17 -fsanitize=address,undefined -o png_mixed_plan_test tools/png_mixed_plan_test.cpp && ./png_mixed_plan_test
// Prints "png mixed plan ok" and exits 0, or says what broke and exits 1.  tests/test_png_mixed_host.py runs it.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../imageprocessor_amd/csrc/ipx_png_layout.h"
#include "../imageprocessor_amd/csrc/ipx_mixed_cut.h"

using namespace ipx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// every rule of the cut, for any input
static void check_cut(const char *name, const std::vector<MixItem> &items, int group_files, size_t group_bytes, size_t chunk_bytes)
{
    const int n = (int)items.size();
    const MixCut c = mixed_cut(items.data(), n, group_files, group_bytes, chunk_bytes);
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

// ---- where decoded frames and palettes go (ipx_png_layout.h) ------------------------------------------------------------------------
static size_t a256(size_t v) { return (v + 255) & ~(size_t)255; }

// the rules every layout keeps; packed: also that the frames lie back to back from 0 and the slots are dense over the paletted files
static void check_layout(const char *name, const PngFrameLayout &at, const std::vector<int> &idx, const std::vector<size_t> &frame_bytes, bool packed,
                         const std::vector<bool> *paletted)
{
    const size_t m = idx.size();
    CHECK(at.idx == idx && at.pal_slot.size() == m && at.off.size() == m, "%s: the vectors do not cover the selection", name);
    if (at.pal_slot.size() != m || at.off.size() != m) return;
    int next_slot = 0;
    for (size_t g = 0; g < m; g++) {
        CHECK(at.off[g] % 256 == 0, "%s: offset %zu of position %zu is not aligned", name, at.off[g], g);
        const size_t end = at.off[g] + frame_bytes[g];
        CHECK(end <= (g + 1 < m ? at.off[g + 1] : at.bytes), "%s: frame %zu runs into the next", name, g);
        if (packed) {
            CHECK(at.off[g] == (g ? at.off[g - 1] + a256(frame_bytes[g - 1]) : 0), "%s: frame %zu is not packed", name, g);
            CHECK(at.pal_slot[g] == ((*paletted)[g] ? next_slot : -1), "%s: slot %d at position %zu", name, at.pal_slot[g], g);
            if ((*paletted)[g]) next_slot++;
        }
    }
    if (m) CHECK(at.bytes == at.off[m - 1] + a256(frame_bytes[m - 1]), "%s: the last frame does not end at bytes", name);
    else CHECK(at.bytes == 0 && at.pal_slots == 0, "%s: an empty selection takes room", name);
    if (packed) CHECK(at.pal_slots == next_slot, "%s: %d palette slots for %d paletted files", name, at.pal_slots, next_slot);
}

static void check_strided(const char *name, const std::vector<int> &idx, size_t fs, bool by_index)
{
    const PngFrameLayout at = png_layout_strided(idx, fs, by_index);
    check_layout(name, at, idx, std::vector<size_t>(idx.size(), fs), false, nullptr);
    for (size_t g = 0; g < idx.size() && g < at.off.size(); g++) {
        const int k = by_index ? idx[g] : (int)g;
        CHECK(at.off[g] == (size_t)k * fs && at.pal_slot[g] == k, "%s: position %zu at offset %zu, slot %d", name, g, at.off[g], at.pal_slot[g]);
    }
    if (!idx.empty()) CHECK(at.pal_slots == (by_index ? idx.back() : (int)idx.size() - 1) + 1, "%s: %d palette slots", name, at.pal_slots);
}

// The four loops the builders replaced, as their callers had them.  What each handed to the decode driver: idx, slot, frame_off; the
// driver uploaded max(slot) + 1 palette slots; the packed callers allocated fbytes and npal slots, run_png_png fs * m and m.
struct OldLayout { std::vector<int> idx, slot; std::vector<size_t> foff; };
static int old_nslot(const OldLayout &o) { return o.idx.empty() ? 0 : *std::max_element(o.slot.begin(), o.slot.end()) + 1; }
static OldLayout old_decode_batch(const std::vector<int> &status, size_t fs)
{
    std::vector<int> idx;
    for (int i = 0; i < (int)status.size(); i++)
        if (status[i] == 0) idx.push_back(i);
    std::vector<size_t> foff(idx.size());
    for (size_t g = 0; g < idx.size(); g++) foff[g] = (size_t)idx[g] * fs;
    return OldLayout{idx, idx, foff};
}
static OldLayout old_run_png_png(const std::vector<int> &of_kind, size_t g0, int m, size_t fs)
{
    std::vector<int> idx(of_kind.begin() + g0, of_kind.begin() + g0 + m), slot(m);
    std::vector<size_t> foff(m);
    for (int g = 0; g < m; g++) { slot[g] = g; foff[g] = (size_t)g * fs; }
    return OldLayout{idx, slot, foff};
}
struct OldFile { int status, w, h, bpp; bool paletted; };
static OldLayout old_decode_mixed(const std::vector<OldFile> &info, size_t *fbytes_out, int *npal_out)
{
    std::vector<int> idx, slot;
    std::vector<size_t> foff;
    size_t fbytes = 0;
    int npal = 0;
    for (int i = 0; i < (int)info.size(); i++) {
        if (info[i].status != 0) continue;
        idx.push_back(i);
        foff.push_back(fbytes);
        slot.push_back(info[i].paletted ? npal++ : -1);
        fbytes += a256((size_t)info[i].w * info[i].h * info[i].bpp);
    }
    *fbytes_out = fbytes;
    *npal_out = npal;
    return OldLayout{idx, slot, foff};
}
static OldLayout old_run_mixed(const std::vector<OldFile> &info, const std::vector<int> &order, int first, int m, size_t *fbytes_out, int *npal_out)
{
    std::vector<int> idx(order.begin() + first, order.begin() + first + m), slot(m);
    std::vector<size_t> foff(m);
    size_t fbytes = 0;
    int npal = 0;
    for (int g = 0; g < m; g++) {
        const OldFile &f = info[idx[g]];
        foff[g] = fbytes;
        slot[g] = f.paletted ? npal++ : -1;
        fbytes += a256((size_t)f.w * f.h * f.bpp);
    }
    *fbytes_out = fbytes;
    *npal_out = npal;
    return OldLayout{idx, slot, foff};
}
static void same_layout(const char *name, const PngFrameLayout &at, const OldLayout &o)
{
    CHECK(at.idx == o.idx && at.pal_slot == o.slot && at.off == o.foff, "%s: not what the old loop made", name);
    CHECK(at.pal_slots == old_nslot(o), "%s: %d palette slots, the old loop's upload covered %d", name, at.pal_slots, old_nslot(o));
}

static void layout_cases()
{
    // the empty selection, one file, a zero-byte frame size
    for (int by_index = 0; by_index < 2; by_index++) {
        check_strided("strided, empty", {}, 512, by_index);
        check_strided("strided, one file", {3}, 256, by_index);
        check_strided("strided, zero-byte frames", {0, 2, 5}, 0, by_index);
        check_strided("strided, gaps", {1, 2, 7, 9}, 1024, by_index);
    }
    {
        const PngFrameLayout at = png_layout_strided({1, 2, 7, 9}, 1024, true);
        CHECK(at.off[2] == 7 * 1024 && at.pal_slot[3] == 9 && at.pal_slots == 10 && at.bytes == 10 * 1024, "strided by index: a known case");
        const PngFrameLayout bt = png_layout_strided({1, 2, 7, 9}, 1024, false);
        CHECK(bt.off[2] == 2 * 1024 && bt.pal_slot[3] == 3 && bt.pal_slots == 4 && bt.bytes == 4 * 1024, "strided by position: a known case");
    }
    {
        // files 4, 0, 6, 2 of 24, 0, 300 and 256 bytes; 4 and 6 paletted
        const std::vector<int> idx = {4, 0, 6, 2};
        const size_t bytes_of[7] = {0, 0, 256, 0, 24, 0, 300};
        const bool pal_of[7] = {false, false, false, false, true, false, true};
        const PngFrameLayout at = png_layout_packed(idx, [&](int i) { return PngFrameNeed{bytes_of[i], pal_of[i]}; });
        const std::vector<bool> pal = {true, false, true, false};
        check_layout("packed, known", at, idx, {24, 0, 300, 256}, true, &pal);
        CHECK(at.off == (std::vector<size_t>{0, 256, 256, 768}) && at.bytes == 1024, "packed: a known case");
        CHECK(at.pal_slot == (std::vector<int>{0, -1, 1, -1}) && at.pal_slots == 2, "packed: the known case's slots");
        const PngFrameLayout e = png_layout_packed({}, [&](int) { return PngFrameNeed{1, true}; });
        check_layout("packed, empty", e, {}, {}, true, nullptr);
        const PngFrameLayout one = png_layout_packed({5}, [&](int) { return PngFrameNeed{1, false}; });
        CHECK(one.off == std::vector<size_t>{0} && one.bytes == 256 && one.pal_slot == std::vector<int>{-1} && one.pal_slots == 0, "packed: one file");
    }
    // seeded random batches against the old loops
    std::mt19937 rng(20241021);
    for (int round = 0; round < 400; round++) {
        const int n = (int)(rng() % 40);
        std::vector<OldFile> info(n);
        std::vector<int> status(n);
        for (int i = 0; i < n; i++) {
            const int bpps[4] = {1, 2, 4, 8};
            info[i] = OldFile{rng() % 4 == 0 ? -1 : 0, 1 + (int)(rng() % 40), 1 + (int)(rng() % 30), bpps[rng() % 4], rng() % 3 == 0};
            if (info[i].paletted) info[i].bpp = 1;
            status[i] = info[i].status;
        }
        auto need = [&](int i) { return PngFrameNeed{(size_t)info[i].w * info[i].h * info[i].bpp, info[i].paletted}; };
        const size_t fs = 256 * (size_t)(rng() % 20);
        // ipx_png_decode_batch
        const OldLayout ob = old_decode_batch(status, fs);
        same_layout("decode batch", png_layout_strided(ob.idx, fs, true), ob);
        check_strided("decode batch", ob.idx, fs, true);
        // run_png_png: a group of the OK files
        if (!ob.idx.empty()) {
            const size_t g0 = rng() % ob.idx.size();
            const int m = 1 + (int)(rng() % (ob.idx.size() - g0));
            const OldLayout og = old_run_png_png(ob.idx, g0, m, fs);
            const PngFrameLayout at = png_layout_strided(og.idx, fs, false);
            same_layout("run_png_png", at, og);
            CHECK(at.bytes == fs * m && at.pal_slots == m, "run_png_png: %zu bytes and %d slots for %d files", at.bytes, at.pal_slots, m);
            check_strided("run_png_png", og.idx, fs, false);
        }
        // ipx_png_decode_mixed
        size_t fbytes;
        int npal;
        const OldLayout om = old_decode_mixed(info, &fbytes, &npal);
        const PngFrameLayout am = png_layout_packed(om.idx, need);
        same_layout("decode mixed", am, om);
        CHECK(am.bytes == fbytes && am.pal_slots == npal, "decode mixed: %zu bytes, %d slots", am.bytes, am.pal_slots);
        std::vector<size_t> fb;
        std::vector<bool> pal;
        for (int i : om.idx) { fb.push_back(need(i).bytes); pal.push_back(info[i].paletted); }
        check_layout("decode mixed", am, om.idx, fb, true, &pal);
        // ipx_run_png_png_mixed: a group of a shuffled order of the OK files
        std::vector<int> order = om.idx;
        std::shuffle(order.begin(), order.end(), rng);
        if (!order.empty()) {
            const int first = (int)(rng() % order.size()), m = 1 + (int)(rng() % (order.size() - first));
            const OldLayout ox = old_run_mixed(info, order, first, m, &fbytes, &npal);
            const PngFrameLayout ax = png_layout_packed(ox.idx, need);
            same_layout("run mixed", ax, ox);
            CHECK(ax.bytes == fbytes && ax.pal_slots == npal, "run mixed: %zu bytes, %d slots", ax.bytes, ax.pal_slots);
        }
    }
}

int main()
{
    layout_cases();
    // n = 0, and nothing but failed files
    {
        const MixCut c = mixed_cut(nullptr, 0, 1024, 1u << 30, 1u << 30);
        CHECK(c.order.empty() && c.groups.empty() && c.chunks.empty() && c.runs.empty(), "n = 0 makes something");
        std::vector<MixItem> bad(5, MixItem{false, 4, 4, 0, 100, 100});
        const MixCut d = mixed_cut(bad.data(), 5, 1024, 1u << 30, 1u << 30);
        CHECK(d.order.empty() && d.groups.empty() && d.chunks.empty() && d.runs.empty(), "failed files make something");
        check_cut("all failed", bad, 1024, 1u << 30, 1u << 30);
    }
    // a known case: sizes interleaved, one failed file, everything within the budgets -> one group, one chunk, a run per size and kind
    {
        std::vector<MixItem> it;
        const int sizes[4][2] = {{64, 48}, {48, 64}, {200, 150}, {5, 1}};
        for (int i = 0; i < 24; i++) it.push_back(MixItem{true, sizes[i % 4][0], sizes[i % 4][1], (i / 4) % 3, 1000, 5000});
        it[7].ok = false;
        const MixCut c = mixed_cut(it.data(), (int)it.size(), 1024, 1u << 30, 1u << 30);
        CHECK(c.order.size() == 23 && c.groups.size() == 1 && c.chunks.size() == 1 && c.runs.size() == 12, "known case: %zu files, %zu groups, %zu chunks, %zu runs",
              c.order.size(), c.groups.size(), c.chunks.size(), c.runs.size());
        CHECK(it[c.order[0]].w == 5 && it[c.order.back()].w == 200, "known case: the order does not start at the narrowest size");
        check_cut("known", it, 1024, 1u << 30, 1u << 30);
        // the same with budgets that split inside a size run: two files per chunk, five per group
        check_cut("known, split", it, 5, 1u << 30, 10000);
        const MixCut s = mixed_cut(it.data(), (int)it.size(), 5, 1u << 30, 10000);
        CHECK(s.groups.size() == 5 && s.chunks.size() == 14, "known case, split: %zu groups, %zu chunks", s.groups.size(), s.chunks.size());
    }
    // a single file larger than both budgets still gets a group and a chunk of its own
    {
        std::vector<MixItem> it = {MixItem{true, 10, 10, 2, 100, 100}, MixItem{true, 9000, 9000, 2, (size_t)5 << 30, (size_t)9 << 30},
                                   MixItem{true, 10, 10, 2, 100, 100}};
        const MixCut c = mixed_cut(it.data(), 3, 1024, (size_t)4 << 30, (size_t)1 << 30);
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
