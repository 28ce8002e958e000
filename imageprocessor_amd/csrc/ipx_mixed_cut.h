// ipx_mixed_cut.h -- how a mixed-size leg orders its files and cuts them: files -> decode groups -> output chunks -> runs of one size
// and kind.  Its one caller is the walk the three legs share (mixed_leg in ipx_mixed_leg.h); `kind` is whatever keeps two files of one size
// out of one operator launch: the frame layout (IPX_PNG_*) for ipx_run_png_png_mixed, the sampling class (0 for Gray, else h0 * 4 + v0)
// for ipx_run_jpeg_jpeg_mixed, 0 for ipx_run_gif_gif_mixed (every frame is paletted).  Plain host C++ with no dependency on the runtime, so that tools/png_mixed_plan_test.cpp and
// tools/jpeg_mixed_plan_test.cpp can hold it to its rules as programs of their own.  DESIGN.md sections 4.10 and 7.
#pragma once

#include <algorithm>
#include <cstddef>
#include <tuple>
#include <vector>

namespace ipx {

// one file as the cut sees it: whether it takes part, its size and kind, the bytes of its decoded frame (what a decode group is
// budgeted by) and the bytes it costs a chunk (its output frames and the encoder's scratch for them)
struct MixItem {
    bool ok;
    int w, h, kind;
    size_t frame_bytes, chunk_bytes;
};
// [first, first + n) are positions in MixCut::order; a group's chunks and a chunk's runs are consecutive
struct MixRun { int first, n; };
struct MixChunk { int first, n, run0, nruns; };
struct MixGroup { int first, n, chunk0, nchunks; };
struct MixCut {
    std::vector<int> order;         // the OK files, by (w, h, kind), ties by index
    std::vector<MixGroup> groups;   // consecutive in order: at most group_files files and group_bytes of frames
    std::vector<MixChunk> chunks;   // consecutive within a group: at most chunk_bytes
    std::vector<MixRun> runs;       // consecutive within a chunk: one size and kind
};

// A file beyond a byte budget still gets a group, or a chunk, of its own; a count limit below 1 counts as 1.
inline MixCut mixed_cut(const MixItem *items, int n, int group_files, size_t group_bytes, size_t chunk_bytes)
{
    MixCut c;
    for (int i = 0; i < n; i++)
        if (items[i].ok) c.order.push_back(i);
    std::stable_sort(c.order.begin(), c.order.end(), [&](int a, int b) {
        return std::make_tuple(items[a].w, items[a].h, items[a].kind) < std::make_tuple(items[b].w, items[b].h, items[b].kind);
    });
    group_files = std::max(group_files, 1);
    const int m = (int)c.order.size();
    auto same = [&](int a, int b) { return items[a].w == items[b].w && items[a].h == items[b].h && items[a].kind == items[b].kind; };
    for (int g0 = 0; g0 < m;) {
        int g1 = g0;
        size_t fb = 0;
        while (g1 < m && g1 - g0 < group_files && (g1 == g0 || fb + items[c.order[g1]].frame_bytes <= group_bytes)) fb += items[c.order[g1++]].frame_bytes;
        MixGroup grp{g0, g1 - g0, (int)c.chunks.size(), 0};
        for (int c0 = g0; c0 < g1;) {
            int c1 = c0;
            size_t cb = 0;
            while (c1 < g1 && (c1 == c0 || cb + items[c.order[c1]].chunk_bytes <= chunk_bytes)) cb += items[c.order[c1++]].chunk_bytes;
            MixChunk ch{c0, c1 - c0, (int)c.runs.size(), 0};
            for (int r0 = c0; r0 < c1;) {
                int r1 = r0 + 1;
                while (r1 < c1 && same(c.order[r0], c.order[r1])) r1++;
                c.runs.push_back(MixRun{r0, r1 - r0});
                ch.nruns++;
                r0 = r1;
            }
            c.chunks.push_back(ch);
            grp.nchunks++;
            c0 = c1;
        }
        c.groups.push_back(grp);
        g0 = g1;
    }
    return c;
}

}  // namespace ipx
