// ipx_png_layout.h -- where one png_decode_files call (ipx_png_dec_runtime.hip) puts the frames and palettes it decodes: a block of
// frames and a block of 1024-byte palette slots, and for every file of the selection its place in each.  Plain host C++ with no
// dependency on the runtime, so that tools/png_mixed_plan_test.cpp can hold the two builders to their rules.  DESIGN.md section 4.10.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

namespace ipx {

struct PngFrameLayout {
    std::vector<int> idx;        // the caller's file index of position g
    std::vector<int> pal_slot;   // palette slot of position g, or -1
    std::vector<size_t> off;     // frame offset of position g, 256-byte aligned
    size_t bytes = 0;            // of the frame block
    int pal_slots = 0;           // of the palette block (slots, 1024 bytes each)
};

// Frames of one size and kind, fs bytes (a multiple of 256) apart, every file with a palette slot (the caller passes no palette block for
// a kind without palettes).  by_index: file i's frame and slot are the i-th of blocks that hold every file of the call, decoded here or
// not (ipx_png_decode_batch; idx ascends); else the g-th of blocks of the selection's own (run_png_png).
inline PngFrameLayout png_layout_strided(std::vector<int> idx, size_t fs, bool by_index)
{
    PngFrameLayout at;
    at.idx = std::move(idx);
    for (size_t g = 0; g < at.idx.size(); g++) {
        const int k = by_index ? at.idx[g] : (int)g;
        at.pal_slot.push_back(k);
        at.off.push_back((size_t)k * fs);
        at.bytes = (size_t)(k + 1) * fs;
        at.pal_slots = k + 1;
    }
    return at;
}

// Frames of any sizes and kinds back to back, each at the next multiple of 256; the paletted files take the slots 0, 1, ... in order
// (ipx_png_decode_mixed, ipx_run_png_png_mixed).  need(i): file i's frame bytes (rows tight) and whether it has a palette.
struct PngFrameNeed { size_t bytes; bool paletted; };
template <class NeedOf> inline PngFrameLayout png_layout_packed(std::vector<int> idx, NeedOf need)
{
    PngFrameLayout at;
    at.idx = std::move(idx);
    for (int i : at.idx) {
        const PngFrameNeed f = need(i);
        at.off.push_back(at.bytes);
        at.pal_slot.push_back(f.paletted ? at.pal_slots++ : -1);
        at.bytes += (f.bytes + 255) & ~(size_t)255;
    }
    return at;
}

}  // namespace ipx
