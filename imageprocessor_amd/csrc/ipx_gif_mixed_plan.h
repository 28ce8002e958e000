// ipx_gif_mixed_plan.h -- the per-frame records of a mixed-size gif.Encode (gif_encode_mixed_core, ipx_gif_mixed.hip): frames of any
// sizes go through the dither, the LZW coder and the packing together; what the uniform kernels (ipx_gif.hip) take as launch arguments
// (w, h, stride, npix, region, blockIdx.x * something) a mixed kernel reads from its frame's record.  Also the two rules both cores
// share: the bound a frame's region is cut by and the rows a frame's dither keeps in flight.  Plain C++ with no dependency on the
// runtime, shared by the kernels' launchers, the driver and tools/gif_mixed_plan_test.cpp, which holds the builder to its rules as a
// program of its own.  DESIGN.md section 4.7.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ipx_align.h"

namespace ipx {

// GIF89a, logical screen w x h with the 256-entry global table (flags 0x87, background 0, aspect 0), the Plan 9 table, the image
// descriptor (0x2C, at 0,0, w x h, flags 0: the frame uses the global table) and the LZW minimum code size 8
constexpr int kGifHeaderBytes = 13 + 768 + 10 + 1;
// where gif_write_header puts a frame's size, little-endian u16 each: the logical screen's width and height, the image descriptor's
// (0x2C, left, top, then width and height) -- the only bytes of the header that depend on the frame
constexpr int kGifHdrScreenW = 6, kGifHdrScreenH = 8, kGifHdrImageW = 13 + 768 + 5, kGifHdrImageH = 13 + 768 + 7;

// an upper bound of a whole stream's length for a w x h frame (header, sub-blocks of LZW data at <= 12 bits per code, trailer)
inline size_t gif_stream_bound(int w, int h)
{
    const size_t npix = (size_t)w * (size_t)h;
    // a code per pixel at most, plus the first clear code, the code Close writes, EOF, and a clear code per 3838 codes (hi runs 257 .. 4095)
    const size_t codes = npix + 3 + npix / 3838 + 1;
    const size_t data = (codes * 12 + 7) / 8;
    return kGifHeaderBytes + data + (data + 254) / 255 + 1 + 1;   // length bytes, terminator, trailer
}

// rows in flight per frame: a wave per 64 rows, more waves per frame while the call's n frames alone would leave the CUs idle (a
// band's 2R-step ramp costs idle lanes, which only matters once every SIMD has a frame).  knob: IPX_GIF_WAVES when has_knob (for
// measurements), clamped to 1 .. 16 waves.
inline int gif_rows_in_flight(int h, int n, bool has_knob, int knob)
{
    const int waves = has_knob ? knob : std::min({16, (h + 63) / 64, 2048 / std::max(n, 1)});
    return 64 * std::max(1, std::min(16, waves));
}

// what the caller says of a frame: RGBA8 in HBM
struct GifMixSrc { const uint8_t *src; int32_t w, h, stride; };

// one frame, in HBM
struct GifMixFrame {
    const uint8_t *src;
    unsigned long long index_off;    // its w * h indices in the index arena (bytes; 256-byte aligned)
    unsigned long long carry_off;    // its w int4s in the carry arena (in int4s: the last error row of a band)
    unsigned long long region_off;   // its region in the stream arena (bytes; 256-byte aligned) ...
    unsigned long long region;       // ... and the region's size: align256(gif_stream_bound(w, h))
    int32_t w, h, stride;
    int32_t rows;                    // rows in flight: its dither workgroup's threads
};
static_assert(sizeof(GifMixFrame) == 56, "one record per frame, read as scalars");

// the frames of one dither launch: order[first .. first + n), every one with `rows` rows in flight
struct GifMixBucket { int32_t rows, first, n; };

struct GifMixPlan {
    std::vector<GifMixFrame> frames;         // in the caller's order
    std::vector<uint32_t> dither_order;      // a permutation of the frames: bucket by bucket, within a bucket the costliest first
    std::vector<GifMixBucket> buckets;       // by ascending rows; at most 16
    std::vector<uint32_t> lzw_order;         // a permutation of the frames: the most pixels first (a launch ends with its longest frame)
    unsigned long long index_bytes = 0, carry_int4s = 0, region_bytes = 0;
    unsigned long long max_region = 0;
};

// steps of frame f's dither workgroup: bands of `rows` rows, each w + 2 (rows - 1) + 1 steps long
inline unsigned long long gif_mix_dither_steps(const GifMixFrame &f)
{
    const unsigned long long bands = ((unsigned long long)f.h + f.rows - 1) / f.rows;
    return bands * ((unsigned long long)f.w + 2ull * (f.rows - 1) + 1);
}

// The records of n frames, in the order given, and the launch orders.  Every sum is kept in 64 bits.  false when a frame cannot be
// encoded: a side below 1 or beyond 65535, or a stride below 4 * w.
inline bool gif_mix_build(const GifMixSrc *in, int n, bool has_knob, int knob, GifMixPlan *out)
{
    *out = GifMixPlan{};
    if (n <= 0) return n == 0;
    out->frames.assign((size_t)n, GifMixFrame{});
    for (int i = 0; i < n; i++) {
        const GifMixSrc &f = in[i];
        if (f.w < 1 || f.h < 1 || f.w > 65535 || f.h > 65535 || (long long)f.stride < (long long)f.w * 4) return false;
        GifMixFrame &g = out->frames[(size_t)i];
        g.src = f.src;
        g.w = f.w; g.h = f.h; g.stride = f.stride;
        g.rows = gif_rows_in_flight(f.h, n, has_knob, knob);
        g.index_off = out->index_bytes;
        g.carry_off = out->carry_int4s;
        g.region_off = out->region_bytes;
        g.region = align256(gif_stream_bound(f.w, f.h));
        out->index_bytes += align256((size_t)f.w * (size_t)f.h);
        out->carry_int4s += (unsigned long long)f.w;
        out->region_bytes += g.region;
        out->max_region = std::max(out->max_region, g.region);
    }
    const std::vector<GifMixFrame> &fr = out->frames;
    out->dither_order.resize((size_t)n);
    out->lzw_order.resize((size_t)n);
    for (int i = 0; i < n; i++) out->dither_order[(size_t)i] = out->lzw_order[(size_t)i] = (uint32_t)i;
    std::stable_sort(out->dither_order.begin(), out->dither_order.end(), [&](uint32_t a, uint32_t b) {
        if (fr[a].rows != fr[b].rows) return fr[a].rows < fr[b].rows;
        return gif_mix_dither_steps(fr[a]) > gif_mix_dither_steps(fr[b]);
    });
    std::stable_sort(out->lzw_order.begin(), out->lzw_order.end(), [&](uint32_t a, uint32_t b) {
        return (unsigned long long)fr[a].w * fr[a].h > (unsigned long long)fr[b].w * fr[b].h;
    });
    for (int p = 0; p < n; p++) {
        const int rows = fr[out->dither_order[(size_t)p]].rows;
        if (out->buckets.empty() || out->buckets.back().rows != rows) out->buckets.push_back(GifMixBucket{rows, p, 0});
        out->buckets.back().n++;
    }
    return true;
}

}  // namespace ipx
