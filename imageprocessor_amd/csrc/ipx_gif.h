// ipx_gif.h -- gif.Encode(w, *image.RGBA, nil) on the GPU: what the kernels (ipx_gif.hip) and the host half (ipx_gif_host.cpp) share.
// Not part of the ABI.  The restatement of Go's writer is in DESIGN.md section 4.7; tests/gif_model.py is the model it is held to.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "ipx_gif_mixed_plan.h"

namespace ipx {

// palette.Plan9 (image/color/palette/gen.go), generated the way gen.go does: for r, v, g, b in 0..3 (nested in that order), i advancing
// 16 per v and j = v - r + 4g + b, den = max(r, g, b); grey 0x11 * v when den == 0, else (r, g, b) * num / den with num = 17 * (4 den + v),
// stored at i + (j & 15).  Every entry is opaque.
struct Plan9 {
    uint8_t rgb[256][3];
    constexpr Plan9() : rgb{}
    {
        int i = 0;
        for (int r = 0; r < 4; r++)
            for (int v = 0; v < 4; v++, i += 16) {
                int j = v - r;
                for (int g = 0; g < 4; g++)
                    for (int b = 0; b < 4; b++, j++) {
                        int den = r > g ? r : g;
                        den = den > b ? den : b;
                        uint8_t *c = rgb[i + (j & 15)];
                        if (den == 0) {
                            c[0] = c[1] = c[2] = (uint8_t)(0x11 * v);
                        } else {
                            const int num = 17 * (4 * den + v);
                            c[0] = (uint8_t)(r * num / den);
                            c[1] = (uint8_t)(g * num / den);
                            c[2] = (uint8_t)(b * num / den);
                        }
                    }
            }
    }
};

// the kGifHeaderBytes of ipx_gif_mixed_plan.h, which also has the bound the regions are cut by (gif_stream_bound) and the rows a
// frame's dither keeps in flight (gif_rows_in_flight)
void gif_write_header(int w, int h, uint8_t out[kGifHeaderBytes]);
// IPX_GIF_WAVES in the environment, read on every call (for measurements): -> whether it is set, *knob its value
inline bool gif_waves_knob(int *knob)
{
    const char *v = getenv("IPX_GIF_WAVES");
    *knob = v && *v ? atoi(v) : 0;
    return v && *v;
}

// ---- kernel launchers (ipx_gif.hip) ----
// rows_in_flight: a multiple of 64 up to 1024 (one wave per 64 rows); carry: n * w int4 of scratch (the last error row of a band)
hipError_t launch_gif_dither(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t *index, int4 *carry,
                             int rows_in_flight, hipStream_t s);
// index: n frames of npix bytes; header: kGifHeaderBytes in HBM; region bytes of out per frame; lens[i] = the stream's length, or
// 0xffffffff if the region was too small (cannot happen with gif_stream_bound; the kernel never writes past the region)
hipError_t launch_gif_lzw(const uint8_t *index, size_t npix, int n, const uint8_t *header, uint8_t *out, size_t region, uint32_t *lens,
                          hipStream_t s);
// stream i (lens[i] bytes at out + i * region) to dst + obase[i]; obase 16-byte aligned, region a multiple of 16
hipError_t launch_gif_pack(const uint8_t *out, size_t region, const uint32_t *lens, const unsigned long long *obase, int n, size_t max_len,
                           uint8_t *dst, hipStream_t s);

// ---- the mixed-size launchers (ipx_gif_mixed.hip): every kernel finds its frame's record, rec[order[...]] or rec[blockIdx.y] ----
// one launch per bucket of plan.buckets: blockDim = the bucket's rows in flight, one workgroup per frame of dorder[first .. first + n)
hipError_t launch_gif_dither_mixed(const GifMixFrame *rec, const uint32_t *dorder, const GifMixBucket *buckets, int nbuckets, uint8_t *index,
                                   int4 *carry, hipStream_t s);
// one wave per frame, frame lorder[blockIdx.x]; header: the kGifHeaderBytes of gif_write_header(0, 0), each wave patches its sizes in;
// lens[f] by the caller's index, as launch_gif_lzw writes them
hipError_t launch_gif_lzw_mixed(const GifMixFrame *rec, const uint32_t *lorder, int n, const uint8_t *index, const uint8_t *header, uint8_t *out,
                                uint32_t *lens, hipStream_t s);
// stream f (lens[f] bytes at out + rec[f].region_off) to dst + obase[f]
hipError_t launch_gif_pack_mixed(const GifMixFrame *rec, const uint8_t *out, const uint32_t *lens, const unsigned long long *obase, int n,
                                 size_t max_len, uint8_t *dst, hipStream_t s);

}  // namespace ipx
