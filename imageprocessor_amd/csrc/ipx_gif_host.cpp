// ipx_gif_host.cpp -- the host half of gif.Encode: the header bytes image/gif's writeHeader / writeImageBlock put before the LZW data of
// a single-frame *image.Paletted with the Plan 9 palette.  (The size bound the device regions are cut by: ipx_gif_mixed_plan.h.)
// Kernels: ipx_gif.hip, ipx_gif_mixed.hip.
#include <cstring>

#include "ipx_gif.h"

namespace ipx {

void gif_write_header(int w, int h, uint8_t out[kGifHeaderBytes])
{
    static constexpr Plan9 pal;
    uint8_t *p = out;
    memcpy(p, "GIF89a", 6);
    p += 6;
    auto u16 = [&](int v) { *p++ = (uint8_t)(v & 0xff); *p++ = (uint8_t)((v >> 8) & 0xff); };
    u16(w);
    u16(h);
    *p++ = 0x80 | 7;   // fColorTable | log2(256) - 1
    *p++ = 0;          // background index
    *p++ = 0;          // pixel aspect ratio
    memcpy(p, pal.rgb, 768);
    p += 768;
    // no NETSCAPE2.0 block (one frame) and no graphic control extension (delay 0, disposal 0, Plan 9 has no transparent entry)
    *p++ = 0x2C;
    u16(0);
    u16(0);
    u16(w);
    u16(h);
    *p++ = 0;          // the global table serves: no local one
    *p++ = 8;          // LZW minimum code size: log2(256) - 1 + 1
}

}  // namespace ipx
