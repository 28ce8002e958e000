// ipx_png_host.cpp -- the host half of png.Encode: the signature and IHDR image/png's writer puts before the image data of an
// *image.RGBA (colour type 2 when the frame is opaque, else 6; depth 8, compression 0, filter 0, no interlace).  Kernels: ipx_png.hip.
#include <cstring>

#include "ipx_png.h"

namespace ipx {

static uint32_t crc32_bytes(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

static void be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

void png_write_heads(int w, int h, uint8_t out[2][kPngHeadBytes])
{
    for (int v = 0; v < 2; v++) {
        uint8_t *p = out[v];
        memcpy(p, "\x89PNG\r\n\x1a\n", 8);
        be32(p + 8, 13);
        memcpy(p + 12, "IHDR", 4);
        be32(p + 16, (uint32_t)w);
        be32(p + 20, (uint32_t)h);
        p[24] = 8;                 // bit depth
        p[25] = v ? 6 : 2;         // truecolour with alpha / truecolour
        p[26] = p[27] = p[28] = 0; // deflate, adaptive filtering, no interlace
        be32(p + 29, crc32_bytes(p + 12, 17));
    }
}

}  // namespace ipx
