// ipx_gif_dec_host.cpp -- the host half of gif.Decode: image/gif's reader.go up to the first image's LZW data (header, tables,
// extensions, descriptor, transparency, code size), the sub-block framing of that data, and the bound the code scratch is cut by.
// Kernels and entries: ipx_gif_dec.hip.  DESIGN.md section 4.8.
#include <algorithm>
#include <cstring>

#include "ipx_gif_dec.h"
#include "ipx_internal.h"

namespace ipx {

namespace {

struct Cursor {
    const uint8_t *p;
    size_t n, i = 0;
    bool byte(uint8_t *v) { if (i >= n) return false; *v = p[i++]; return true; }
    bool skip(size_t k) { if (k > n - i) return false; i += k; return true; }
};

// readColorTable: 1 << (1 + (fields & 7)) opaque entries
bool read_table(Cursor &c, uint8_t fields, uint8_t pal[1024], uint32_t *len)
{
    const uint32_t k = 1u << (1 + (fields & 7));
    if ((size_t)3 * k > c.n - c.i) return false;
    memset(pal, 0, 1024);
    for (uint32_t e = 0; e < k; e++) {
        memcpy(pal + 4 * e, c.p + c.i + 3 * e, 3);
        pal[4 * e + 3] = 255;
    }
    c.i += 3 * k;
    *len = k;
    return true;
}

}  // namespace

int gif_parse(const uint8_t *p, size_t n, GifFileInfo *info)
{
    GifFileInfo &f = *info;
    f = GifFileInfo();
    if (!p) return f.status = IPX_ERR_INVALID;
    if (n >= ((size_t)1 << 31)) return f.status = IPX_ERR_UNSUPPORTED;
    Cursor c{p, n};
    if (n < 13 || (memcmp(p, "GIF87a", 6) && memcmp(p, "GIF89a", 6))) return f.status = IPX_ERR_INVALID;
    const int sw = p[6] | p[7] << 8, sh = p[8] | p[9] << 8;
    c.i = 13;
    uint8_t gpal[1024];
    uint32_t glen = 0;
    bool has_global = false;
    if (p[10] & 0x80) {
        if (!read_table(c, p[10], gpal, &glen)) return f.status = IPX_ERR_INVALID;
        has_global = true;
    }
    bool has_trans = false;
    uint8_t trans = 0;
    for (;;) {          // the blocks before the first image
        uint8_t b;
        if (!c.byte(&b)) return f.status = IPX_ERR_INVALID;
        if (b == 0x2C) break;
        if (b != 0x21) return f.status = IPX_ERR_INVALID;          // the trailer ("missing image data") or an unknown block
        uint8_t label;
        if (!c.byte(&label)) return f.status = IPX_ERR_INVALID;
        if (label == 0xF9) {                                        // readGraphicControl: six bytes, no sub-blocks after them
            if (c.n - c.i < 6) return f.status = IPX_ERR_INVALID;
            const uint8_t *g = p + c.i;
            if (g[0] != 4 || g[5] != 0) return f.status = IPX_ERR_INVALID;
            if (g[1] & 1) { has_trans = true; trans = g[4]; }
            c.i += 6;
            continue;
        }
        if (label == 0x01) {
            if (!c.skip(13)) return f.status = IPX_ERR_INVALID;
        } else if (label == 0xFF) {
            uint8_t sz;
            if (!c.byte(&sz) || !c.skip(sz)) return f.status = IPX_ERR_INVALID;
        } else if (label != 0xFE) {
            return f.status = IPX_ERR_INVALID;                      // unknown extension
        }
        for (;;) {
            uint8_t sz;
            if (!c.byte(&sz)) return f.status = IPX_ERR_INVALID;
            if (sz == 0) break;
            if (!c.skip(sz)) return f.status = IPX_ERR_INVALID;
        }
    }
    if (c.n - c.i < 9) return f.status = IPX_ERR_INVALID;
    const uint8_t *d = p + c.i;
    c.i += 9;
    f.left = d[0] | d[1] << 8;
    f.top = d[2] | d[3] << 8;
    f.w = d[4] | d[5] << 8;
    f.h = d[6] | d[7] << 8;
    const uint8_t fields = d[8];
    if (f.left + f.w > sw || f.top + f.h > sh) return f.status = IPX_ERR_INVALID;   // "frame bounds larger than image bounds"
    f.interlaced = (fields & 0x40) != 0;
    if (fields & 0x80) {
        if (!read_table(c, fields, f.pal, &f.pal_len)) return f.status = IPX_ERR_INVALID;
    } else {
        if (!has_global) return f.status = IPX_ERR_INVALID;                          // "no color table"
        memcpy(f.pal, gpal, 1024);
        f.pal_len = glen;
    }
    if (has_trans) {        // the zero colour; an index past the table lengthens it with zero colours (golang.org/issue/15059)
        memset(f.pal + 4 * trans, 0, 4);
        f.pal_len = std::max<uint32_t>(f.pal_len, (uint32_t)trans + 1);
    }
    uint8_t lit;
    if (!c.byte(&lit) || lit < 2 || lit > 8) return f.status = IPX_ERR_INVALID;
    f.lit = lit;
    // the image data's sub-blocks as blockReader.fill delivers them: one the file cuts short is not delivered
    f.data_pos = c.i;
    for (;;) {
        uint8_t sz;
        if (!c.byte(&sz)) break;
        if (sz == 0) { f.terminated = true; break; }
        if (!c.skip(sz)) break;
        f.last_start = f.data_len;
        f.last_is_one = sz == 1;
        f.data_len += sz;
    }
    // what the GPU path does not take (Go decodes these itself)
    if (f.left != 0 || f.top != 0 || f.w == 0 || f.h == 0 || !frame_span_ok(f.w, f.h, f.w, 1)) return f.status = IPX_ERR_UNSUPPORTED;
    return f.status = IPX_OK;
}

void gif_gather(const uint8_t *p, size_t n, const GifFileInfo &info, uint8_t *dst)
{
    size_t i = info.data_pos, o = 0;
    while (o < info.data_len && i < n) {
        const size_t sz = p[i++];
        memcpy(dst + o, p + i, sz);
        o += sz;
        i += sz;
    }
}

uint32_t gif_code_cap(const GifFileInfo &info)
{
    const uint64_t by_bits = (uint64_t)info.data_len * 8 / (uint64_t)(info.lit + 1);
    const uint64_t by_pix = (uint64_t)info.w * (uint64_t)info.h;
    return (uint32_t)std::min(by_bits, by_pix) + 1;
}

}  // namespace ipx
