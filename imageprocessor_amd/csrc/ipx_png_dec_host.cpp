// ipx_png_dec_host.cpp -- the host half of png.Decode: image/png's reader.go over the chunk headers only (signature, IHDR, PLTE, tRNS,
// the IDAT run, IEND; unknown ancillary chunks skipped), never the image data.  It decides the rules that need no inflate, the file's
// frame layout and raw length, the palette with tRNS applied, and the chunk spans the CRC kernel checks.  Kernels: ipx_png_dec.hip;
// driver and entries: ipx_png_dec_runtime.hip.  DESIGN.md section 4.10.
#include <cstring>

#include "ipx_internal.h"
#include "ipx_png_dec.h"

namespace ipx {

namespace {

inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// the legal (colour type, depth) pairs of parseIHDR
bool legal(int ctype, int depth)
{
    switch (ctype) {
    case 0: return depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    case 3: return depth == 1 || depth == 2 || depth == 4 || depth == 8;
    case 2: case 4: case 6: return depth == 8 || depth == 16;
    default: return false;
    }
}

int channels(int ctype) { return ctype == 0 || ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 2 ? 3 : 4; }

}  // namespace

int png_parse(const uint8_t *p, size_t n, bool adam7, PngFileInfo *info)
{
    PngFileInfo &f = *info;
    f.status = 0;
    f.w = f.h = 0;
    f.kind = -1;
    f.trns = false;
    f.interlace = false;
    f.crc.clear();
    f.idat.clear();
    f.idat_len = 0;
    f.idat_last = 0;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    if (!p || n < 8 || memcmp(p, sig, 8)) return f.status = IPX_ERR_INVALID;
    if (n >= ((size_t)1 << 31)) return f.status = IPX_ERR_UNSUPPORTED;
    enum { kStart, kIHDR, kPLTE, kTRNS, kIDAT } stage = kStart;
    int np = 0;                     // PLTE entries
    bool idat_open = false;         // the last chunk read was an IDAT
    uint8_t plte[768], alpha[256];
    memset(alpha, 255, sizeof alpha);
    size_t i = 8;
    for (;;) {
        if (n - i < 12) return f.status = IPX_ERR_INVALID;                  // the file ends before IEND (io.ErrUnexpectedEOF)
        const uint32_t len = be32(p + i);
        if (len > n - i - 12) return f.status = IPX_ERR_INVALID;
        const uint8_t *type = p + i + 4, *d = p + i + 8;
        f.crc.push_back(PngSpan{(uint32_t)(i + 4), len + 4});
        const bool was_idat = idat_open;
        idat_open = false;
        if (!memcmp(type, "IHDR", 4)) {
            if (stage != kStart || len != 13) return f.status = IPX_ERR_INVALID;
            const int32_t w = (int32_t)be32(d), h = (int32_t)be32(d + 4);
            f.depth = d[8];
            f.ctype = d[9];
            if (d[10] != 0 || d[11] != 0 || d[12] > 1 || w <= 0 || h <= 0 || !legal(f.ctype, f.depth)) return f.status = IPX_ERR_INVALID;
            if (d[12] == 1 && !adam7) return f.status = IPX_ERR_UNSUPPORTED;   // Adam7 without the caller's switch
            f.interlace = d[12] == 1;
            f.w = w;
            f.h = h;
            stage = kIHDR;
        } else if (stage == kStart) {
            // Go answers chunkOrderError for the known chunks; an unknown first chunk is not restated
            const bool known = !memcmp(type, "PLTE", 4) || !memcmp(type, "tRNS", 4) || !memcmp(type, "IDAT", 4) || !memcmp(type, "IEND", 4);
            return f.status = known ? IPX_ERR_INVALID : IPX_ERR_UNSUPPORTED;
        } else if (!memcmp(type, "PLTE", 4)) {
            if (stage != kIHDR) return f.status = IPX_ERR_INVALID;
            np = (int)(len / 3);
            if (len % 3 || np <= 0 || np > 256 || (f.depth < 16 && np > (1 << f.depth))) return f.status = IPX_ERR_INVALID;
            if (f.ctype == 0 || f.ctype == 4) return f.status = IPX_ERR_INVALID;   // PLTE, color type mismatch
            memcpy(plte, d, len);
            if (f.ctype != 3) np = 0;                                        // ignored on truecolour
            stage = kPLTE;
        } else if (!memcmp(type, "tRNS", 4)) {
            if (f.ctype == 4 || f.ctype == 6) return f.status = IPX_ERR_INVALID;   // tRNS, color type mismatch
            if (f.ctype == 3) {
                if (stage != kPLTE) return f.status = IPX_ERR_INVALID;
                if (len > 256) return f.status = IPX_ERR_INVALID;
                if ((int)len > np) return f.status = IPX_ERR_UNSUPPORTED;   // entries past the palette: not restated
                memcpy(alpha, d, len);
            } else {
                if (stage == kPLTE) return f.status = IPX_ERR_UNSUPPORTED;  // truecolour tRNS after an ignored PLTE: not restated
                if (stage != kIHDR) return f.status = IPX_ERR_INVALID;
                if (len != (f.ctype == 0 ? 2u : 6u)) return f.status = IPX_ERR_INVALID;
                const int ns = f.ctype == 0 ? 1 : 3;
                for (int k = 0; k < ns; k++) {
                    f.trns_v[k] = (uint16_t)(d[2 * k] << 8 | d[2 * k + 1]);
                    if (f.depth < 16 && f.trns_v[k] >= (1u << f.depth)) return f.status = IPX_ERR_UNSUPPORTED;
                }
                if (f.ctype == 0 && f.depth < 8) return f.status = IPX_ERR_UNSUPPORTED;
                f.trns = true;
            }
            stage = kTRNS;
        } else if (!memcmp(type, "IDAT", 4)) {
            if (f.ctype == 3 && stage < kPLTE) return f.status = IPX_ERR_INVALID;   // a palette image without PLTE
            if (stage == kIDAT && !was_idat) return f.status = IPX_ERR_UNSUPPORTED;   // IDAT after another chunk
            f.idat.push_back(PngSpan{(uint32_t)(i + 8), len});
            f.idat_last = f.idat_len;
            f.idat_len += len;
            stage = kIDAT;
            idat_open = true;
        } else if (!memcmp(type, "IEND", 4)) {
            if (stage != kIDAT || len != 0) return f.status = IPX_ERR_INVALID;
            f.file_len = (uint32_t)(i + 12);
            break;
        } else if (!(type[0] & 0x20)) {
            return f.status = IPX_ERR_UNSUPPORTED;                          // an unknown critical chunk: not restated
        }
        i += 12 + (size_t)len;
    }
    // the frame layout of the type Go returns
    const int bits = channels(f.ctype) * f.depth;
    f.bpp = bits >= 8 ? bits / 8 : 1;
    f.rowbytes = (uint32_t)(1 + ((uint64_t)bits * f.w + 7) / 8);
    f.raw_len = (uint64_t)f.h * f.rowbytes;
    if (f.interlace) {
        // each non-empty pass is an image of its own: ph rows of a filter byte and pw pixels; an empty pass has no bytes at all
        f.raw_len = 0;
        for (int k = 0; k < 7; k++) {
            const PngPass ps = png_pass(k);
            const uint64_t pw = png_pass_dim((uint32_t)f.w, ps.xo, ps.xf), ph = png_pass_dim((uint32_t)f.h, ps.yo, ps.yf);
            if (pw && ph) f.raw_len += ph * (1 + ((uint64_t)bits * pw + 7) / 8);
        }
    }
    switch (f.ctype) {
    case 0: f.kind = f.depth == 16 ? (f.trns ? IPX_PNG_NRGBA64 : IPX_PNG_GRAY16) : (f.trns ? IPX_PNG_NRGBA : IPX_PNG_GRAY); break;
    case 2: f.kind = f.depth == 16 ? (f.trns ? IPX_PNG_NRGBA64 : IPX_PNG_RGBA64) : (f.trns ? IPX_PNG_NRGBA : IPX_PNG_RGBA); break;
    case 3: f.kind = IPX_PNG_PALETTED; break;
    default: f.kind = f.depth == 16 ? IPX_PNG_NRGBA64 : IPX_PNG_NRGBA; break;
    }
    const int kb = png_kind_bpp(f.kind);
    if (!frame_span_ok(f.w, f.h, (long long)f.w * kb, kb) || f.raw_len >= ((uint64_t)1 << 32)) return f.status = IPX_ERR_UNSUPPORTED;
    if (f.kind == IPX_PNG_PALETTED) {
        // parsePLTE: 256 opaque entries, black past the chunk's; tRNS turns the first ones into color.NRGBA
        for (int k = 0; k < 256; k++) {
            uint8_t *e = f.pal + 4 * k;
            if (k < np) { e[0] = plte[3 * k]; e[1] = plte[3 * k + 1]; e[2] = plte[3 * k + 2]; e[3] = alpha[k]; }
            else { e[0] = e[1] = e[2] = 0; e[3] = 255; }
        }
    }
    return f.status = IPX_OK;
}

}  // namespace ipx
