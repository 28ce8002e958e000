// ipx_device.h -- device-side arithmetic shared by the kernels.  Include after
// `#pragma clang fp contract(off)`: the float64 lerp must round every product before the add.
#pragma once

#include "ipx_internal.h"

namespace ipx {
namespace {

constexpr uint32_t kM = 0xffffu;

// color.YCbCrToRGB on 8-bit samples (the uint32 overflow test of the Go code): R | G << 8 | B << 16 | 0xff << 24, as imageutil.DrawYCbCr
// stores a pixel
__device__ __forceinline__ uint32_t ycbcr_to_rgb8(uint32_t y, uint32_t cb, uint32_t cr)
{
    const int32_t yy1 = (int32_t)y * 0x10101, cb1 = (int32_t)cb - 128, cr1 = (int32_t)cr - 128;
    int32_t r = yy1 + 91881 * cr1, g = yy1 - 22554 * cb1 - 46802 * cr1, b = yy1 + 116130 * cb1;
    r = ((uint32_t)r & 0xff000000u) == 0 ? r >> 16 : ~(r >> 31);
    g = ((uint32_t)g & 0xff000000u) == 0 ? g >> 16 : ~(g >> 31);
    b = ((uint32_t)b & 0xff000000u) == 0 ? b >> 16 : ~(b >> 31);
    return ((uint32_t)r & 0xffu) | (((uint32_t)g & 0xffu) << 8) | (((uint32_t)b & 0xffu) << 16) | 0xff000000u;
}

// v * 0x101 for byte `C` of a packed RGBA dword, as float64
template <int C>
__device__ __forceinline__ double widen(uint32_t px)
{
    // v_perm_b32: bytes {0, 0, b, b} -> b * 0x101 in one instruction
    constexpr uint32_t sel = 0x0c0c0000u | (uint32_t)C | ((uint32_t)C << 8);
    return (double)__builtin_amdgcn_perm(0u, px, sel);
}

// one output channel: the three lerps of scale_RGBA_RGBA_*, products rounded separately
template <int C>
__device__ __forceinline__ uint32_t lerp_channel(uint32_t p00, uint32_t p10, uint32_t p01,
                                                 uint32_t p11, double xw0, double xw1, double yw0,
                                                 double yw1)
{
    const double s00 = widen<C>(p00), s10 = widen<C>(p10);
    const double s01 = widen<C>(p01), s11 = widen<C>(p11);
    const double top = xw0 * s00 + xw1 * s10;
    const double bot = xw0 * s01 + xw1 * s11;
    const double v = yw0 * top + yw1 * bot;
    return (uint32_t)v;  // truncation, as Go's uint32(float64)
}

__device__ __forceinline__ uint32_t pack_src(uint32_t pr, uint32_t pg, uint32_t pb, uint32_t pa)
{
    // uint8(p >> 8) per channel; p <= 0xffff
    return (pr >> 8) | (pg & 0xff00u) | ((pb & 0xff00u) << 8) | ((pa & 0xff00u) << 16);
}

__device__ __forceinline__ uint32_t blend_over(uint32_t d, uint32_t pr, uint32_t pg, uint32_t pb,
                                               uint32_t pa)
{
    // scale_RGBA_RGBA_Over: dst = uint8((uint32(dst)*pa1/0xffff + p) >> 8), pa1 = (0xffff-pa)*0x101
    const uint32_t pa1 = (kM - pa) * 0x101u;
    const uint32_t r = (((d & 0xffu) * pa1 / kM + pr) >> 8) & 0xffu;
    const uint32_t g = ((((d >> 8) & 0xffu) * pa1 / kM + pg) >> 8) & 0xffu;
    const uint32_t b = ((((d >> 16) & 0xffu) * pa1 / kM + pb) >> 8) & 0xffu;
    const uint32_t a = (((d >> 24) * pa1 / kM + pa) >> 8) & 0xffu;
    return r | (g << 8) | (b << 16) | (a << 24);
}

// ---------------------------------------------------------------------------------------------
// drawGlyphOver for one pixel and one mask value; uint32 arithmetic wraps exactly as in Go
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t glyph_over(uint32_t d, uint32_t mask8, uint32_t sr, uint32_t sg,
                                               uint32_t sb, uint32_t sa)
{
    const uint32_t ma = mask8 | (mask8 << 8);
    const uint32_t a = (kM - (sa * ma / kM)) * 0x101u;
    const uint32_t r = (((d & 0xffu) * a + sr * ma) / kM >> 8) & 0xffu;
    const uint32_t g = ((((d >> 8) & 0xffu) * a + sg * ma) / kM >> 8) & 0xffu;
    const uint32_t b = ((((d >> 16) & 0xffu) * a + sb * ma) / kM >> 8) & 0xffu;
    const uint32_t al = (((d >> 24) * a + sa * ma) / kM >> 8) & 0xffu;
    return r | (g << 8) | (b << 16) | (al << 24);
}

// all glyphs, in string order, on the pixel (x, y)
__device__ __forceinline__ uint32_t glyph_run(uint32_t d, int x, int y, const DevGlyph *__restrict__ gl,
                                              int n, uint32_t sr, uint32_t sg, uint32_t sb,
                                              uint32_t sa)
{
    for (int g = 0; g < n; g++) {
        const DevGlyph G = gl[g];
        if (x >= G.x0 && x < G.x1 && y >= G.y0 && y < G.y1) {
            const uint32_t m = G.mask[(size_t)(y - G.y0) * G.mstride + (x - G.x0)];
            if (m) d = glyph_over(d, m, sr, sg, sb, sa);
        }
    }
    return d;
}

// The text walk of the stand-alone composites (composite_kernel, ks_tail_kernel): the glyph table `tab` (LDS) four glyphs at a time on
// a lane's pixels d[r][k] = (x + k, ybase + YSTEP * r): rectangle tests from the table, the mask bytes of the glyphs that hold a pixel
// loaded together (the PX bytes of a row packed into a dword), then the composites in string order -- a step costs one global latency
// instead of one per glyph.  A ballot skips steps no lane of the wave touches.
template <int PX, int ROWS, int YSTEP>
__device__ __forceinline__ void glyph_walk(const DevGlyph *tab, int n, int x, int ybase, Rect bbox, uint32_t (&d)[ROWS][PX], uint32_t sr,
                                           uint32_t sg, uint32_t sb, uint32_t sa)
{
    static_assert(PX >= 1 && PX <= 4, "a row's mask bytes travel in one dword");
    for (int g = 0; g < n; g += 4) {
        uint32_t m[4][ROWS];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const DevGlyph G = tab[min(g + j, n - 1)];
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const int y = ybase + YSTEP * r;
                const bool iny = g + j < n && y >= G.y0 && y < G.y1 && y < bbox.y1;
                uint32_t mm = 0u;
#pragma unroll
                for (int k = 0; k < PX; k++) {
                    const bool in = iny && x + k >= G.x0 && x + k < G.x1;
                    mm |= (in ? (uint32_t)G.mask[(size_t)(y - G.y0) * G.mstride + (x + k - G.x0)] : 0u) << (8 * k);
                    any |= in;
                }
                m[j][r] = mm;
            }
        }
        if (!__any(any)) continue;  // wave-uniform skip
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int r = 0; r < ROWS; r++)
#pragma unroll
                for (int k = 0; k < PX; k++) {
                    const uint32_t mk = (m[j][r] >> (8 * k)) & 0xffu;
                    if (mk) d[r][k] = glyph_over(d[r][k], mk, sr, sg, sb, sa);
                }
    }
}

}  // namespace
}  // namespace ipx
