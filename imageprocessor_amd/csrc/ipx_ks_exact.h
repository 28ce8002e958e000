// ipx_ks_exact.h -- device code of the kernel scaler's float64 per-pixel paths, shared by ipx_ks_generic.hip (ks_generic_kernel,
// ks_fix_kernel) and ipx_ks_tail.hip (ks_tail_kernel): how a source pixel becomes the four 16-bit values scaleX weights, ftou, and the
// exact pass over a list of destination pixels.  The same float64 operations in the reference's order everywhere; only how the loads
// are issued differs between the callers.
#pragma once

#include "ipx_ks.h"

#pragma clang fp contract(off)

#include "ipx_device.h"

namespace ipx {
namespace {

struct Tap4 { uint32_t r, g, b, a; };

// kinds whose source pixel is one dword (a lane's taps of one source row are then contiguous bytes)
template <int KIND> constexpr bool ks_dword_kind = KIND == IPX_SRC_RGBA || KIND == IPX_SRC_NRGBA || KIND == IPX_SRC_RGBA_CROP || KIND == IPX_SRC_NRGBA_CROP;

// the four values of a dword kind from the pixel's dword
template <int KIND>
__device__ __forceinline__ Tap4 ks_tap_px(uint32_t p)
{
    Tap4 t;
    if (KIND == IPX_SRC_NRGBA || KIND == IPX_SRC_NRGBA_CROP) {
        t.a = (p >> 24) * 0x101u;
        t.r = (p & 0xffu) * t.a / 0xffu;
        t.g = ((p >> 8) & 0xffu) * t.a / 0xffu;
        t.b = ((p >> 16) & 0xffu) * t.a / 0xffu;
        if (KIND == IPX_SRC_NRGBA_CROP) { t.r = (t.r >> 8) * 0x101u; t.g = (t.g >> 8) * 0x101u; t.b = (t.b >> 8) * 0x101u; }
    } else {
        const uint32_t al = p >> 24;
        uint32_t r = p & 0xffu, g = (p >> 8) & 0xffu, b = (p >> 16) & 0xffu;
        if (KIND == IPX_SRC_RGBA_CROP) { r = min(r, al); g = min(g, al); b = min(b, al); }
        t.r = r * 0x101u; t.g = g * 0x101u; t.b = b * 0x101u; t.a = al * 0x101u;
    }
    return t;
}

// the four 16-bit values scaleX_<type> weights for the source pixel (x, y); see ipx_ks.h for the kinds
template <int KIND>
__device__ __forceinline__ Tap4 ks_tap(const KsGenArgs &a, int x, int y)
{
    Tap4 t;
    if (KIND == IPX_SRC_YCBCR || KIND == IPX_SRC_YCBCR_CROP) {
        const int cx = x >> ycbcr_hshift(a.ratio), cy = y >> ycbcr_vshift(a.ratio);   // COffset: x, x / 2 or (4:1:1, 4:1:0) x / 4; y or y / 2
        const size_t ci = (size_t)cy * a.cstride + cx;
        const int yy1 = (int)a.src[(size_t)y * a.sstride + x] * 0x10101;
        const int cb1 = (int)a.cb[ci] - 128, cr1 = (int)a.cr[ci] - 128;
        t.r = (uint32_t)min(max((yy1 + 91881 * cr1) >> 8, 0), 0xffff);
        t.g = (uint32_t)min(max((yy1 - 22554 * cb1 - 46802 * cr1) >> 8, 0), 0xffff);
        t.b = (uint32_t)min(max((yy1 + 116130 * cb1) >> 8, 0), 0xffff);
        t.a = 0xffffu;
        if (KIND == IPX_SRC_YCBCR_CROP) { t.r = (t.r >> 8) * 0x101u; t.g = (t.g >> 8) * 0x101u; t.b = (t.b >> 8) * 0x101u; }
    } else if (KIND == IPX_SRC_TAP64 || KIND == IPX_SRC_TAP64_CROP) {
        const uint2 p = *(const uint2 *)(a.src + (size_t)y * a.sstride + (size_t)x * 8);
        t.r = p.x & 0xffffu; t.g = p.x >> 16; t.b = p.y & 0xffffu; t.a = p.y >> 16;
        if (KIND == IPX_SRC_TAP64_CROP) {
            t.r = (min(t.r, t.a) >> 8) * 0x101u; t.g = (min(t.g, t.a) >> 8) * 0x101u; t.b = (min(t.b, t.a) >> 8) * 0x101u;
            t.a = (t.a >> 8) * 0x101u;
        }
    } else {
        t = ks_tap_px<KIND>(*(const uint32_t *)(a.src + (size_t)y * a.sstride + (size_t)x * 4));
    }
    return t;
}

__device__ __forceinline__ uint32_t ks_ftou(double f)   // impl.go ftou
{
    const int i = (int)(0xffff * f + 0.5);
    return i > 0xffff ? 0xffffu : (i > 0 ? (uint32_t)i : 0u);
}

// four pixels that are only known to start on a dword boundary (a global dwordx4 load asks for no more)
struct __attribute__((packed, aligned(4))) KsPx4 { uint32_t p[4]; };

// scaleX's sum for tmp[y][dx]: the `xn` taps from source column `x` on, times their weights, in source-column order.
// Dword kinds with a.src_w set take the taps in 16-byte pieces -- one line request per piece instead of one per tap -- wherever the
// piece ends inside the row (src_w pixels); the last piece of a row, and every piece when src_w is 0, goes dword by dword.
template <int KIND>
__device__ __forceinline__ void ks_row_sum(const KsGenArgs &a, int x, int y, int xn, const double *wx, double &pr, double &pg, double &pb, double &pa)
{
    constexpr bool alpha_one = KIND == IPX_SRC_YCBCR;   // scaleX_YCbCr4xx (and scaleX_Gray) store a literal 1 as tmp alpha
    if constexpr (ks_dword_kind<KIND>) {
        const uint8_t *row = a.src + (size_t)y * a.sstride + (size_t)x * 4;
#pragma unroll 2
        for (int t = 0; t < xn; t += 4) {                                 // (the pieces' loads do not wait for one another)
            uint32_t p[4];
            double w[4];
            if (x + t + 4 <= a.src_w) {
                const KsPx4 q = *(const KsPx4 *)(row + (size_t)t * 4);
#pragma unroll
                for (int k = 0; k < 4; k++) p[k] = q.p[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) p[k] = t + k < xn ? *(const uint32_t *)(row + (size_t)(t + k) * 4) : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = t + k < xn ? wx[t + k] : 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (t + k < xn) {
                    const Tap4 tp = ks_tap_px<KIND>(p[k]);
                    pr += (double)tp.r * w[k];
                    pg += (double)tp.g * w[k];
                    pb += (double)tp.b * w[k];
                    pa += (double)tp.a * w[k];
                }
        }
    } else {
#pragma unroll 4
        for (int t = 0; t < xn; t++) {                                    // (the taps' loads do not wait for one another)
            const Tap4 tp = ks_tap<KIND>(a, x + t, y);
            const double w = wx[t];
            pr += (double)tp.r * w;
            pg += (double)tp.g * w;
            pb += (double)tp.b * w;
            if (!alpha_one) pa += (double)tp.a * w;
        }
    }
}

// The exact pass over one frame's list of one output: entries base + off, base + step + off, ... below n (base and step are the same
// for every lane of the block, `off` is the lane's pixel among the block's; `a` already points at the frame).
// R lanes per pixel (R = 4, 8, 16 or 64, at least the vertical tap count where that is at most 64): lane j of a pixel's group walks
// source row j from left to right -- scaleX's sum for tmp[row][dx], in source-column order -- and the group's values are then added in
// source-row order, one after the other as scaleY does, in every lane of the group (the first one stores).  A thread per pixel would
// walk nx * ny taps one after the other: 1936 dependent steps for an 8K frame's thumbnail, 0.7 ms for a batch of two frames.
// A pass is a chain of dependent round trips (list entry -> lo / cnt / itwffff of its column and row -> taps).  The entry of the pass
// after the next and the table values of the next pass are fetched before this pass's taps are consumed, so a pass exposes one
// (itw of the row included: it used to be a round trip of its own in front of the store).
template <int KIND>
__device__ __forceinline__ void ks_exact_list(const KsGenArgs &a, const uint2 *list, int n, int base, int step, int off, int R, int sub, int sl)
{
    constexpr bool alpha_one = KIND == IPX_SRC_YCBCR;
    struct Cols { int xlo, xn, ylo, yn; double xs, ys; bool live; };
    auto entry = [&](int i0) {                                            // (dy, dx); a row no output has where the list ends
        const int i = i0 + off;
        return i < n ? list[i] : make_uint2(0x7fffffffu, 0u);
    };
    auto cols = [&](uint2 e) {
        Cols c;
        const int dy = (int)e.x, dx = (int)e.y;
        c.live = dx < a.adr_x1 && dy < a.adr_y1;
        c.xlo = c.live ? a.ax.lo[dx] : 0; c.xn = c.live ? a.ax.cnt[dx] : 0; c.ylo = c.live ? a.ay.lo[dy] : 0; c.yn = c.live ? a.ay.cnt[dy] : 0;
        c.xs = c.live ? a.ax.itwffff[dx] : 0.0; c.ys = c.live ? a.ay.itw[dy] : 0.0;
        return c;
    };
    if (base >= n) return;
    uint2 e = entry(base), e1 = entry(base + step);
    Cols c = cols(e);
    for (int i0 = base; i0 < n; i0 += step) {
        const uint2 e2 = entry(i0 + 2 * step);
        const Cols c1 = cols(e1);
        const int dy = (int)e.x, dx = (int)e.y;
        const bool live = c.live;
        const int xlo = c.xlo, xn = c.xn, ylo = c.ylo, yn = c.yn;
        const double *wx = a.ax.w + (size_t)(live ? dx : 0) * a.ax.ntap, *wy = a.ay.w + (size_t)(live ? dy : 0) * a.ay.ntap;
        const double xs = c.xs;
        double qr = 0, qg = 0, qb = 0, qa = 0;
        for (int jb = 0; __any(jb < yn); jb += R) {                      // (wave-uniform) R source rows at a time, top to bottom
            const int j = jb + sl;
            double pr = 0, pg = 0, pb = 0, pa = 0;
            if (j < yn) ks_row_sum<KIND>(a, a.sr_x0 + xlo, a.sr_y0 + ylo + j, xn, wx, pr, pg, pb, pa);
            const double tr = pr * xs, tg = pg * xs, tb = pb * xs, ta = alpha_one ? 1.0 : pa * xs;
            const double wl = j < yn ? wy[j] : 0.0;                       // the row's vertical weight travels with its sums (a load per
                                                                          // step of the loop below was a memory round trip per row)
            for (int jj = 0; jj < R; jj++) {                              // every lane of the group adds the group's rows in order
                const int from = sub * R + jj;
                const double vr = __shfl(tr, from), vg = __shfl(tg, from), vb = __shfl(tb, from), va = __shfl(ta, from);
                const double w = __shfl(wl, from);
                if (jb + jj < yn) {
                    qr += vr * w;
                    qg += vg * w;
                    qb += vb * w;
                    qa += va * w;
                }
            }
        }
        if (live && sl == 0) {
            const double ys = c.ys;
            if (qr > qa) qr = qa;
            if (qg > qa) qg = qa;
            if (qb > qa) qb = qa;
            const uint32_t pr0 = ks_ftou(qr * ys), pg0 = ks_ftou(qg * ys), pb0 = ks_ftou(qb * ys), pa0 = ks_ftou(qa * ys);
            *(uint32_t *)(a.dst + (size_t)(a.dr_y0 + dy) * a.dstride + (size_t)(a.dr_x0 + dx) * 4) = pack_src(pr0, pg0, pb0, pa0);
        }
        e = e1; e1 = e2; c = c1;
    }
}

}  // namespace
}  // namespace ipx
