// ipx_ks_generic.hip -- xdraw.BiLinear.Scale (x/image/draw kernelScaler) for any rectangles, either op and every source type: the
// per-operation seam (resize.go:121-125, thumbnail.go:128-131) and the fallback of the batched path for shapes the fused kernel
// (ipx_ks_fused.hip) is not built for.
//
// One thread per destination pixel.  The reference fills tmp[sy][dx] once per source row and destination column and then walks the
// columns; a destination pixel depends on tmp[sy][dx] for the rows sy of its vertical range only, so the thread recomputes those few
// tmp values itself -- the same float64 operations in the same order (horizontal sum in source-column order, times invTotalWeightFFFF;
// vertical sum in source-row order; clamp to alpha; times invTotalWeight; ftou) -- and no float64 image ever goes to HBM.  The price
// is that a tmp value is computed by every destination row that uses it (two for a downscale).  Bound: FP64 VALU and L2 gathers; this
// is not the throughput path.
#include <algorithm>
#include <cstdlib>

#include "ipx_ks_exact.h"

namespace ipx {
namespace {

// one destination pixel (dx, dy relative to dr.Min) of the frame `a` points at
template <int KIND>
__device__ __forceinline__ void ks_pixel(const KsGenArgs &a, int dx, int dy)
{
    const int xlo = a.ax.lo[dx], xn = a.ax.cnt[dx], ylo = a.ay.lo[dy], yn = a.ay.cnt[dy];
    const double *wx = a.ax.w + (size_t)dx * a.ax.ntap, *wy = a.ay.w + (size_t)dy * a.ay.ntap;
    const double xs = a.ax.itwffff[dx], ys = a.ay.itw[dy];
    constexpr bool alpha_one = KIND == IPX_SRC_YCBCR;   // scaleX_YCbCr4xx (and scaleX_Gray) store a literal 1 as tmp alpha

    double qr = 0, qg = 0, qb = 0, qa = 0;
    for (int j = 0; j < yn; j++) {
        double pr = 0, pg = 0, pb = 0, pa = 0;
        for (int i = 0; i < xn; i++) {
            const Tap4 t = ks_tap<KIND>(a, a.sr_x0 + xlo + i, a.sr_y0 + ylo + j);
            const double w = wx[i];
            pr += (double)t.r * w;
            pg += (double)t.g * w;
            pb += (double)t.b * w;
            if (!alpha_one) pa += (double)t.a * w;
        }
        const double w = wy[j];
        qr += (pr * xs) * w;
        qg += (pg * xs) * w;
        qb += (pb * xs) * w;
        qa += (alpha_one ? 1.0 : pa * xs) * w;
    }
    if (qr > qa) qr = qa;
    if (qg > qa) qg = qa;
    if (qb > qa) qb = qa;
    const uint32_t pr0 = ks_ftou(qr * ys), pg0 = ks_ftou(qg * ys), pb0 = ks_ftou(qb * ys), pa0 = ks_ftou(qa * ys);

    uint32_t *d = (uint32_t *)(a.dst + (size_t)(a.dr_y0 + dy) * a.dstride + (size_t)(a.dr_x0 + dx) * 4);
    int op = a.op;
    if (op == IPX_OP_OVER && a.opaque_flag && *a.opaque_flag) op = IPX_OP_SRC;  // draw/scale.go opaque()
    *d = op == IPX_OP_SRC ? pack_src(pr0, pg0, pb0, pa0) : blend_over(*d, pr0, pg0, pb0, pa0);   // scaleY_RGBA_Src / _Over
}

template <int KIND>
__global__ __launch_bounds__(256) void ks_generic_kernel(KsGenArgs a)
{
    a.dst += blockIdx.z * a.dst_fs;      // frame of a batch (all zero for a single frame)
    a.src += blockIdx.z * a.src_fs;
    if (KIND == IPX_SRC_YCBCR || KIND == IPX_SRC_YCBCR_CROP) { a.cb += blockIdx.z * a.c_fs; a.cr += blockIdx.z * a.c_fs; }
    const int dx = a.adr_x0 + (int)(blockIdx.x * 64 + threadIdx.x);
    const int dy = a.adr_y0 + (int)(blockIdx.y * 4 + threadIdx.y);
    if (dx >= a.adr_x1 || dy >= a.adr_y1) return;
    ks_pixel<KIND>(a, dx, dy);
}

// The exact pass behind the one-pass kernel's float pass (ipx_ks_fused.hip): per frame (blockIdx.y) a list of the pixels whose byte the
// float sums could not decide; the ones of output `k` are recomputed here, in float64 and in the reference's order.
// The pass itself is ks_exact_list (ipx_ks_exact.h), which the batch path's ks_tail_kernel runs too.
template <int KIND>
__global__ __launch_bounds__(256) void ks_fix_kernel(KsGenArgs a, const uint2 *list, size_t list_stride, const int *count, int count_stride, int cap, int R)
{
    const int frame = (int)blockIdx.y, n = min(count[(size_t)frame * count_stride], cap);
    list += (size_t)frame * list_stride;
    a.dst += frame * a.dst_fs;
    a.src += frame * a.src_fs;
    if (KIND == IPX_SRC_YCBCR || KIND == IPX_SRC_YCBCR_CROP) { a.cb += frame * a.c_fs; a.cr += frame * a.c_fs; }
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int per_wave = 64 / R, sub = lane / R, sl = lane - sub * R, per_block = ((int)blockDim.x >> 6) * per_wave;
    ks_exact_list<KIND>(a, list, n, (int)blockIdx.x * per_block, (int)gridDim.x * per_block, wv * per_wave + sub, R, sub, sl);
}

}  // namespace

hipError_t launch_ks_generic(const KsGenArgs &a, hipStream_t s)
{
    const int w = a.adr_x1 - a.adr_x0, h = a.adr_y1 - a.adr_y0;
    if (w <= 0 || h <= 0) return hipSuccess;
    dim3 block(64, 4), grid((w + 63) / 64, (h + 3) / 4, a.nframes > 0 ? a.nframes : 1);
    switch (a.kind) {
    case IPX_SRC_NRGBA: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_NRGBA>, grid, block, 0, s, a); break;
    case IPX_SRC_YCBCR: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_YCBCR>, grid, block, 0, s, a); break;
    case IPX_SRC_TAP64: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_TAP64>, grid, block, 0, s, a); break;
    case IPX_SRC_RGBA_CROP: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_RGBA_CROP>, grid, block, 0, s, a); break;
    case IPX_SRC_NRGBA_CROP: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_NRGBA_CROP>, grid, block, 0, s, a); break;
    case IPX_SRC_YCBCR_CROP: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_YCBCR_CROP>, grid, block, 0, s, a); break;
    case IPX_SRC_TAP64_CROP: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_TAP64_CROP>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(ks_generic_kernel<IPX_SRC_RGBA>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_ks_fix(const KsGenArgs &a, const uint2 *list, size_t list_stride, const int *count, int count_stride, int cap, hipStream_t s)
{
    if (a.nframes <= 0 || cap <= 0) return hipSuccess;
    const int R = a.ay.ntap <= 8 ? 8 : a.ay.ntap <= 16 ? 16 : 64;
    // about two thousand blocks in all: two per frame for a batch of 1024 (a photograph leaves a few hundred pixels of an output on
    // its frame's list: a block takes 32 or 16 per pass), more per frame when the batch is small.  Measured per 1024 x 1080p
    // (tools/fix_grid.sh): 8192 blocks 113 + 96 us (most of them find nothing to do), 2048 105 + 63, 1024-thread blocks 108 - 250.
    constexpr int threads = 256, budget = 2048;
    const int per_block = (threads / 64) * (64 / R), most = (cap + per_block - 1) / per_block;
    dim3 block(threads), grid(std::max(1, std::min(most, std::max(1, budget / a.nframes))), a.nframes);
    switch (a.kind) {
    case IPX_SRC_YCBCR: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_YCBCR>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_YCBCR_CROP: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_YCBCR_CROP>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_RGBA_CROP: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_RGBA_CROP>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_RGBA: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_RGBA>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_NRGBA: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_NRGBA>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_NRGBA_CROP: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_NRGBA_CROP>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_TAP64: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_TAP64>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    case IPX_SRC_TAP64_CROP: hipLaunchKernelGGL(ks_fix_kernel<IPX_SRC_TAP64_CROP>, grid, block, 0, s, a, list, list_stride, count, count_stride, cap, R); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ipx
