// ipx_png.hip -- png.Encode(w, *image.RGBA) on the GPU and the ABI entries built on it.  Kernels: the opacity reduction (colour type
// 2 or 6), the un-premultiply and filter pass (a workgroup per row: the filter of a row depends only on raw bytes), the deflate of one
// segment of whole rows per workgroup (match candidates, greedy parse, histograms, Huffman tables, bit emission by prefix sum, CRC-32
// and Adler sums), the per-frame head and tail and the pack of the finished pieces.  What is done to a row, a segment and a frame's tail
// lives in ipx_png_kernels.h and ipx_png_deflate_body.inc, shared with the mixed-size kernels of ipx_png_mixed.hip.  Host half: ipx_png_host.cpp.  The restatement and
// the stream's definition: DESIGN.md section 4.9; tests/png_model.py is the model the bytes are held to.
#include <vector>

#include "ipx_png.h"
#include "ipx_png_kernels.h"
#include "ipx_runtime_internal.h"

namespace ipx {

// ---- opacity ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_opacity_kernel(const uint8_t *__restrict__ src, int w, int h, int stride, size_t frame_stride,
                                                          uint32_t *__restrict__ alpha)
{
    const uint8_t *f = src + (size_t)blockIdx.y * frame_stride;
    const size_t npix = (size_t)w * h;
    int any = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
        const size_t y = i / w, x = i - y * w;
        any |= f[y * stride + 4 * x + 3] != 0xFF;
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(alpha + blockIdx.y, 1u);
}

hipError_t launch_png_opacity(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint32_t *alpha, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min<size_t>(512, ((size_t)w * h + 4095) / 4096);
    hipLaunchKernelGGL(png_opacity_kernel, dim3(blocks, n), dim3(256), 0, s, src, w, h, stride, frame_stride, alpha);
    return hipGetLastError();
}

// ---- un-premultiply and filter ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t *__restrict__ src, int w, int stride, size_t frame_stride,
                                                         const uint32_t *__restrict__ alpha, uint8_t *__restrict__ filt, size_t fbytes)
{
    const int y = blockIdx.x, f = blockIdx.y;
    const int bpp = alpha[f] ? 4 : 3, rb = w * bpp;
    const uint8_t *row = src + (size_t)f * frame_stride + (size_t)y * stride;
    const uint8_t *prev = y > 0 ? row - stride : nullptr;
    png_filter_row(row, prev, rb, bpp, filt + (size_t)f * fbytes + (size_t)y * (rb + 1));
}

hipError_t launch_png_filter(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, const uint32_t *alpha,
                             uint8_t *filt, size_t fbytes, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_filter_kernel, dim3(h, n), dim3(256), 0, s, src, w, stride, frame_stride, alpha, filt, fbytes);
    return hipGetLastError();
}

// ---- deflate of one segment ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDefThreads) void png_deflate_kernel(const uint8_t *__restrict__ filt, uint32_t *__restrict__ match,
                                                                  size_t fbytes, int w, int h, const uint32_t *__restrict__ alpha,
                                                                  const PngSeg *__restrict__ segs, uint8_t *__restrict__ out,
                                                                  uint32_t *__restrict__ lens, uint32_t *__restrict__ adler)
{
    __shared__ uint32_t table[kHashSize];   // phase 1: the hash table; phase 2: the walk's window
    __shared__ DefShared S;
    const int t = threadIdx.x;
    const PngSeg sg = segs[blockIdx.x];
    const int bpp = alpha[sg.frame] ? 4 : 3, stride = 1 + w * bpp;
    const uint32_t N = (uint32_t)h * stride, s0 = sg.s0, s1 = sg.s1, L = s1 - s0;
    const bool first = sg.flags & 1, last = sg.flags & 2;
    const uint8_t *data = filt + (size_t)sg.frame * fbytes;
    uint32_t *M = match + (size_t)sg.frame * fbytes;
    uint8_t *o = out + sg.out;

#include "ipx_png_deflate_body.inc"
}

hipError_t launch_png_deflate(const uint8_t *filt, uint32_t *match, size_t fbytes, int w, int h, const uint32_t *alpha, const PngSeg *segs,
                              int nseg, uint8_t *out, uint32_t *lens, uint32_t *adler, hipStream_t s)
{
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_deflate_kernel, dim3(nseg), dim3(kDefThreads), 0, s, filt, match, fbytes, w, h, alpha, segs, out, lens, adler);
    return hipGetLastError();
}

// ---- head, tail, pack ------------------------------------------------------------------------------------------------------------
__global__ void png_frame_kernel(const uint8_t *__restrict__ heads, const uint32_t *__restrict__ alpha, const uint32_t *__restrict__ item0,
                                 const PngSeg *__restrict__ segs, const uint32_t *__restrict__ adler, uint8_t *__restrict__ out,
                                 size_t region, size_t tail)
{
    const int f = blockIdx.x, t = threadIdx.x;
    uint8_t *o = out + (size_t)f * region;
    const uint8_t *hd = heads + (alpha[f] ? kPngHeadBytes : 0);
    for (int i = t; i < kPngHeadBytes; i += blockDim.x) o[i] = hd[i];
    if (t != 0) return;
    png_frame_tail(segs, adler, item0[f], item0[f + 1], o + tail);
}

hipError_t launch_png_frame(const uint8_t *heads, const uint32_t *alpha, const uint32_t *item0, const PngSeg *segs, const uint32_t *adler,
                            int n, uint8_t *out, size_t region, size_t tail, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_frame_kernel, dim3(n), dim3(64), 0, s, heads, alpha, item0, segs, adler, out, region, tail);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void png_pack_kernel(const uint8_t *__restrict__ out, const PngPiece *__restrict__ pieces,
                                                       uint8_t *__restrict__ dst)
{
    const PngPiece pc = pieces[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < pc.len; i += blockDim.x) dst[pc.dst + i] = out[pc.src + i];
}

hipError_t launch_png_pack(const uint8_t *out, const PngPiece *pieces, int npieces, uint8_t *dst, hipStream_t s)
{
    if (npieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_pack_kernel, dim3(npieces), dim3(256), 0, s, out, pieces, dst);
    return hipGetLastError();
}

}  // namespace ipx

// ---- the entries -----------------------------------------------------------------------------------------------------------------

static int png_check(const char *who, const void *src, int w, int h, long long stride, int n)
{
    if (!src || n < 0 || w <= 0 || h <= 0 || stride < (long long)w * 4) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    if (!frame_span_ok(w, h, (long long)w * 4, 4)) { set_error("%s: %dx%d is beyond the frames the encoder addresses", who, w, h); return IPX_ERR_UNSUPPORTED; }
    return IPX_OK;
}

// n frames in HBM -> streams in one pinned block (ipx_host_alloc), everything on stream s; returns once the block is filled
int ipx::png_encode_core(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                           uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    uint8_t heads[2][kPngHeadBytes];
    png_write_heads(w, h, heads);
    std::vector<uint32_t> alpha(n), item0(n + 1), sl;
    std::vector<PngSeg> segs;
    std::vector<PngPiece> pieces;
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    const size_t fbytes = align256((size_t)h * (1 + 4 * (size_t)w));
    const size_t tail = kPngSegBase + std::max(png_segs_bytes(w, h, 3), png_segs_bytes(w, h, 4)), region = align256(tail + kPngTailBytes);
    uint32_t *dalpha;
    IPX_HIP(mem.get(&dalpha, (size_t)n * 4));
    IPX_HIP(hipMemsetAsync(dalpha, 0, (size_t)n * 4, s));
    IPX_HIP(launch_png_opacity(src, w, h, stride, frame_stride, n, dalpha, s));
    IPX_HIP(hipMemcpyAsync(alpha.data(), dalpha, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // the segments of every frame, by its colour type
    for (int f = 0; f < n; f++) {
        item0[f] = (uint32_t)segs.size();
        png_append_segs(&segs, (uint32_t)f, w, h, alpha[f] ? 4 : 3, (size_t)f * region);
    }
    item0[n] = (uint32_t)segs.size();
    const int nseg = (int)segs.size();
    uint8_t *dfilt, *dout, *dheads;
    uint32_t *dmatch, *dlens, *dadler, *ditem0;
    PngSeg *dsegs;
    IPX_HIP(mem.get(&dfilt, fbytes * n));
    IPX_HIP(mem.get(&dmatch, fbytes * n * 4));
    IPX_HIP(mem.get(&dout, region * n));
    IPX_HIP(mem.get(&dheads, sizeof heads));
    IPX_HIP(mem.get(&dlens, (size_t)nseg * 4));
    IPX_HIP(mem.get(&dadler, (size_t)nseg * 8));
    IPX_HIP(mem.get(&ditem0, (size_t)(n + 1) * 4));
    IPX_HIP(mem.get(&dsegs, (size_t)nseg * sizeof(PngSeg)));
    IPX_HIP(hipMemcpyAsync(dheads, heads, sizeof heads, hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(ditem0, item0.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(dsegs, segs.data(), (size_t)nseg * sizeof(PngSeg), hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemsetAsync(dout, 0, region * n, s));
    IPX_HIP(launch_png_filter(src, w, h, stride, frame_stride, n, dalpha, dfilt, fbytes, s));
    IPX_HIP(launch_png_deflate(dfilt, dmatch, fbytes, w, h, dalpha, dsegs, nseg, dout, dlens, dadler, s));
    IPX_HIP(launch_png_frame(dheads, dalpha, ditem0, dsegs, dadler, n, dout, region, tail, s));
    sl.resize(nseg);
    IPX_HIP(hipMemcpyAsync(sl.data(), dlens, (size_t)nseg * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // the pieces: head, the segments' chunks, tail, frame after frame, each stream starting 16-byte aligned
    pieces.reserve(nseg + 2 * (size_t)n);
    size_t total = 0;
    for (int f = 0; f < n; f++) {
        offs[f] = total;
        if (!(lens[f] = png_place_pieces(&pieces, segs, sl, item0[f], item0[f + 1], (size_t)f * region, tail, &total))) return IPX_ERR_INVALID;
    }
    uint8_t *dpack;
    PngPiece *dpieces;
    IPX_HIP(mem.get(&dpack, total));
    IPX_HIP(mem.get(&dpieces, pieces.size() * sizeof(PngPiece)));
    IPX_HIP(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(PngPiece), hipMemcpyHostToDevice, s));
    IPX_HIP(launch_png_pack(dout, dpieces, (int)pieces.size(), dpack, s));
    return download_streams(ctx, s, dpack, total, "png ", blob);
}

extern "C" {

int ipx_png_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                             size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    if (!blob || !offs || !lens) { set_error("ipx_png_encode_batch_dev: bad argument"); return IPX_ERR_INVALID; }
    *blob = nullptr;
    int rc = png_check("ipx_png_encode_batch_dev", src, w, h, stride, n);
    if (rc) return rc;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_png_encode_batch_dev: at most 65535 frames per call"); return IPX_ERR_UNSUPPORTED; }
    LaneLease lane(ctx);
    return png_encode_core(ctx, lane->stream, src, w, h, stride, frame_stride, n, blob, offs, lens);
}
IPX_CATCH_STATUS

int ipx_png_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, uint8_t **out, size_t *len) try
{
    IPX_ENTER(ctx);
    return encode_one_rgba8("ipx_png_encode_rgba8", ctx, png_check, png_encode_core, pix, w, h, stride, out, len);
}
IPX_CATCH_STATUS

// The PNG task's GPU leg (resize.go:83, thumbnail.go:73, watermark.go:71 with png.Encode): chunks of RGBA frames go up, the operators
// run, every output is PNG-encoded in HBM; only the streams come back, into pinned blocks owned by *result.
int ipx_plan_run_host_png(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                          ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    return run_host_streams("ipx_plan_run_host_png", ctx, pl, n, packed_src(kSrcRGBA, src, sstride, src_frame_stride), Codec::Png, Codec::Png,
                            Codec::Png, "IPX_HOST_CHUNK_PNG", 64, 0, resize_out, thumb_out, wm_out, result);
}
IPX_CATCH_STATUS

}  // extern "C"
