// ipx_gif.hip -- gif.Encode(w, *image.RGBA, nil) on the GPU (image/gif writer.go, image/draw drawPaletted, compress/lzw writer.go) and
// the ABI entries built on it.  Kernels: the Plan 9 / Floyd-Steinberg dither (a wavefront, rows in flight across lanes), LZW (one wave
// per frame, one lane coding, the dictionary in LDS) and the packing of the finished streams into one block -- here for n frames of one
// size, frame i found by arithmetic; their bodies are ipx_gif_kernels.h's, which the mixed-size kernels (ipx_gif_mixed.hip) share.
// Host half: ipx_gif_host.cpp.  DESIGN.md section 4.7 has the restatement and the numbers.
#include <memory>
#include <vector>

#include "ipx_gif_kernels.h"
#include "ipx_runtime_internal.h"

namespace ipx {

// ---- dither: gif_dither_frame on frame blockIdx.x of n frames of one size --------------------------------------------------------
__global__ __launch_bounds__(1024) void gif_dither_kernel(const uint8_t *__restrict__ src, int w, int h, int stride, size_t frame_stride,
                                                          uint8_t *__restrict__ index, int4 *__restrict__ carry)
{
    gif_dither_frame(src + (size_t)blockIdx.x * frame_stride, w, h, stride, index + (size_t)blockIdx.x * w * h, carry + (size_t)blockIdx.x * w);
}

hipError_t launch_gif_dither(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t *index, int4 *carry,
                             int rows_in_flight, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_dither_kernel, dim3(n), dim3(rows_in_flight), 0, s, src, w, h, stride, frame_stride, index, carry);
    return hipGetLastError();
}

// ---- LZW: gif_lzw_frame on frame blockIdx.x, behind the one header every frame of the launch has ---------------------------------
__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t *__restrict__ index, size_t npix, const uint8_t *__restrict__ header,
                                                     uint8_t *__restrict__ out, size_t region, uint32_t *__restrict__ lens)
{
    const int lane = threadIdx.x;
    uint8_t *o = out + (size_t)blockIdx.x * region;
    for (int i = lane; i < kGifHeaderBytes; i += 64) o[i] = header[i];
    const uint32_t word = gif_lzw_frame(index + (size_t)blockIdx.x * npix, npix, o, region);
    if (lane == 0) lens[blockIdx.x] = word;
}

hipError_t launch_gif_lzw(const uint8_t *index, size_t npix, int n, const uint8_t *header, uint8_t *out, size_t region, uint32_t *lens,
                          hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_lzw_kernel, dim3(n), dim3(64), 0, s, index, npix, header, out, region, lens);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gif_pack_kernel(const uint8_t *__restrict__ out, size_t region, const uint32_t *__restrict__ lens,
                                                       const unsigned long long *__restrict__ obase, uint8_t *__restrict__ dst)
{
    const int f = blockIdx.y;
    gif_pack_stream(out + (size_t)f * region, lens[f], dst + obase[f]);
}

hipError_t launch_gif_pack(const uint8_t *out, size_t region, const uint32_t *lens, const unsigned long long *obase, int n, size_t max_len,
                           uint8_t *dst, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_pack_kernel, dim3(gif_pack_blocks(max_len), n), dim3(256), 0, s, out, region, lens, obase, dst);
    return hipGetLastError();
}

}  // namespace ipx

// ---- the entries -----------------------------------------------------------------------------------------------------------------

static int gif_check(const char *who, const void *src, int w, int h, long long stride, int n)
{
    if (!src || n < 0 || w <= 0 || h <= 0 || stride < (long long)w * 4) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    if (w >= 1 << 16 || h >= 1 << 16) { set_error("gif: image is too large to encode"); return IPX_ERR_INVALID; }
    return IPX_OK;
}

// rows in flight per frame of a call of n frames: the rule of ipx_gif_mixed_plan.h, which the mixed-size core applies frame by frame
static int gif_call_rows(int h, int n)
{
    int knob;
    const bool has_knob = gif_waves_knob(&knob);
    return gif_rows_in_flight(h, n, has_knob, knob);
}

// Asynchronous: the scratch is a stream-ordered allocation of s.
static int gif_dither(hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t *index)
{
    AsyncFree mem{s, {}};
    int4 *carry;
    IPX_HIP(mem.get(&carry, (size_t)n * w * sizeof(int4)));
    IPX_HIP(launch_gif_dither(src, w, h, stride, frame_stride, n, index, carry, gif_call_rows(h, n), s));
    return IPX_OK;
}

// n frames in HBM -> streams in one pinned block (ipx_host_alloc), everything on stream s; returns once the block is filled
int gif_encode_core(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                           uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    uint8_t hdr[kGifHeaderBytes];
    gif_write_header(w, h, hdr);
    std::vector<uint32_t> hl(n);
    std::vector<unsigned long long> ob(n);
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    const size_t npix = (size_t)w * h, region = align256(gif_stream_bound(w, h));
    uint8_t *didx, *dout, *dhdr;
    uint32_t *dlens;
    unsigned long long *dob;
    IPX_HIP(mem.get(&didx, npix * n));
    IPX_HIP(mem.get(&dout, region * n));
    IPX_HIP(mem.get(&dhdr, sizeof hdr));
    IPX_HIP(mem.get(&dlens, (size_t)n * 4));
    IPX_HIP(mem.get(&dob, (size_t)n * 8));
    IPX_HIP(hipMemcpyAsync(dhdr, hdr, sizeof hdr, hipMemcpyHostToDevice, s));
    int rc = gif_dither(s, src, w, h, stride, frame_stride, n, didx);
    if (rc) return rc;
    IPX_HIP(launch_gif_lzw(didx, npix, n, dhdr, dout, region, dlens, s));
    IPX_HIP(hipMemcpyAsync(hl.data(), dlens, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    size_t total = 0, max_len = 0;
    for (int i = 0; i < n; i++) {
        if (hl[i] == 0xffffffffu || hl[i] > region) { set_error("gif: stream of frame %d overran its bound", i); return IPX_ERR_INVALID; }
        offs[i] = total;
        lens[i] = hl[i];
        ob[i] = total;
        total += align16(hl[i]);
        max_len = std::max<size_t>(max_len, hl[i]);
    }
    uint8_t *dpack;
    IPX_HIP(mem.get(&dpack, total));
    IPX_HIP(hipMemcpyAsync(dob, ob.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    IPX_HIP(launch_gif_pack(dout, region, dlens, dob, n, max_len, dpack, s));
    return download_streams(ctx, s, dpack, total, "gif ", blob);
}

extern "C" {

int ipx_dev_gif_dither_rgba8(ipx_ctx *ctx, void *stream, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                             uint8_t *index) try
{
    IPX_ENTER(ctx);
    int rc = gif_check("ipx_dev_gif_dither_rgba8", src, w, h, stride, n);
    if (rc) return rc;
    if (!index) { set_error("ipx_dev_gif_dither_rgba8: bad argument"); return IPX_ERR_INVALID; }
    if (n == 0) return IPX_OK;
    return gif_dither(stream ? (hipStream_t)stream : ctx->stream, src, w, h, stride, frame_stride, n, index);
}
IPX_CATCH_STATUS

int ipx_gif_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                             size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    if (!blob || !offs || !lens) { set_error("ipx_gif_encode_batch_dev: bad argument"); return IPX_ERR_INVALID; }
    *blob = nullptr;
    int rc = gif_check("ipx_gif_encode_batch_dev", src, w, h, stride, n);
    if (rc) return rc;
    if (n == 0) return IPX_OK;
    LaneLease lane(ctx);
    return gif_encode_core(ctx, lane->stream, src, w, h, stride, frame_stride, n, blob, offs, lens);
}
IPX_CATCH_STATUS

int ipx_gif_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, uint8_t **out, size_t *len) try
{
    IPX_ENTER(ctx);
    return encode_one_rgba8("ipx_gif_encode_rgba8", ctx, gif_check, gif_encode_core, pix, w, h, stride, out, len);
}
IPX_CATCH_STATUS

// The GIF task's GPU leg (resize.go:78-91, thumbnail.go:68-81 with gif.Encode; watermark.go:66-79, where a GIF watermark becomes a JPEG):
// chunks of paletted frames go up, the operators run, resize and thumbnail outputs are GIF-encoded and the
// watermark output JPEG-encoded, all in HBM; only the streams come back, into pinned blocks owned by *result.
int ipx_plan_run_host_paletted_gif(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *index, int stride, size_t frame_stride,
                                   const uint8_t *palettes, int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out,
                                   ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    return run_host_streams("ipx_plan_run_host_paletted_gif", ctx, pl, n, packed_src(kSrcPaletted, index, stride, frame_stride, palettes), Codec::Gif,
                            Codec::Gif, Codec::Jpeg, "IPX_HOST_CHUNK_GIF", 64, quality, resize_out, thumb_out, wm_out, result);
}
IPX_CATCH_STATUS

}  // extern "C"
