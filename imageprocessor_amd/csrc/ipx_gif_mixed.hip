// ipx_gif_mixed.hip -- gif.Encode of n RGBA8 frames of ANY sizes on the GPU: the kernels of ipx_gif.hip with a record per frame
// (GifMixFrame, built by ipx_gif_mixed_plan.h) in place of one geometry per launch, the core that drives them and
// ipx_gif_encode_mixed_dev.  What is done to a pixel, a code or a byte is ipx_gif_kernels.h's, shared with the uniform kernels; a
// kernel here only finds its frame.  DESIGN.md section 4.7.
#include <vector>

#include "ipx_gif_kernels.h"
#include "ipx_runtime_internal.h"

namespace ipx {

// One workgroup per frame of a bucket: every frame of order[0 .. gridDim.x) has blockDim.x rows in flight, so no thread of a workgroup
// is surplus and a frame's band loop is as long as its own width and rows make it.  The record is read through a uniform index: every
// thread of the workgroup gets the same frame and reaches every barrier of gif_dither_frame.
__global__ __launch_bounds__(1024) void gif_dither_mixed_kernel(const GifMixFrame *__restrict__ rec, const uint32_t *__restrict__ order,
                                                                uint8_t *__restrict__ index, int4 *__restrict__ carry)
{
    const GifMixFrame f = rec[order[blockIdx.x]];
    gif_dither_frame(f.src, f.w, f.h, f.stride, index + f.index_off, carry + f.carry_off);
}

hipError_t launch_gif_dither_mixed(const GifMixFrame *rec, const uint32_t *dorder, const GifMixBucket *buckets, int nbuckets, uint8_t *index,
                                   int4 *carry, hipStream_t s)
{
    for (int b = 0; b < nbuckets; b++) {
        const GifMixBucket &k = buckets[b];
        if (k.n <= 0) continue;
        hipLaunchKernelGGL(gif_dither_mixed_kernel, dim3(k.n), dim3(k.rows), 0, s, rec, dorder + k.first, index, carry);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One wave per frame, the longest frames in the first workgroups.  The header is the template of gif_write_header(0, 0): the wave
// copies it and writes its frame's width and height over the four size fields (the logical screen's and the image descriptor's,
// little-endian u16 each), then codes into its own region.
__global__ __launch_bounds__(64) void gif_lzw_mixed_kernel(const GifMixFrame *__restrict__ rec, const uint32_t *__restrict__ order,
                                                           const uint8_t *__restrict__ index, const uint8_t *__restrict__ header,
                                                           uint8_t *__restrict__ out, uint32_t *__restrict__ lens)
{
    const int lane = threadIdx.x;
    const uint32_t fi = order[blockIdx.x];
    const GifMixFrame f = rec[fi];
    uint8_t *o = out + f.region_off;
    for (int i = lane; i < kGifHeaderBytes; i += 64) {
        uint8_t b = header[i];
        if (i == kGifHdrScreenW || i == kGifHdrImageW) b = (uint8_t)(f.w & 0xff);
        else if (i == kGifHdrScreenW + 1 || i == kGifHdrImageW + 1) b = (uint8_t)(f.w >> 8);
        else if (i == kGifHdrScreenH || i == kGifHdrImageH) b = (uint8_t)(f.h & 0xff);
        else if (i == kGifHdrScreenH + 1 || i == kGifHdrImageH + 1) b = (uint8_t)(f.h >> 8);
        o[i] = b;
    }
    const uint32_t word = gif_lzw_frame(index + f.index_off, (size_t)f.w * (size_t)f.h, o, (size_t)f.region);
    if (lane == 0) lens[fi] = word;
}

hipError_t launch_gif_lzw_mixed(const GifMixFrame *rec, const uint32_t *lorder, int n, const uint8_t *index, const uint8_t *header, uint8_t *out,
                                uint32_t *lens, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_lzw_mixed_kernel, dim3(n), dim3(64), 0, s, rec, lorder, index, header, out, lens);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gif_pack_mixed_kernel(const GifMixFrame *__restrict__ rec, const uint8_t *__restrict__ out,
                                                             const uint32_t *__restrict__ lens, const unsigned long long *__restrict__ obase,
                                                             uint8_t *__restrict__ dst)
{
    const int f = blockIdx.y;
    gif_pack_stream(out + rec[f].region_off, lens[f], dst + obase[f]);
}

hipError_t launch_gif_pack_mixed(const GifMixFrame *rec, const uint8_t *out, const uint32_t *lens, const unsigned long long *obase, int n,
                                 size_t max_len, uint8_t *dst, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_pack_mixed_kernel, dim3(gif_pack_blocks(max_len), n), dim3(256), 0, s, rec, out, lens, obase, dst);
    return hipGetLastError();
}

}  // namespace ipx

// gif.Encode of n frames of ANY sizes in HBM -> streams in one pinned block, with the two waits for the device of gif_encode_core -- the
// lengths back, the streams down -- whatever sizes the call holds: one dither launch per bucket of rows in flight (at most 16, queued
// back to back), one LZW launch, one packing launch.  The index bytes, the carry rows and the regions are one arena each, cut by the
// records; stream i is byte for byte what gif_encode_core writes for frame i alone.  Frames are taken as checked
// (ipx_gif_encode_mixed_dev checks them; the leg's come from plans).  n <= 65535 keeps the packing grid's y dimension in range.
int gif_encode_mixed_core(ipx_ctx *ctx, hipStream_t s, const GifMixSrc *frames, int n, uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n <= 0) return IPX_OK;
    int knob;
    const bool has_knob = gif_waves_knob(&knob);
    GifMixPlan plan;
    if (!gif_mix_build(frames, n, has_knob, knob, &plan)) { set_error("gif: a frame of the call cannot be encoded"); return IPX_ERR_INVALID; }
    uint8_t hdr[kGifHeaderBytes];
    gif_write_header(0, 0, hdr);
    // one upload: the records, then the two launch orders
    const size_t rec_bytes = align256((size_t)n * sizeof(GifMixFrame)), ord_bytes = align256((size_t)n * 4);
    std::vector<uint8_t> up(rec_bytes + 2 * ord_bytes);
    memcpy(up.data(), plan.frames.data(), (size_t)n * sizeof(GifMixFrame));
    memcpy(up.data() + rec_bytes, plan.dither_order.data(), (size_t)n * 4);
    memcpy(up.data() + rec_bytes + ord_bytes, plan.lzw_order.data(), (size_t)n * 4);
    std::vector<uint32_t> hl(n);
    std::vector<unsigned long long> ob(n);
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    uint8_t *dup, *didx, *dout, *dhdr;
    int4 *dcarry;
    uint32_t *dlens;
    unsigned long long *dob;
    IPX_HIP(mem.get(&dup, up.size()));
    IPX_HIP(mem.get(&didx, (size_t)plan.index_bytes));
    IPX_HIP(mem.get(&dcarry, (size_t)plan.carry_int4s * sizeof(int4)));
    IPX_HIP(mem.get(&dout, (size_t)plan.region_bytes));
    IPX_HIP(mem.get(&dhdr, sizeof hdr));
    IPX_HIP(mem.get(&dlens, (size_t)n * 4));
    IPX_HIP(mem.get(&dob, (size_t)n * 8));
    IPX_HIP(hipMemcpyAsync(dup, up.data(), up.size(), hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(dhdr, hdr, sizeof hdr, hipMemcpyHostToDevice, s));
    const GifMixFrame *drec = (const GifMixFrame *)dup;
    const uint32_t *ddord = (const uint32_t *)(dup + rec_bytes), *dlord = (const uint32_t *)(dup + rec_bytes + ord_bytes);
    IPX_HIP(launch_gif_dither_mixed(drec, ddord, plan.buckets.data(), (int)plan.buckets.size(), didx, dcarry, s));
    IPX_HIP(launch_gif_lzw_mixed(drec, dlord, n, didx, dhdr, dout, dlens, s));
    IPX_HIP(hipMemcpyAsync(hl.data(), dlens, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    size_t total = 0, max_len = 0;
    for (int i = 0; i < n; i++) {
        if (hl[i] == 0xffffffffu || hl[i] > plan.frames[i].region) { set_error("gif: stream of frame %d overran its bound", i); return IPX_ERR_INVALID; }
        offs[i] = total;
        lens[i] = hl[i];
        ob[i] = total;
        total += align16(hl[i]);
        max_len = std::max<size_t>(max_len, hl[i]);
    }
    uint8_t *dpack;
    IPX_HIP(mem.get(&dpack, total));
    IPX_HIP(hipMemcpyAsync(dob, ob.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    IPX_HIP(launch_gif_pack_mixed(drec, dout, dlens, dob, n, max_len, dpack, s));
    return download_streams(ctx, s, dpack, total, "gif ", blob);
}

extern "C" int ipx_gif_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, uint8_t **blob, size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    const auto encodable = [](const char *, int, const ipx_rgba_frame &fr) -> int {
        if (fr.w < 1 << 16 && fr.h < 1 << 16) return IPX_OK;
        set_error("gif: image is too large to encode");
        return IPX_ERR_INVALID;
    };
    const int rc = rgba_frames_check("ipx_gif_encode_mixed_dev", frames, n, blob, offs, lens, encodable, true);
    if (rc || n == 0) return rc;
    std::vector<GifMixSrc> src((size_t)n);
    for (int f = 0; f < n; f++) src[(size_t)f] = GifMixSrc{frames[f].pix, frames[f].w, frames[f].h, frames[f].stride};
    LaneLease lane(ctx);
    return gif_encode_mixed_core(ctx, lane->stream, src.data(), n, blob, offs, lens);
}
IPX_CATCH_STATUS
