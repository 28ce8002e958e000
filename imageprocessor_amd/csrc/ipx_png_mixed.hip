// ipx_png_mixed.hip -- png.Encode of n RGBA8 frames of ANY sizes in one launch per stage: opacity, filter, deflate, head and tail, pack.
// The uniform encoder (ipx_png.hip) finds frame i by arithmetic (i * frame_stride, i * fbytes, i * region) and takes w and h as kernel
// arguments; here every kernel reads a per-frame table in HBM (PngMixFrame) instead.  The filter's workgroup finds its frame from the
// table's prefix of first rows, the deflate's from its segment; both lookups are uniform over the workgroup.  What is then done to a
// row, a segment or a frame is the code the uniform kernels run (ipx_png_kernels.h, ipx_png_deflate_body.inc), so a frame's stream is byte for byte the one
// png_encode_core writes for it alone, whatever its neighbours are.  DESIGN.md section 4.9.
#include <climits>
#include <vector>

#include "ipx_png.h"
#include "ipx_png_kernels.h"
#include "ipx_runtime_internal.h"

namespace ipx {

// ---- opacity ---------------------------------------------------------------------------------------------------------------------
// blockIdx.y: the frame; the grid's x is sized for the largest frame and a smaller frame's surplus workgroups leave at once
__global__ __launch_bounds__(256) void png_mixed_opacity_kernel(const PngMixFrame *__restrict__ frames, uint32_t *__restrict__ alpha)
{
    const PngMixFrame fr = frames[blockIdx.y];
    const size_t npix = (size_t)fr.w * fr.h;
    const size_t nb = min((size_t)512, (npix + 4095) / 4096);
    if (blockIdx.x >= nb) return;
    int any = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += nb * blockDim.x) {
        const size_t y = i / fr.w, x = i - y * fr.w;
        any |= fr.src[y * fr.stride + 4 * x + 3] != 0xFF;
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(alpha + blockIdx.y, 1u);
}

hipError_t launch_png_mixed_opacity(const PngMixFrame *frames, int n, size_t max_pixels, uint32_t *alpha, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>(512, (max_pixels + 4095) / 4096));
    hipLaunchKernelGGL(png_mixed_opacity_kernel, dim3(blocks, n), dim3(256), 0, s, frames, alpha);
    return hipGetLastError();
}

// ---- un-premultiply and filter ---------------------------------------------------------------------------------------------------
// A workgroup per row over the rows of all frames.  The row's frame is the last one whose first row is not behind it: a binary search
// of the table by a value every lane shares (the workgroup's index), so the probes are scalar loads and the frame's fields stay in
// scalar registers.
constexpr unsigned kMixRowGridX = 1u << 20;

__global__ __launch_bounds__(256) void png_mixed_filter_kernel(const PngMixFrame *__restrict__ frames, int n, unsigned long long rows,
                                                               const uint32_t *__restrict__ alpha, uint8_t *__restrict__ filt)
{
    const unsigned long long r = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;
    if (r >= rows) return;
    const uint32_t row_id = (uint32_t)r;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frames[mid].row0 <= row_id) lo = mid; else hi = mid - 1;
    }
    const PngMixFrame fr = frames[lo];
    const int y = (int)(row_id - fr.row0);
    const int bpp = alpha[lo] ? 4 : 3, rb = fr.w * bpp;
    const uint8_t *row = fr.src + (size_t)y * fr.stride;
    const uint8_t *prev = y > 0 ? row - fr.stride : nullptr;
    png_filter_row(row, prev, rb, bpp, filt + fr.filt + (size_t)y * (rb + 1));
}

hipError_t launch_png_mixed_filter(const PngMixFrame *frames, int n, size_t rows, const uint32_t *alpha, uint8_t *filt, hipStream_t s)
{
    if (n <= 0 || rows == 0) return hipSuccess;
    const unsigned gx = (unsigned)std::min<size_t>(rows, kMixRowGridX), gy = (unsigned)((rows + gx - 1) / gx);
    hipLaunchKernelGGL(png_mixed_filter_kernel, dim3(gx, gy), dim3(256), 0, s, frames, n, (unsigned long long)rows, alpha, filt);
    return hipGetLastError();
}

// ---- deflate of one segment ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDefThreads) void png_mixed_deflate_kernel(const PngMixFrame *__restrict__ frames, const uint8_t *__restrict__ filt,
                                                                        uint32_t *__restrict__ match, const uint32_t *__restrict__ alpha,
                                                                        const PngSeg *__restrict__ segs, uint8_t *__restrict__ out,
                                                                        uint32_t *__restrict__ lens, uint32_t *__restrict__ adler)
{
    __shared__ uint32_t table[kHashSize];   // phase 1: the hash table; phase 2: the walk's window
    __shared__ DefShared S;
    const int t = threadIdx.x;
    const PngSeg sg = segs[blockIdx.x];
    const PngMixFrame fr = frames[sg.frame];
    const int bpp = alpha[sg.frame] ? 4 : 3, stride = 1 + fr.w * bpp;
    const uint32_t N = (uint32_t)fr.h * stride, s0 = sg.s0, s1 = sg.s1, L = s1 - s0;
    const bool first = sg.flags & 1, last = sg.flags & 2;
    const uint8_t *data = filt + fr.filt;
    uint32_t *M = match + fr.filt;
    uint8_t *o = out + sg.out;

#include "ipx_png_deflate_body.inc"
}

hipError_t launch_png_mixed_deflate(const PngMixFrame *frames, const uint8_t *filt, uint32_t *match, const uint32_t *alpha, const PngSeg *segs,
                                    int nseg, uint8_t *out, uint32_t *lens, uint32_t *adler, hipStream_t s)
{
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_mixed_deflate_kernel, dim3(nseg), dim3(kDefThreads), 0, s, frames, filt, match, alpha, segs, out, lens, adler);
    return hipGetLastError();
}

// ---- head and tail ---------------------------------------------------------------------------------------------------------------
// One lane per frame: the signature and the frame's own IHDR (png_write_heads' bytes for its size and colour type), then the tail
__global__ __launch_bounds__(64) void png_mixed_frame_kernel(const PngMixFrame *__restrict__ frames, int n, const uint32_t *__restrict__ alpha,
                                                             const PngSeg *__restrict__ segs, const uint32_t *__restrict__ adler,
                                                             uint8_t *__restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const PngMixFrame fr = frames[f];
    uint8_t *o = out + fr.region;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    for (int i = 0; i < 8; i++) o[i] = sig[i];
    const uint32_t w = (uint32_t)fr.w, h = (uint32_t)fr.h;
    const uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
                              (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h,
                              8, (uint8_t)(alpha[f] ? 6 : 2), 0, 0, 0};   // depth, colour type, deflate, adaptive filtering, no interlace
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < 17; i++) c = c_png_crc.crc[(c ^ ihdr[i]) & 0xFF] ^ (c >> 8);
    c = ~c;
    o[8] = o[9] = o[10] = 0;
    o[11] = 13;
    for (int i = 0; i < 17; i++) o[12 + i] = ihdr[i];
    o[29] = (uint8_t)(c >> 24);
    o[30] = (uint8_t)(c >> 16);
    o[31] = (uint8_t)(c >> 8);
    o[32] = (uint8_t)c;
    png_frame_tail(segs, adler, fr.seg0, fr.seg1, o + fr.tail);
}

hipError_t launch_png_mixed_frame(const PngMixFrame *frames, int n, const uint32_t *alpha, const PngSeg *segs, const uint32_t *adler,
                                  uint8_t *out, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_mixed_frame_kernel, dim3((n + 63) / 64), dim3(64), 0, s, frames, n, alpha, segs, adler, out);
    return hipGetLastError();
}

}  // namespace ipx

// ---- the core and the entry ------------------------------------------------------------------------------------------------------

// n frames of any sizes in HBM -> streams in one pinned block (ipx_host_alloc), everything on stream s; returns once the block is
// filled.  The host waits twice before the download, as png_encode_core does: for the opacity words (the colour type decides a frame's
// segments) and for the segments' lengths (they decide where the pieces go).
int ipx::png_encode_mixed_core(ipx_ctx *ctx, hipStream_t s, const ipx_rgba_frame *frames, int n, uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    std::vector<PngMixFrame> tab(n);
    std::vector<uint32_t> alpha(n), sl;
    std::vector<PngSeg> segs;
    std::vector<PngPiece> pieces;
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    size_t max_pixels = 0;
    for (int f = 0; f < n; f++) {
        memset(&tab[f], 0, sizeof tab[f]);
        tab[f].src = frames[f].pix;
        tab[f].w = frames[f].w;
        tab[f].h = frames[f].h;
        tab[f].stride = frames[f].stride;
        max_pixels = std::max(max_pixels, (size_t)frames[f].w * frames[f].h);
    }
    PngMixFrame *dtab;
    uint32_t *dalpha;
    IPX_HIP(mem.get(&dtab, (size_t)n * sizeof(PngMixFrame)));
    IPX_HIP(mem.get(&dalpha, (size_t)n * 4));
    IPX_HIP(hipMemsetAsync(dalpha, 0, (size_t)n * 4, s));
    IPX_HIP(hipMemcpyAsync(dtab, tab.data(), (size_t)n * sizeof(PngMixFrame), hipMemcpyHostToDevice, s));
    IPX_HIP(launch_png_mixed_opacity(dtab, n, max_pixels, dalpha, s));
    IPX_HIP(hipMemcpyAsync(alpha.data(), dalpha, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // every frame's place in the scratch and its segments, by its own size and colour type
    size_t rows = 0, fbytes = 0, obytes = 0;
    for (int f = 0; f < n; f++) {
        const int w = tab[f].w, h = tab[f].h, bpp = alpha[f] ? 4 : 3;
        const size_t tail = kPngSegBase + png_segs_bytes(w, h, bpp);
        tab[f].row0 = (uint32_t)rows;
        tab[f].filt = fbytes;
        tab[f].region = obytes;
        tab[f].tail = (uint32_t)tail;
        tab[f].seg0 = (uint32_t)segs.size();
        png_append_segs(&segs, (uint32_t)f, w, h, bpp, obytes);
        tab[f].seg1 = (uint32_t)segs.size();
        rows += (size_t)h;
        fbytes += align256((size_t)h * PngSegs(w, h, bpp).stride);
        obytes += align256(tail + kPngTailBytes);
    }
    if (segs.size() > (size_t)INT_MAX) { set_error("png: too many segments in one call"); return IPX_ERR_UNSUPPORTED; }
    const int nseg = (int)segs.size();
    uint8_t *dfilt, *dout;
    uint32_t *dmatch, *dlens, *dadler;
    PngSeg *dsegs;
    IPX_HIP(mem.get(&dfilt, fbytes));
    IPX_HIP(mem.get(&dmatch, fbytes * 4));
    IPX_HIP(mem.get(&dout, obytes));
    IPX_HIP(mem.get(&dlens, (size_t)nseg * 4));
    IPX_HIP(mem.get(&dadler, (size_t)nseg * 8));
    IPX_HIP(mem.get(&dsegs, (size_t)nseg * sizeof(PngSeg)));
    IPX_HIP(hipMemcpyAsync(dtab, tab.data(), (size_t)n * sizeof(PngMixFrame), hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(dsegs, segs.data(), (size_t)nseg * sizeof(PngSeg), hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemsetAsync(dout, 0, obytes, s));
    IPX_HIP(launch_png_mixed_filter(dtab, n, rows, dalpha, dfilt, s));
    IPX_HIP(launch_png_mixed_deflate(dtab, dfilt, dmatch, dalpha, dsegs, nseg, dout, dlens, dadler, s));
    IPX_HIP(launch_png_mixed_frame(dtab, n, dalpha, dsegs, dadler, dout, s));
    sl.resize(nseg);
    IPX_HIP(hipMemcpyAsync(sl.data(), dlens, (size_t)nseg * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // the pieces: head, the segments' chunks, tail, frame after frame, each stream starting 16-byte aligned
    pieces.reserve(nseg + 2 * (size_t)n);
    size_t total = 0;
    for (int f = 0; f < n; f++) {
        offs[f] = total;
        if (!(lens[f] = png_place_pieces(&pieces, segs, sl, tab[f].seg0, tab[f].seg1, tab[f].region, tab[f].tail, &total))) return IPX_ERR_INVALID;
    }
    if (pieces.size() > (size_t)INT_MAX) { set_error("png: too many pieces in one call"); return IPX_ERR_UNSUPPORTED; }
    uint8_t *dpack;
    PngPiece *dpieces;
    IPX_HIP(mem.get(&dpack, total));
    IPX_HIP(mem.get(&dpieces, pieces.size() * sizeof(PngPiece)));
    IPX_HIP(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(PngPiece), hipMemcpyHostToDevice, s));
    IPX_HIP(launch_png_pack(dout, dpieces, (int)pieces.size(), dpack, s));
    return download_streams(ctx, s, dpack, total, "png ", blob);
}

extern "C" {

int ipx_png_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, uint8_t **blob, size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    const auto aligned = [](const char *who, int f, const ipx_rgba_frame &fr) -> int {
        if (!(((uintptr_t)fr.pix | (unsigned)fr.stride) & 3)) return IPX_OK;
        set_error("%s: frame %d: the address and the stride must be multiples of 4", who, f);
        return IPX_ERR_INVALID;
    };
    const int rc = rgba_frames_check("ipx_png_encode_mixed_dev", frames, n, blob, offs, lens, aligned, false);
    if (rc || n == 0) return rc;
    LaneLease lane(ctx);
    return png_encode_mixed_core(ctx, lane->stream, frames, n, blob, offs, lens);
}
IPX_CATCH_STATUS

}  // extern "C"
