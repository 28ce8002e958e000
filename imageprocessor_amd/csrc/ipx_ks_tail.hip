// ipx_ks_tail.hip -- what runs behind the one-pass kernel's float pass and its float64 redo pass (ipx_ks_fused.hip), as ONE launch: the
// exact pass over the resize output's list, the exact pass over the thumbnail's, and the text of the watermark frames.  As three
// launches (ks_fix_kernel twice, composite_kernel) they ran strictly one after the other although they write disjoint bytes.
//
// Block-uniform dispatch on the block index, frame by frame: a frame's exact blocks of output 0, of output 1, then its text blocks, so
// that all three kinds of work are resident at the same time (all exact blocks in front of all text blocks ran them one after the
// other: a batch has several times more blocks than the chip holds).  A block works on one output (its tap kind is a template
// argument, R and the tables are block-uniform).  The arithmetic is ks_exact_list's (ipx_ks_exact.h) and glyph_walk's
// (ipx_device.h), shared with ks_fix_kernel and composite_kernel; what differs from those launches:
//   * exact part: R = 4 lanes per pixel where the vertical range has at most 4 rows (with R = 8 half of every group idles on a
//     1080 -> 768 resize), the taps of the dword kinds in 16-byte pieces (KsGenArgs::src_w), the chain of a pass prefetched;
//   * text part: composite_kernel's layout (a lane takes one column of four rows, a block 64 x 16 pixels).  Four adjacent pixels per
//     lane as one 16-byte access was built and measured slower.  Pixels no glyph touches are never written.
#include <algorithm>
#include <cstdlib>

#include "ipx_ks_exact.h"

namespace ipx {
namespace {

constexpr int kTailThreads = 256;
constexpr int kTextRows = 4;        // pixels per lane: one column, 4 rows apart (a block covers 64 x 16 pixels, as composite_kernel's does)

template <int KIND>
__device__ __forceinline__ void tail_exact(KsGenArgs a, const uint2 *list, size_t list_stride, const int *count, int count_stride, int cap, int R,
                                           int frame, int chunk, int chunks)
{
    const int n = min(count[(size_t)frame * count_stride], cap);
    list += (size_t)frame * list_stride;
    a.dst += frame * a.dst_fs;
    a.src += frame * a.src_fs;
    if (KIND == IPX_SRC_YCBCR || KIND == IPX_SRC_YCBCR_CROP) { a.cb += frame * a.c_fs; a.cr += frame * a.c_fs; }
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int per_wave = 64 / R, sub = lane / R, sl = lane - sub * R, per_block = (kTailThreads >> 6) * per_wave;
    ks_exact_list<KIND>(a, list, n, chunk * per_block, chunks * per_block, wv * per_wave + sub, R, sub, sl);
}

__device__ __forceinline__ void tail_text(const KsTailArgs &t, DevGlyph *tab, int f, int rb)
{
    const int by = rb / t.tbx, bx = rb - by * t.tbx;
    const Rect bbox = t.text.bbox;
    const int n = t.text.n;
    const int x = bbox.x0 + bx * 64 + ((int)threadIdx.x & 63);
    const int ybase = bbox.y0 + by * (4 * kTextRows) + ((int)threadIdx.x >> 6);
    uint8_t *frame = t.wm + (size_t)f * t.wm_fs;
    // the pixels first (their loads fly while the table arrives)
    uint32_t d[kTextRows][1], d0[kTextRows];
#pragma unroll
    for (int r = 0; r < kTextRows; r++) {
        const int y = ybase + 4 * r;
        d0[r] = d[r][0] = x < bbox.x1 && y < bbox.y1 ? *(const uint32_t *)(frame + (size_t)y * t.wm_stride + (size_t)x * 4) : 0u;
    }
    for (int g = (int)threadIdx.x; g < n; g += kTailThreads) tab[g] = t.text.gl[g];
    __syncthreads();
    glyph_walk<1, kTextRows, 4>(tab, n, x, ybase, bbox, d, t.text.sr, t.text.sg, t.text.sb, t.text.sa);
#pragma unroll
    for (int r = 0; r < kTextRows; r++) {
        const int y = ybase + 4 * r;
        if (x < bbox.x1 && y < bbox.y1 && d[r][0] != d0[r]) *(uint32_t *)(frame + (size_t)y * t.wm_stride + (size_t)x * 4) = d[r][0];
    }
}

// K0 / K1: the tap kinds of the two exact parts (K1 is K0 or its `_CROP` kind)
template <int K0, int K1>
__global__ __launch_bounds__(kTailThreads) void ks_tail_kernel(KsTailArgs t)
{
    __shared__ DevGlyph tab[kMaxGlyphs];                                  // only the text blocks load it
    // frame by frame: the exact blocks of output 0, of output 1, the text blocks -- so that all three kinds are resident together
    const int nx = t.chunks[0] + t.chunks[1], per = nx + t.tbx * t.tby, b = (int)blockIdx.x;
    const int frame = b / per, c = b - frame * per;
    if (c < nx) {
        const int k = c >= t.chunks[0] ? 1 : 0, chunk = c - (k ? t.chunks[0] : 0);
        if (K0 == K1 || k == 0)
            tail_exact<K0>(k ? t.g[1] : t.g[0], t.list[k], t.list_stride, t.count[k], t.count_stride, t.cap[k], t.R[k], frame, chunk, t.chunks[k]);
        else
            tail_exact<K1>(t.g[1], t.list[1], t.list_stride, t.count[1], t.count_stride, t.cap[1], t.R[1], frame, chunk, t.chunks[1]);
        return;
    }
    tail_text(t, tab, frame, c - nx);
}

template <int K0, int K1>
void tail_go(const KsTailArgs &t, unsigned blocks, hipStream_t s)
{
    hipLaunchKernelGGL((ks_tail_kernel<K0, K1>), dim3(blocks), dim3(kTailThreads), 0, s, t);
}

// the pairs that occur: a source kind with itself (no crop, or one output), with its `_CROP` kind, and the `_CROP` kind alone
template <int S, int C>
bool tail_pair(int k0, int k1, const KsTailArgs &t, unsigned blocks, hipStream_t s)
{
    if (k0 == S && k1 == S) tail_go<S, S>(t, blocks, s);
    else if (k0 == S && k1 == C) tail_go<S, C>(t, blocks, s);
    else if (k0 == C && k1 == C) tail_go<C, C>(t, blocks, s);
    else return false;
    return true;
}

}  // namespace

hipError_t launch_ks_tail(KsTailArgs t, hipStream_t s)
{
    if (t.nframes <= 0) return hipSuccess;
    // Blocks per frame and output: about two thousand per output, i.e. two per frame for a batch of 1024 (a photograph leaves a few
    // hundred pixels of an output on its frame's list; a block takes 64 (R = 4) to 4 (R = 64) per pass), more per frame when the batch
    // is small.  Measured per 1024 x 1080p with the exact part launched alone: 8192 blocks 129 us, 2048 126, 1024 117; inside the
    // whole tail 2048 was the fastest.  IPX_KS_TAIL_BLOCKS: test knob, that budget.
    const char *ev = getenv("IPX_KS_TAIL_BLOCKS");
    const int budget = ev && atoi(ev) > 0 ? atoi(ev) : 2048;
    for (int k = 0; k < 2; k++) {
        t.R[k] = 8; t.chunks[k] = 0;
        if (!t.list[k] || t.cap[k] <= 0) { t.cap[k] = 0; continue; }
        const int ntap = t.g[k].ay.ntap;
        t.R[k] = ntap <= 4 ? 4 : ntap <= 8 ? 8 : ntap <= 16 ? 16 : 64;
        const int per_block = (kTailThreads / 64) * (64 / t.R[k]), most = (t.cap[k] + per_block - 1) / per_block;
        t.chunks[k] = std::max(1, std::min(most, std::max(1, budget / t.nframes)));
    }
    const bool text = t.wm && t.text.gl && t.text.n > 0 && !t.text.bbox.empty();
    if (!text) t.text.n = 0;
    t.tbx = text ? (t.text.bbox.dx() + 63) / 64 : 0;
    t.tby = text ? (t.text.bbox.dy() + 4 * kTextRows - 1) / (4 * kTextRows) : 0;
    const long long blocks = (long long)t.nframes * (t.chunks[0] + t.chunks[1]) + (long long)t.nframes * t.tbx * t.tby;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    // one output: both slots name its kind (slot 1 has no blocks)
    const int k0 = t.chunks[0] ? t.g[0].kind : t.g[1].kind, k1 = t.chunks[1] ? t.g[1].kind : k0;
    const bool none = !t.chunks[0] && !t.chunks[1];                       // text alone: any instantiation does
    if (none) { tail_go<IPX_SRC_RGBA, IPX_SRC_RGBA>(t, (unsigned)blocks, s); return hipGetLastError(); }
    if (!tail_pair<IPX_SRC_RGBA, IPX_SRC_RGBA_CROP>(k0, k1, t, (unsigned)blocks, s) && !tail_pair<IPX_SRC_NRGBA, IPX_SRC_NRGBA_CROP>(k0, k1, t, (unsigned)blocks, s) &&
        !tail_pair<IPX_SRC_YCBCR, IPX_SRC_YCBCR_CROP>(k0, k1, t, (unsigned)blocks, s) && !tail_pair<IPX_SRC_TAP64, IPX_SRC_TAP64_CROP>(k0, k1, t, (unsigned)blocks, s))
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ipx
