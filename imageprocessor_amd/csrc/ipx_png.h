// ipx_png.h -- png.Encode(w, *image.RGBA) on the GPU: what the kernels (ipx_png.hip) and the host half (ipx_png_host.cpp) share.
// Not part of the ABI.  Go's visible decisions (colour type, un-premultiply, filter per row) are kept exactly; the zlib stream is this
// project's own and is held byte for byte to tests/png_model.py, which defines the same constants.  DESIGN.md section 4.9.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ipx_internal.h"

namespace ipx {

constexpr int kPngSegMin = 65536;      // a segment: whole rows, at least this many filtered bytes (the frame's last takes the remainder)
constexpr int kPngTile = 256;          // the hashed candidate of i lies before the start of i's tile (tiles counted from segment start)
constexpr int kPngHashBits = 15;       // hash(j) = (u32le(data + j) * kPngHashMul) >> (32 - kPngHashBits), for j + 4 <= frame bytes
constexpr uint32_t kPngHashMul = 0x9E3779B1u;
constexpr int kPngWindow = 32768;
constexpr int kPngMaxMatch = 258;
constexpr int kPngMinMatch = 3;
constexpr int kPngHeadBytes = 8 + 25;  // signature + IHDR
constexpr int kPngTailBytes = 16 + 12; // the Adler-32 IDAT chunk + IEND

// the segments of a w x h frame of bpp 3 or 4: rows_per_seg rows each, nseg of them, the last one taking the remaining rows
struct PngSegs {
    int stride, rps, nseg;   // stride: filtered row bytes, 1 + w * bpp
    PngSegs(int w, int h, int bpp)
    {
        stride = 1 + w * bpp;
        rps = (kPngSegMin + stride - 1) / stride;
        if (rps < 1) rps = 1;
        nseg = h / rps;
        if (nseg < 1) nseg = 1;
    }
    int row0(int s, int h) const { return s == nseg ? h : s * rps; }
};

// chunk data bytes of a segment of `len` filtered bytes sent as stored blocks (<= 65535 bytes each) and the empty stored block
__host__ __device__ inline size_t png_stored_bytes(size_t len, bool first) { return (first ? 2 : 0) + 5 * ((len + 65534) / 65535) + len + 5; }

// where the pieces of a frame's stream sit in its region of the output: the head at 0, the segments' chunks from kPngSegBase (each in
// a slot of its stored bound, 4-byte aligned), the tail behind them
constexpr size_t kPngSegBase = 36;
inline size_t png_slot_bytes(size_t len, bool first) { return (12 + png_stored_bytes(len, first) + 3) & ~(size_t)3; }
inline size_t png_segs_bytes(int w, int h, int bpp)
{
    const PngSegs g(w, h, bpp);
    size_t b = 0;
    for (int s = 0; s < g.nseg; s++) b += png_slot_bytes((size_t)(g.row0(s + 1, h) - g.row0(s, h)) * g.stride, s == 0);
    return b;
}

// one segment to compress (a workgroup of png_deflate_kernel): frame, byte range [s0, s1) of the frame's filtered stream, where its
// IDAT chunk goes in the output regions (4-byte aligned) and whether it is the frame's first / last
struct PngSeg {
    uint32_t frame, s0, s1, flags;   // flags: 1 first, 2 last
    unsigned long long out;
};
// a copy of the pack kernel: len bytes from the regions to the packed block
struct PngPiece {
    unsigned long long src, dst;
    uint32_t len, pad;
};

// ---- the host arithmetic of both encode cores (png_encode_core, png_encode_mixed_core) ----
// Appends the segments of frame `frame`, w x h of bpp 3 or 4 (its colour type), whose region of the output scratch starts at `region`:
// each segment's IDAT chunk gets the slot of its stored bound, from kPngSegBase on.
inline void png_append_segs(std::vector<PngSeg> *segs, uint32_t frame, int w, int h, int bpp, size_t region)
{
    const PngSegs g(w, h, bpp);
    size_t at = region + kPngSegBase;
    for (int k = 0; k < g.nseg; k++) {
        PngSeg sg;
        sg.frame = frame;
        sg.s0 = (uint32_t)((size_t)g.row0(k, h) * g.stride);
        sg.s1 = (uint32_t)((size_t)g.row0(k + 1, h) * g.stride);
        sg.flags = (k == 0 ? 1u : 0u) | (k == g.nseg - 1 ? 2u : 0u);
        sg.out = at;
        at += png_slot_bytes(sg.s1 - sg.s0, k == 0);
        segs->push_back(sg);
    }
}
// Appends the pieces of one frame's stream, which starts at *total of the packed block: the head at `region`, the chunks of its
// segments [seg0, seg1) at the lengths the deflate reported (sl), the tail at region + tail.  -> the stream's length, with *total moved
// to where the next stream starts (16-byte aligned); 0, with the error text set, when a segment overran its slot.
inline size_t png_place_pieces(std::vector<PngPiece> *pieces, const std::vector<PngSeg> &segs, const std::vector<uint32_t> &sl, uint32_t seg0,
                               uint32_t seg1, size_t region, size_t tail, size_t *total)
{
    size_t at = *total;
    pieces->push_back({region, at, (uint32_t)kPngHeadBytes, 0});
    at += kPngHeadBytes;
    for (uint32_t k = seg0; k < seg1; k++) {
        if (sl[k] > png_slot_bytes(segs[k].s1 - segs[k].s0, k == seg0)) { set_error("png: segment %u overran its bound", k); return 0; }
        pieces->push_back({segs[k].out, at, sl[k], 0});
        at += sl[k];
    }
    pieces->push_back({region + tail, at, (uint32_t)kPngTailBytes, 0});
    at += kPngTailBytes;
    const size_t len = at - *total;
    *total = align16(at);
    return len;
}

// ---- CRC-32 of chunks and the Paeth predictor: shared by the encoder (ipx_png.hip) and the decoder (ipx_png_dec.hip) ----------------
// crc: the byte table of the reflected polynomial 0xEDB88320; x2n[k]: x^(2^k) mod P (zlib's x2n_table).  Each translation unit that
// uses them keeps its own copy in constant memory.
struct PngCrcTables {
    uint32_t crc[256];
    uint32_t x2n[32];
    constexpr PngCrcTables() : crc{}, x2n{}
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            crc[i] = c;
        }
        uint32_t p = 1u << 30;   // x^1
        for (int k = 0; k < 32; k++) {
            x2n[k] = p;
            p = mult(p, p);
        }
    }
    static constexpr uint32_t mult(uint32_t a, uint32_t b)
    {
        uint32_t m = 1u << 31, p = 0;
        for (;;) {
            if (a & m) {
                p ^= b;
                if ((a & (m - 1)) == 0) break;
            }
            m >>= 1;
            b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1;
        }
        return p;
    }
};

__device__ inline uint32_t crc_mult(uint32_t a, uint32_t b)   // a * b mod P (reflected)
{
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) {
        if (a & (1u << k)) p ^= b;
        b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// the raw CRC state c after nbytes zero bytes (x2n: PngCrcTables::x2n in constant memory)
__device__ inline uint32_t crc_shift(uint32_t c, uint32_t nbytes, const uint32_t *x2n)
{
    uint32_t p = 1u << 31;
    for (int k = 3; nbytes; nbytes >>= 1, k++)
        if (nbytes & 1) p = crc_mult(x2n[k & 31], p);
    return crc_mult(p, c);
}

__device__ inline int paeth(int a, int b, int c)
{
    int pa = b - c, pb = a - c;
    const int pc = abs(pa + pb);
    pa = abs(pa);
    pb = abs(pb);
    if (pa <= pb && pa <= pc) return a;
    return pb <= pc ? b : c;
}

// signature + IHDR for colour type 2 (bpp 3) and 6 (bpp 4) of a w x h frame: out[0] and out[1]
void png_write_heads(int w, int h, uint8_t out[2][kPngHeadBytes]);

// ---- kernel launchers (ipx_png.hip) ----
// alpha[i] |= 1 when frame i has an alpha byte other than 0xff (alpha: n zeroed words)
hipError_t launch_png_opacity(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint32_t *alpha, hipStream_t s);
// frame i's filtered stream (h rows of 1 + w * bpp bytes, bpp = alpha[i] ? 4 : 3) at filt + i * fbytes
hipError_t launch_png_filter(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, const uint32_t *alpha,
                             uint8_t *filt, size_t fbytes, hipStream_t s);
// one workgroup per segment: match candidates (scratch: match, 4 bytes per filtered byte), the greedy parse, the block and its IDAT
// chunk at out + seg.out (zeroed beforehand); lens[k]: the chunk's bytes; adler[2k], adler[2k + 1]: the segment's Adler sums
hipError_t launch_png_deflate(const uint8_t *filt, uint32_t *match, size_t fbytes, int w, int h, const uint32_t *alpha, const PngSeg *segs,
                              int nseg, uint8_t *out, uint32_t *lens, uint32_t *adler, hipStream_t s);
// per frame: signature + IHDR (heads: the two variants) at out + i * region, the Adler-32 chunk and IEND at out + i * region + tail;
// item0[i] .. item0[i + 1]: frame i's segments
hipError_t launch_png_frame(const uint8_t *heads, const uint32_t *alpha, const uint32_t *item0, const PngSeg *segs, const uint32_t *adler,
                            int n, uint8_t *out, size_t region, size_t tail, hipStream_t s);
hipError_t launch_png_pack(const uint8_t *out, const PngPiece *pieces, int npieces, uint8_t *dst, hipStream_t s);

// ---- frames of any sizes in one launch per stage (ipx_png_mixed.hip) ----
// One frame of a mixed-size encode, in HBM: where its pixels are and where its pieces go.  The host fills src, w, h, stride before the
// opacity launch and the rest once the colour types are known.
struct PngMixFrame {
    const uint8_t *src;          // RGBA8 rows, `stride` bytes apart
    int32_t w, h, stride;
    uint32_t row0;               // the frame's first row among the rows of all frames (the filter's workgroups)
    uint32_t seg0, seg1;         // its segments in the segment table
    uint32_t tail;               // its region: the head at 0, the tail here
    unsigned long long filt;     // its filtered stream in the filter scratch (bytes); its match scratch is the same number of words in
    unsigned long long region;   // its region in the output scratch (bytes, 256-byte aligned)
};
// alpha[i] |= 1 when frame i has an alpha byte other than 0xff (alpha: n zeroed words); only src, w, h, stride of the table are read
hipError_t launch_png_mixed_opacity(const PngMixFrame *frames, int n, size_t max_pixels, uint32_t *alpha, hipStream_t s);
// a workgroup per row of every frame (rows: their sum): frame i's filtered stream at filt + frames[i].filt
hipError_t launch_png_mixed_filter(const PngMixFrame *frames, int n, size_t rows, const uint32_t *alpha, uint8_t *filt, hipStream_t s);
// a workgroup per segment, as launch_png_deflate; seg.frame indexes the table
hipError_t launch_png_mixed_deflate(const PngMixFrame *frames, const uint8_t *filt, uint32_t *match, const uint32_t *alpha, const PngSeg *segs,
                                    int nseg, uint8_t *out, uint32_t *lens, uint32_t *adler, hipStream_t s);
// per frame: signature and the frame's own IHDR at its region, the Adler-32 chunk and IEND at its tail
hipError_t launch_png_mixed_frame(const PngMixFrame *frames, int n, const uint32_t *alpha, const PngSeg *segs, const uint32_t *adler,
                                  uint8_t *out, hipStream_t s);

}  // namespace ipx

struct ipx_ctx;
namespace ipx {
// png.Encode of n RGBA8 frames in HBM -> streams in one pinned block (ipx_host_alloc), everything on stream s; returns once the block
// is filled (ipx_png.hip; the chunk step of ipx_out_stage.hip calls it for every PNG leg)
int png_encode_core(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                    uint8_t **blob, size_t *offs, size_t *lens);
// the same for n frames of any sizes, one launch per stage (ipx_png_mixed.hip; the mixed PNG leg of ipx_png_legs.hip).  The frames are
// taken as checked (ipx_png_encode_mixed_dev checks them).
int png_encode_mixed_core(ipx_ctx *ctx, hipStream_t s, const ipx_rgba_frame *frames, int n, uint8_t **blob, size_t *offs, size_t *lens);

}  // namespace ipx
