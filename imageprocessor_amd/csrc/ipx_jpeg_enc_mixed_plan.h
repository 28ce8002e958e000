// ipx_jpeg_enc_mixed_plan.h -- the per-frame records of a mixed-size jpeg.Encode (jpeg_encode_mixed_core, ipx_jpeg_runtime.hip): frames of
// any sizes go through one launch per stage; what the uniform kernels take as launch arguments (w, h, stride, aligned16, nblk,
// max_chunks, blockIdx.y * nblk) a mixed kernel reads from its frame's record.  The records are built in three steps, one before each of
// the encoder's waits for the device: the geometry (jpeg_enc_build), the unstuffed streams once the scans' bit counts are back
// (jpeg_enc_place_scans), the finished streams once the 0xff counts are back (jpeg_enc_place_streams).  Plain C++ with no dependency
// on the runtime, shared by the kernels, the driver and tools/jpeg_enc_mixed_plan_test.cpp, which holds the builder, the search and the
// scan-length rule (jpeg_scan_limit: the uniform core's too) to their rules as a program of its own.  DESIGN.md section 4.6.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ipx_align.h"

#if defined(__HIPCC__)
#define IPX_ENC_HD __host__ __device__
#else
#define IPX_ENC_HD
#endif

namespace ipx {

constexpr int kJpegEncMcuPerWg = 8;        // MCUs of one MCU row that a transform workgroup takes (ipx_jpeg.hip)
constexpr int kJpegEncBlkPerWg = 256;      // blocks a sizing or packing workgroup takes, chunks a stuffing workgroup takes
constexpr int kJpegEncChunk = 64;          // unstuffed bytes per chunk of the stuffing passes (ipx_jpeg_entropy.hip: kChunk)
// jpeg_write_header: SOI (2), DQT (2 + 2 + 2 * 65), the SOF0 marker, length and precision (2 + 2 + 1), then height and width, two
// big-endian bytes each -- the only bytes of the header that depend on the frame
constexpr int kJpegSofDims = 2 + 2 + 2 + 2 * 65 + 2 + 2 + 1;

// what the caller says of a frame: RGBA8 in HBM, and where its quantised coefficients go (mcus * 384 int16, 16-byte aligned)
struct JpegEncSrc { const uint8_t *src; int16_t *coefs; int32_t w, h, stride; };

// one frame, in HBM
struct JpegEncFrame {
    const uint8_t *src;
    int16_t *coefs;
    unsigned long long mcu_base;     // its first MCU in the dense block-length and DC arrays, six entries per MCU (replaces blockIdx.y * nblk)
    unsigned long long ff0;          // its first chunk in the 0xff-count array (replaces f * max_chunks)
    unsigned long long ubase, obase; // its unstuffed scan in the scratch, its finished stream in the output block
    int32_t w, h, stride;
    int32_t aligned16;               // base and row stride are multiples of 16
    int32_t mw, mcus;                // MCUs per row and per frame; the frame has mcus * 6 blocks
    int32_t wgs_per_row;             // transform workgroups per MCU row
    uint32_t wg_fdct, wg_blk, wg_chunk;   // its first workgroup in the transform's grid, the block grids' and the chunk grids'
    uint32_t nchunks, ubytes;        // of the unstuffed scan
};
static_assert(sizeof(JpegEncFrame) == 96, "read as scalars, one record per frame");

struct JpegEncTotals {
    unsigned long long mcus = 0;                              // the block-length and DC arrays hold mcus * 6 entries
    unsigned long long fdct_wgs = 0, blk_wgs = 0;             // the grids of the transform, and of the sizing and packing kernels
    unsigned long long chunks = 0, chunk_wgs = 0, ubytes = 0; // jpeg_enc_place_scans: the 0xff-count array, the stuffing grids, the scratch
};

// The records of n frames, in the order given: the geometry and the first workgroups of the grids that do not depend on the scans'
// lengths.  Every prefix sum is kept in 64 bits; false when the frames cannot be one launch set: a side below 1 or beyond 65535, a
// stride below 4 * w, or more workgroups than a grid's x dimension holds (2^31 - 1).
inline bool jpeg_enc_build(const JpegEncSrc *in, int n, std::vector<JpegEncFrame> *out, JpegEncTotals *tot)
{
    out->assign((size_t)(n > 0 ? n : 0), JpegEncFrame{});
    *tot = JpegEncTotals{};
    for (int i = 0; i < n; i++) {
        const JpegEncSrc &f = in[i];
        if (f.w < 1 || f.h < 1 || f.w > 65535 || f.h > 65535 || (long long)f.stride < (long long)f.w * 4) return false;
        if (tot->fdct_wgs > 0x7fffffffull || tot->blk_wgs > 0x7fffffffull) return false;
        JpegEncFrame &g = (*out)[(size_t)i];
        g.src = f.src; g.coefs = f.coefs;
        g.w = f.w; g.h = f.h; g.stride = f.stride;
        g.aligned16 = ((((uintptr_t)f.src) | (uintptr_t)(uint32_t)f.stride) & 15) == 0;
        const int mh = (f.h + 15) >> 4;
        g.mw = (f.w + 15) >> 4;
        g.mcus = g.mw * mh;                                   // at most 4096 * 4096
        g.wgs_per_row = (g.mw + kJpegEncMcuPerWg - 1) / kJpegEncMcuPerWg;
        g.mcu_base = tot->mcus;
        g.wg_fdct = (uint32_t)tot->fdct_wgs;
        g.wg_blk = (uint32_t)tot->blk_wgs;
        tot->mcus += (unsigned long long)g.mcus;
        tot->fdct_wgs += (unsigned long long)g.wgs_per_row * (unsigned long long)mh;
        tot->blk_wgs += ((unsigned long long)g.mcus * 6 + kJpegEncBlkPerWg - 1) / kJpegEncBlkPerWg;
    }
    return tot->fdct_wgs <= 0x7fffffffull && tot->blk_wgs <= 0x7fffffffull;
}

// The scan-length rule of both encode cores.  The block offsets (the block lengths after the scan) and a frame's unstuffed bytes are
// 32-bit: a frame whose scan reaches 2^32 - 1 bits (some 200 M pixels of binary noise at quality 100) would wrap them, and the bit
// packer would then write beyond the unstuffed scratch.  The cores refuse such a call once the sizes are back, before anything reads
// the offsets or is sized from them.  knob: IPX_JPEG_MAX_SCAN_BITS, which can only lower the limit (for the tests); 0 or less: unset.
constexpr unsigned long long kJpegScanBitsTop = 0xffffffffull;
inline unsigned long long jpeg_scan_limit(int knob)
{
    return knob > 0 && (unsigned long long)knob < kJpegScanBitsTop ? (unsigned long long)knob : kJpegScanBitsTop;
}
// the first of n scans that is at the limit or beyond it, or -1
inline long long jpeg_scan_too_long(const unsigned long long *bits, size_t n, unsigned long long limit)
{
    for (size_t j = 0; j < n; j++)
        if (bits[j] >= limit) return (long long)j;
    return -1;
}

// Once every frame's scan length is known (bits[i] < 2^32 - 1, the caller's refusal): its unstuffed bytes, their place in the scratch
// (256-byte aligned, eight bytes of slack for the bit packer's last word), its chunks and its first workgroup in the chunk grids.  A
// frame has at least one chunk workgroup -- the one that writes its header -- so first workgroups are strictly increasing.
inline bool jpeg_enc_place_scans(const unsigned long long *bits, int n, std::vector<JpegEncFrame> *recs, JpegEncTotals *tot)
{
    tot->chunks = tot->chunk_wgs = tot->ubytes = 0;
    for (int i = 0; i < n; i++) {
        JpegEncFrame &g = (*recs)[(size_t)i];
        if (bits[i] >= kJpegScanBitsTop || tot->chunk_wgs > 0x7fffffffull) return false;
        g.ubytes = (uint32_t)((bits[i] + 7) / 8);
        g.nchunks = (g.ubytes + kJpegEncChunk - 1) / kJpegEncChunk;
        g.ubase = tot->ubytes;
        g.ff0 = tot->chunks;
        g.wg_chunk = (uint32_t)tot->chunk_wgs;
        const unsigned long long wgs = ((unsigned long long)g.nchunks + kJpegEncBlkPerWg - 1) / kJpegEncBlkPerWg;
        tot->ubytes += align256((size_t)g.ubytes + 8);
        tot->chunks += g.nchunks;
        tot->chunk_wgs += wgs ? wgs : 1;
    }
    return tot->chunk_wgs <= 0x7fffffffull;
}

// Once every frame's 0xff count is known: its stream's length (header, stuffed scan, EOI) and its place in the block, every stream
// starting 16-byte aligned as jpeg_encode_sets lays them.  -> the block's bytes.
inline unsigned long long jpeg_enc_place_streams(const uint32_t *ff, int n, size_t hdr_len, std::vector<JpegEncFrame> *recs, size_t *offs, size_t *lens)
{
    unsigned long long total = 0;
    for (int i = 0; i < n; i++) {
        JpegEncFrame &g = (*recs)[(size_t)i];
        lens[i] = hdr_len + g.ubytes + ff[i] + 2;
        g.obase = total;
        offs[i] = (size_t)total;
        total += align16(lens[i]);
    }
    return total;
}

// The frame that owns workgroup wg of one of the one-dimensional grids: the last one whose first workgroup in that grid (`first`:
// wg_fdct, wg_blk or wg_chunk) is not behind it -- jpeg_mix_find's rule and form (ipx_jpeg_mixed_plan.h).  Every frame has at least one
// workgroup in each grid, so first workgroups are strictly increasing.  The kernels call this with a value every lane shares: the
// probes are scalar loads.  wg must be below the grid's total.
IPX_ENC_HD inline int jpeg_enc_find(const JpegEncFrame *g, int n, uint32_t wg, uint32_t JpegEncFrame::*first)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g[mid].*first <= wg) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace ipx
