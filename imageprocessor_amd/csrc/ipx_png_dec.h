// ipx_png_dec.h -- png.Decode (non-interlaced files, and Adam7 ones under IPX_PNG_ADAM7=1) on the GPU: what the kernels
// (ipx_png_dec.hip), the driver (ipx_png_dec_runtime.hip), the legs (ipx_png_legs.hip) and the host half (ipx_png_dec_host.cpp) share.
// Not part of the ABI.  The restatement of Go's reader is in DESIGN.md section 4.10; tests/png_decode_model.py is the model it is held to.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ipx_internal.h"
#include "ipx_png_layout.h"

namespace ipx {

// the frame layouts (IPX_PNG_* of include/ipx.h) and their bytes per pixel
constexpr int kPngKinds = 7;
inline int png_kind_bpp(int kind) { return src_bpp(src_of_png(kind)); }

// ---- host parse ----------------------------------------------------------------------------------------------------------------
// What the host reads of one file: the chunk headers up to IEND (never the image data).  status: IPX_OK (the chunks' CRCs and the zlib
// stream still have to be checked), IPX_ERR_INVALID (Go's reader fails on the container) or IPX_ERR_UNSUPPORTED (outside the GPU
// path: Adam7 unless the caller passes adam7, another chunk order, sub-byte gray with tRNS, ...).
struct PngSpan { uint32_t off, len; };   // bytes of the file
struct PngFileInfo {
    int status = 0;
    int w = 0, h = 0, kind = -1;
    int depth = 0, ctype = 0;
    int bpp = 1;                  // the filters' bytes per pixel: max(1, bits per pixel / 8)
    uint32_t rowbytes = 0;        // 1 + (bits per pixel * w + 7) / 8
    uint64_t raw_len = 0;         // h * rowbytes; Adam7: the sum over the non-empty passes of ph * (1 + (bits per pixel * pw + 7) / 8)
    bool interlace = false;       // Adam7 (only with adam7 set; otherwise such a file is UNSUPPORTED)
    uint32_t file_len = 0;        // through IEND's CRC
    uint32_t idat_len = 0;        // the zlib stream: every IDAT payload
    uint32_t idat_last = 0;       // where the last IDAT's payload starts in that stream
    bool trns = false;
    uint16_t trns_v[3] = {0, 0, 0};   // gray or R, G, B sample of tRNS
    std::vector<PngSpan> crc;     // per chunk: type + data (the CRC follows)
    std::vector<PngSpan> idat;    // IDAT payloads in file order
    uint8_t pal[1024];            // palette kinds: 256 x (R, G, B, A), tRNS applied, entries past PLTE opaque black
};
int png_parse(const uint8_t *p, size_t n, bool adam7, PngFileInfo *info);

// Adam7's pass p (0 .. 6): pixel (px, py) of the pass is pixel (xo + px * xf, yo + py * yf) of the frame.  One hex digit per pass.
struct PngPass { uint32_t xf, yf, xo, yo; };
__host__ __device__ inline PngPass png_pass(int p)
{
    const int s = 4 * p;
    return PngPass{(0x1224488u >> s) & 15, (0x2244888u >> s) & 15, (0x0102040u >> s) & 15, (0x1020400u >> s) & 15};
}
// the pass's width or height in a frame of n columns or rows (0: the pass is skipped, filter bytes and all)
__host__ __device__ inline uint32_t png_pass_dim(uint32_t n, uint32_t off, uint32_t f) { return n > off ? (n - off + f - 1) / f : 0; }

// ---- device side ---------------------------------------------------------------------------------------------------------------
// One piece of a chunk's CRC (a workgroup of png_crc_kernel): the piece's bytes at blob + src, its chunk, the bytes of the chunk after
// it; IDAT payload bytes are also copied to the file's zlib stream (from byte `skip` of the piece on, to zlib + dst; dst ~0: no copy).
struct PngCrcPiece {
    uint64_t src, dst;
    uint32_t len, chunk, after, skip;
};
// A chunk to check: its type + data at blob + off (cn bytes), the stored CRC right after, the file it belongs to.
struct PngChunk {
    uint64_t off;
    uint32_t cn, file;
};
// One file of an inflate / unfilter launch.
struct PngDecDesc {
    uint64_t zoff;      // its zlib stream at zlib + zoff (zlen bytes)
    uint64_t roff;      // its filtered rows at raw + roff (raw_len bytes), unfiltered in place
    uint64_t foff;      // its frame at frames + foff
    uint32_t zlen, raw_len;
    uint32_t zlast;     // the last IDAT's payload starts here in the stream: at or after the Adler-32's end is UNSUPPORTED
    uint32_t w, h, rowbytes, slot;
    uint16_t ctype, depth, kind, trns;   // trns: 1 when tRNS samples are compared (gray / truecolour)
    uint16_t tv[3], bpp;
    uint16_t interlace, pad;   // (pad: the size stays a multiple of 8 in the open)  interlace 1: the rows are Adam7's passes (png_unfilter_kernel<true>), 0: the frame's rows
};
// per-file status word, written by the kernels: 0 OK; bit 0 a chunk CRC differs; bit 1 the zlib stream breaks a rule of Go's reader;
// bit 2 a row's filter type is above 4; bit 3 bytes or an IDAT chunk follow the Adler-32 (UNSUPPORTED unless another bit is set)
enum : uint32_t { kPngBadCrc = 1, kPngBadZlib = 2, kPngBadFilter = 4, kPngTrailing = 8 };

hipError_t launch_png_crc(const uint8_t *blob, const PngCrcPiece *pieces, int npieces, uint32_t *acc, uint8_t *zlib, hipStream_t s);
hipError_t launch_png_crc_check(const uint8_t *blob, const PngChunk *chunks, int nchunks, const uint32_t *acc, uint32_t *status,
                                hipStream_t s);
hipError_t launch_png_inflate(const uint8_t *zlib, const PngDecDesc *desc, int n, uint8_t *raw, uint32_t *status, hipStream_t s);
// under IPX_PNG_PAR=1: the parallel inflate (ipx_png_dec_par.hip) and, behind it, the serial one for the files whose redo bit it set.
// par: the launch's word pairs (below), zero before; sub: the sub-sequence size in bits, kPngParSubMin .. kPngParSubMax.
// The per-file word pair of a launch under IPX_PNG_PAR=1 (par + 2 * slot): word 0 the tokens the parallel lanes decoded, word 1 those
// of the wave-uniform loop inside the parallel kernel; bit 31 of word 1 is the redo bit (the parallel kernel left the file: the serial
// launch behind it decodes it from scratch, and the two counts are 0).
constexpr uint32_t kPngParRedo = 0x80000000u;
constexpr int kPngParSub = 256, kPngParSubMin = 48, kPngParSubMax = 1000;
hipError_t launch_png_inflate_par(const uint8_t *zlib, const PngDecDesc *desc, int n, uint8_t *raw, const uint32_t *status, uint32_t *par,
                                  uint32_t sub, hipStream_t s);
hipError_t launch_png_inflate_redo(const uint8_t *zlib, const PngDecDesc *desc, int n, uint8_t *raw, uint32_t *status, const uint32_t *par,
                                   hipStream_t s);
hipError_t launch_png_unfilter(const PngDecDesc *desc, int n, uint8_t *raw, uint8_t *frames, uint32_t *status, hipStream_t s);
hipError_t launch_png_unfilter_adam7(const PngDecDesc *desc, int n, uint8_t *raw, uint8_t *frames, uint32_t *status, hipStream_t s);

// a file's frame as the packed layout (ipx_png_layout.h) takes it
inline PngFrameNeed png_frame_need(const PngFileInfo &f) { return PngFrameNeed{(size_t)f.w * f.h * png_kind_bpp(f.kind), f.kind == IPX_PNG_PALETTED}; }

}  // namespace ipx

// ---- the decode driver (ipx_png_dec_runtime.hip), as the entries and the legs (ipx_png_legs.hip) call it -------------------------
// parse n files on the host pool: status[i] and info[i] from the container (png_parse; IPX_PNG_ADAM7 is read here)
int png_parse_all(const ipx_bytes *files, int n, std::vector<ipx::PngFileInfo> &info, int *status);
// decodes files[at.idx[g]] into frames + at.off[g], its palette into slot at.pal_slot[g] of palettes (when set); verdicts in status
int png_decode_files(ipx_ctx *ctx, hipStream_t s, const ipx_bytes *files, const ipx::PngFrameLayout &at, const std::vector<ipx::PngFileInfo> &info,
                     uint8_t *frames, uint8_t *palettes, int *status);
