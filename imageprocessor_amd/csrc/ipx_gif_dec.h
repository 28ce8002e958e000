// ipx_gif_dec.h -- gif.Decode (the first image of a file) on the GPU: what the kernels (ipx_gif_dec.hip) and the host half
// (ipx_gif_dec_host.cpp) share.  Not part of the ABI.  The restatement of Go's reader is in DESIGN.md section 4.8;
// tests/gif_decode_model.py is the model it is held to.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ipx {

// ---- host parse ----------------------------------------------------------------------------------------------------------------
// What the host reads of one file: the container up to the first image's LZW minimum code size, then the sub-block framing of its
// image data.  status: IPX_OK (the image data still has to be decoded), IPX_ERR_INVALID (Go's reader fails before the image data:
// header, tables, extensions, descriptor, code size) or IPX_ERR_UNSUPPORTED (a geometry the GPU path does not take: a non-zero
// origin, an empty frame, a frame beyond the span the kernels address, a file of 2 GiB or more).
struct GifFileInfo {
    int status = 0;
    int left = 0, top = 0, w = 0, h = 0;
    int lit = 0;
    bool interlaced = false;
    bool terminated = false;     // the sub-blocks end in a block terminator (else the file ends first: Go fails once it reads there)
    bool last_is_one = false;    // the last sub-block holds one byte
    size_t data_pos = 0;         // offset in the file of the first sub-block's length byte
    uint32_t data_len = 0;       // bytes of LZW data in the complete sub-blocks
    uint32_t last_start = 0;     // offset in that data of the last sub-block's first byte
    uint32_t pal_len = 0;        // len(m.Palette) (the transparent index may lengthen it past the table)
    uint8_t pal[1024];           // 256 x (R, G, B, A): opaque entries A = 255, the transparent entry and unused entries zero
};
int gif_parse(const uint8_t *p, size_t n, GifFileInfo *info);
// the LZW bytes of the complete sub-blocks, framing stripped, to dst (info.data_len bytes)
void gif_gather(const uint8_t *p, size_t n, const GifFileInfo &info, uint8_t *dst);
// entries of code scratch a file needs: one per code that outputs bytes (at most one per 3 bits of data and at most one per pixel:
// the walk stops at the first byte past the frame) plus the closing offset
uint32_t gif_code_cap(const GifFileInfo &info);

// ---- device side ---------------------------------------------------------------------------------------------------------------
enum : uint8_t { kGifTerminated = 1, kGifLastIsOne = 2, kGifInterlaced = 4 };
struct GifDecDesc {              // one file of a launch
    uint64_t data_off;           // its LZW bytes at blob + data_off
    uint64_t code_off;           // its code scratch: code_cap entries at codes + code_off
    uint64_t frame_off;          // its frame: w x h bytes, rows tight, at frames + frame_off
    uint32_t data_len, last_start, code_cap;
    uint32_t w, h;
    uint32_t pal_len;            // 256 or more: no index is out of range
    uint32_t slot;               // its state words: state + kGifStateWords * slot (the file's place in the call)
    uint16_t lit;
    uint8_t flags, pad;
};
// One record per code that outputs bytes, written by the code walk: its string goes to [off, next record's off) of the frame's
// (interlaced) pixel order.  segb: the record index of its segment's first code (since the last clear code); the code at ordinal
// t >= 1 of a segment defines the entry eof + t = (the string of the code before it) + (the first byte of its own string).
// packed: value (12 bits) | the previous code's value in the segment (12 bits) << 12 | the first byte of its string << 24.
struct GifCode { uint32_t off, segb, packed; };
// per file, after the walk: [0] status (0: decoded, 1: Go's reader fails on the image data, 2: the code scratch was too small --
// cannot happen with gif_code_cap), [1] records written; under IPX_GIF_PAR=1 also [2] the redo word (gif_walk_par_kernel left the file
// to the serial walk) and [3] the records the parallel lanes wrote (0 for a file it left)
constexpr int kGifStateWords = 4;

// redo: nullptr, or the files' redo words (redo[kGifStateWords * slot]): then only the files whose word is set are walked
hipError_t launch_gif_walk(const uint8_t *blob, const GifDecDesc *desc, int n, GifCode *codes, uint32_t *state, const uint32_t *redo,
                           hipStream_t s);
// under IPX_GIF_PAR=1 (ipx_gif_dec_par.hip): the 64 lanes of a file's wave read its codes side by side; writes all four state words
hipError_t launch_gif_walk_par(const uint8_t *blob, const GifDecDesc *desc, int n, GifCode *codes, uint32_t *state, hipStream_t s);
// blocks_per_file: workgroups of 256 lanes striding over a file's records
hipError_t launch_gif_expand(const GifDecDesc *desc, int n, const GifCode *codes, const uint32_t *state, uint8_t *frames,
                             int blocks_per_file, hipStream_t s);

// ---- where one gif_decode_files call (ipx_gif_dec.hip) puts what it decodes --------------------------------------------------------
// A block of frames and a block of 1024-byte palette slots, and for every file of the call its place in each.
struct GifFrameLayout {
    std::vector<size_t> off;     // frame offset of file i (256-byte aligned); unused for a file that is not decoded
    std::vector<int> pal_slot;   // palette slot of file i, or -1: none is written (a slot of a file that is not decoded is zeroed)
    size_t bytes = 0;            // of the frame block
    int pal_slots = 0;           // of the palette block
    // The walk is one wave per file and a launch ends with its longest file: with files of different sizes the records of a launch are
    // ordered longest data first (what is written depends on nothing but a file's own record).  Files of one size keep the caller's
    // order, in which neighbouring workgroups write neighbouring frames: sorted, 1024 flat 1024x768 files measured 8 % slower.
    bool longest_first = false;
};
// n frames of one size fs bytes (a multiple of 256) apart, file i's frame and palette the i-th (ipx_gif_decode_batch, run_gif_gif)
inline GifFrameLayout gif_layout_strided(int n, size_t fs)
{
    GifFrameLayout at;
    for (int i = 0; i < n; i++) { at.off.push_back((size_t)i * fs); at.pal_slot.push_back(i); }
    at.bytes = (size_t)n * fs;
    at.pal_slots = n;
    return at;
}
// Frames of any sizes back to back, each at the next multiple of 256, and palette slots 0, 1, ... for the files take(i) says are decoded,
// in the order of the call; the others get neither (ipx_gif_decode_mixed, ipx_run_gif_gif_mixed).  Neighbours of one size lie
// align256(w * h) apart.  frame_bytes(i): w * h of file i.
template <class Take, class Bytes> inline GifFrameLayout gif_layout_packed(int n, Take take, Bytes frame_bytes)
{
    GifFrameLayout at;
    at.longest_first = true;
    for (int i = 0; i < n; i++) {
        if (!take(i)) { at.off.push_back(0); at.pal_slot.push_back(-1); continue; }
        at.off.push_back(at.bytes);
        at.pal_slot.push_back(at.pal_slots++);
        at.bytes += ((size_t)frame_bytes(i) + 255) & ~(size_t)255;
    }
    return at;
}

}  // namespace ipx
