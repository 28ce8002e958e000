// ipx_gif_kernels.h -- the device bodies of gif.Encode that the uniform kernels (ipx_gif.hip: one geometry per launch, frame i found by
// arithmetic) and the mixed-size kernels (ipx_gif_mixed.hip: a record per frame) both run: what is done to a pixel, a code or a byte is
// stated once, here; a kernel only says where its frame lies.  Not part of the ABI.  DESIGN.md section 4.7.
#pragma once

#include "ipx_gif.h"

namespace ipx {

// ---- dither ----------------------------------------------------------------------------------------------------------------------
// The palette as drawPaletted holds it: color.RGBA.RGBA() of each entry, i.e. every byte x 0x101 (alpha is 0xffff throughout).
struct Plan9Taps {
    int4 c[256];
    constexpr Plan9Taps() : c{}
    {
        const Plan9 p;
        for (int i = 0; i < 256; i++) c[i] = int4{p.rgb[i][0] * 0x101, p.rgb[i][1] * 0x101, p.rgb[i][2] * 0x101, 0xffff};
    }
};
static __constant__ Plan9Taps c_plan9 = Plan9Taps();

__device__ inline int clamp16(int v) { return min(max(v, 0), 0xffff); }
// d * d for d <= 0xffff on the 24-bit multiplier (full rate); HIP's __umul24 returns int, and the product may exceed INT_MAX
__device__ inline uint32_t sq24(uint32_t d) { return (uint32_t)__umul24(d, d); }

// One workgroup per frame, R = blockDim.x rows in flight: thread r codes rows r, r + R, ... ("bands" of R rows); within a band row r
// handles pixel x = t - 2r at step t, so pixel (x, y) runs after (x - 1, y) and (x - 1 .. x + 1, y - 1), which is every error term it
// reads.  drawPaletted's quantErrorCurr[x + 1] for (x, y) is 3 e(x+1, y-1) + 5 e(x, y-1) + e(x-1, y-1) + 7 e(x-1, y): each thread keeps
// its last three errors (h1 h2 h3: steps t-1 .. t-3) and hands the row below 3 h1 + 5 h2 + h3 through a lane shuffle, through LDS at a
// wave boundary (one barrier per step, double-buffered by step parity), and through `cy` (global scratch, one int4 per column) from
// the last row of a band to the first row of the next.  All of it is int32 arithmetic: the order of the adds changes nothing, and the
// truncating division by 16 is applied once per pixel to the complete sum, as Go applies it.
// The search: the first minimum of sqDiff(r) + sqDiff(g) + sqDiff(b) + sqDiff(a) over the 256 entries.  Every entry has alpha 0xffff,
// so the alpha term is the same for all of them; every sum stays below 2^32 (four terms of at most 0x3fff8000), so dropping that term
// changes no comparison.  |d| <= 0xffff: d * d is the 24-bit multiplier's low 32 bits exactly.
// fs: the frame's pixels, rows `stride` apart; fi: its w * h indices; cy: its w int4s of carry.  Every thread of the workgroup calls
// it with the same arguments and reaches every barrier.
__device__ inline void gif_dither_frame(const uint8_t *__restrict__ fs, int w, int h, int stride, uint8_t *__restrict__ fi, int4 *__restrict__ cy)
{
    __shared__ int4 link[2][16];   // [step parity][wave]: what the last row of a wave hands the first row of the next
    const int R = blockDim.x;
    const int r = threadIdx.x, lane = r & 63, wv = r >> 6;
    const int4 zero{0, 0, 0, 0};
    for (int y0 = 0; y0 < h; y0 += R) {
        const int y = y0 + r;
        const bool row_ok = y < h;
        int4 h1 = zero, h2 = zero, h3 = zero, comb = zero;
        const int last = w + 2 * (R - 1);     // the band's last row reaches x = w here: it then hands over the terms of pixel w - 1
        for (int t = 0; t <= last; t++) {
            const int x = t - 2 * r;
            int4 up;
            up.x = __shfl_up(comb.x, 1, 64);
            up.y = __shfl_up(comb.y, 1, 64);
            up.z = __shfl_up(comb.z, 1, 64);
            up.w = __shfl_up(comb.w, 1, 64);
            if (lane == 0) {
                if (wv > 0) up = link[(t - 1) & 1][wv - 1];
                else if (y0 > 0 && x >= 0 && x < w) up = cy[x];
                else up = zero;
            }
            int4 e = zero;
            if (row_ok && x >= 0 && x < w) {
                const uint8_t *p = fs + (size_t)y * stride + 4 * (size_t)x;
                const int er = clamp16(p[0] * 0x101 + (up.x + 7 * h1.x) / 16);
                const int eg = clamp16(p[1] * 0x101 + (up.y + 7 * h1.y) / 16);
                const int eb = clamp16(p[2] * 0x101 + (up.z + 7 * h1.z) / 16);
                const int ea = clamp16(p[3] * 0x101 + (up.w + 7 * h1.w) / 16);
                uint32_t best_sum = 0xffffffffu;
                int best = 0;
#pragma unroll 16
                for (int i = 0; i < 256; i++) {
                    const int4 q = c_plan9.c[i];
                    const uint32_t dr = (uint32_t)abs(er - q.x), dg = (uint32_t)abs(eg - q.y), db = (uint32_t)abs(eb - q.z);
                    const uint32_t sum = (sq24(dr) >> 2) + (sq24(dg) >> 2) + (sq24(db) >> 2);
                    if (sum < best_sum) { best_sum = sum; best = i; }
                }
                fi[(size_t)y * w + x] = (uint8_t)best;
                const int4 q = c_plan9.c[best];
                e = int4{er - q.x, eg - q.y, eb - q.z, ea - 0xffff};
            }
            h3 = h2;
            h2 = h1;
            h1 = e;
            comb = int4{3 * h1.x + 5 * h2.x + h3.x, 3 * h1.y + 5 * h2.y + h3.y, 3 * h1.z + 5 * h2.z + h3.z, 3 * h1.w + 5 * h2.w + h3.w};
            if (lane == 63) link[t & 1][wv] = comb;
            if (r == R - 1 && x >= 1 && x <= w) cy[x - 1] = comb;   // the terms of pixel x - 1 of the row below (the next band's first)
            __syncthreads();
        }
    }
}

// ---- LZW -------------------------------------------------------------------------------------------------------------------------
// compress/lzw's writer (LSB, literal width 8) inside image/gif's blockWriter.  The codes it writes are fixed by the algorithm -- greedy
// longest match, a clear code first, width 9 at hi = 257 growing when hi reaches overflow, a clear code and an empty table when hi reaches
// 4095 (that key is not inserted), the saved code, incHi, EOF on Close -- not by Go's hash table, which only finds the matches.  Here the
// dictionary is an open-addressing table in LDS: 8192 entries of (key << 12 | code), key = prefix code << 8 | byte, 0 = empty; at most
// 3838 entries live between clears (load factor <= 0.47).  Lane 0 codes; the wave stages 4 KiB of indices in LDS at a time and clears the
// table.  Bytes go into 255-byte sub-blocks as they come; nothing is written at or past `region`.
constexpr int kLzwTab = 8192, kLzwChunk = 4096;

// One wave per frame.  src: the frame's npix indices; o: its region, whose first kGifHeaderBytes the calling kernel fills with the
// header (its own stores: nothing here reads them).  -> in lane 0 the word for lens[]: the stream's length, or 0xffffffff if the
// region was too small.
__device__ inline uint32_t gif_lzw_frame(const uint8_t *__restrict__ src, size_t npix, uint8_t *__restrict__ o, size_t region)
{
    __shared__ uint32_t table[kLzwTab];
    __shared__ uint8_t chunk[kLzwChunk];
    __shared__ int s_clear;
    const int lane = threadIdx.x;
    for (int i = lane; i < kLzwTab; i += 64) table[i] = 0;
    // the coder (meaningful in lane 0)
    uint32_t code = 0, hi = 257, width = 9, overflow = 512, bits = 0, nbits = 0, blk = 0;
    size_t pos = kGifHeaderBytes, lenpos = 0;
    bool over = false;
    auto put = [&](uint32_t byte) {
        if (blk == 0) lenpos = pos++;
        if (pos < region) o[pos] = (uint8_t)byte; else over = true;
        pos++;
        if (++blk == 255) {
            if (lenpos < region) o[lenpos] = 255;
            blk = 0;
        }
    };
    auto emit = [&](uint32_t c) {
        bits |= c << nbits;
        nbits += width;
        while (nbits >= 8) { put(bits & 0xff); bits >>= 8; nbits -= 8; }
    };
    auto inc_hi = [&]() {   // true: out of codes (a clear code went out; the table must be emptied)
        hi++;
        if (hi == overflow) { width++; overflow <<= 1; }
        if (hi == 4095) { emit(256); width = 9; hi = 257; overflow = 512; return true; }
        return false;
    };
    size_t base = 0;
    int p = 0;           // next byte of the staged chunk (lane 0)
    bool load = true;
    for (;;) {
        const int clen = (int)min((size_t)kLzwChunk, npix - base);
        if (load) {
            __syncthreads();
            for (int i = lane; i < clen; i += 64) chunk[i] = src[base + i];
            __syncthreads();
        }
        if (lane == 0) {
            s_clear = 0;
            if (base == 0 && p == 0) { emit(256); code = chunk[0]; p = 1; }
            while (p < clen) {
                const uint32_t lit = chunk[p++];
                const uint32_t key = code << 8 | lit;
                uint32_t slot = (key * 0x9E3779B1u) >> 19, t;
                bool hit = false;
                while ((t = table[slot]) != 0) {
                    if ((t >> 12) == key) { hit = true; break; }
                    slot = (slot + 1) & (kLzwTab - 1);
                }
                if (hit) { code = t & 4095; continue; }
                emit(code);
                code = lit;
                if (inc_hi()) { s_clear = 1; break; }
                table[slot] = key << 12 | hi;
            }
        }
        __syncthreads();
        if (s_clear) {
            for (int i = lane; i < kLzwTab; i += 64) table[i] = 0;
            __syncthreads();
            load = false;
            continue;
        }
        base += clen;
        p = 0;
        load = true;
        if (base >= npix) break;
    }
    uint32_t word = 0;
    if (lane == 0) {
        emit(code);
        (void)inc_hi();
        emit(257);
        if (nbits > 0) put(bits & 0xff);
        if (blk > 0 && lenpos < region) o[lenpos] = (uint8_t)blk;
        if (pos < region) o[pos] = 0;       // block terminator
        pos++;
        if (pos < region) o[pos] = 0x3B;    // trailer
        pos++;
        word = over || pos > region ? 0xffffffffu : (uint32_t)pos;
    }
    return word;
}

// ---- packing ---------------------------------------------------------------------------------------------------------------------
// a workgroup's share of the copy of one finished stream (len bytes at src, 16-byte aligned with a multiple of 16 behind it) to dst
__device__ inline void gif_pack_stream(const uint8_t *__restrict__ src, size_t len, uint8_t *__restrict__ dst)
{
    const size_t n16 = (len + 15) / 16;
    const uint4 *s = (const uint4 *)src;
    uint4 *d = (uint4 *)dst;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

// blocks of a packing grid's x dimension, sized by the longest stream
inline int gif_pack_blocks(size_t max_len) { return (int)std::min<size_t>(64, (max_len / 16 + 255) / 256 + 1); }

}  // namespace ipx
