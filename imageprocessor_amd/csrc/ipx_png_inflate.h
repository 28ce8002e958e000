// ipx_png_inflate.h -- the inflate of one zlib stream by one wave, as pieces: what the two kernels of ipx_png_dec_par.hip (under
// IPX_PNG_PAR=1) are made of -- png_inflate_par_kernel, whose lanes parse a Huffman block's body side by side, and png_inflate_redo_kernel,
// the serial walk behind it.  It restates png_inflate_kernel (ipx_png_dec.hip) step for step; that kernel keeps its own text, so that
// the code that runs while the switch is unset is the code it was, instruction for instruction (compiled through these pieces it took
// 155 VGPRs for 159 and ran 6 % slower).  The names live in ipx::flate.  Device code only; not part of the ABI.  DESIGN.md section 4.10.
//
// Every lane runs the same decoder on the same LDS bytes (broadcast reads; readfirstlane keeps the state scalar), so the symbol loop
// has no cross-lane hand-off; a match is copied by all 64 lanes, lane k taking bytes k, k + 64, ... from (k mod distance) behind the
// match for overlaps.  Nothing from global memory is on the per-symbol chain: the input is staged into LDS 8 KiB at a time, and
// finished window bytes leave in 16 KiB units.  Rules are Go's; every loop consumes input bits or produces output bytes, no write goes
// past raw_len, and input past the stream's end reads as zero bits that only count against the stream (consumed > 8 * zlen is an error).
#pragma once

#include "ipx_png_dec.h"

namespace ipx {
namespace flate {

constexpr int kInBytes = 8192;
constexpr int kWinBytes = 32768;
constexpr int kFlush = 16384;
constexpr int kLitRoot = 10, kDistRoot = 8, kClenRoot = 7;

struct PngFlate {
    uint16_t len_base[29], dist_base[30];
    uint8_t len_extra[29], dist_extra[30];
    uint8_t clen_order[19];
    constexpr PngFlate() : len_base{}, dist_base{}, len_extra{}, dist_extra{}, clen_order{16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}
    {
        const int lb[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        for (int s = 0; s < 29; s++) {
            len_base[s] = (uint16_t)lb[s];
            len_extra[s] = (uint8_t)(s < 8 || s == 28 ? 0 : (s - 4) / 4);
        }
        for (int s = 0; s < 30; s++) {
            dist_base[s] = (uint16_t)(s < 4 ? s + 1 : (1 << ((s >> 1) - 1)) * (2 + (s & 1)) + 1);
            dist_extra[s] = (uint8_t)(s < 4 ? 0 : (s >> 1) - 1);
        }
    }
};
static __constant__ PngFlate c_flate = PngFlate();

struct HuffLds { uint16_t count[16], first[16], offset[16], next[16]; };

// kWin: the window ring's bytes (a power of two, at least 32 KiB)
template <int kWin>
struct InflateLds {
    uint8_t win[kWin];
    uint8_t in[kInBytes + 16];
    uint16_t lit_root[1 << kLitRoot];
    uint16_t dist_root[1 << kDistRoot];    // also the code-length code's table during a dynamic header
    uint16_t lit_sorted[288], dist_sorted[32], clen_sorted[19];
    HuffLds lit, dist, clen;
    uint8_t lens[320];
    uint8_t clens[20];
    int ok;
};

__device__ inline uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// Go's huffmanDecoder.init over lens[0 .. n): false unless the code is complete, empty, or a single code of length 1.  On success
// the canonical arrays (count / first / offset per length, symbols sorted by code) and the root table (entry: symbol << 4 | length,
// 0 for a longer code or none) are built.  Called by every lane.
__device__ inline bool huff_build(const uint8_t *lens, int n, HuffLds &h, uint16_t *sorted, uint16_t *root, int rbits, int lane, int *s_ok)
{
    if (lane == 0) {
        for (int L = 0; L < 16; L++) h.count[L] = 0;
        for (int s = 0; s < n; s++) h.count[lens[s]]++;
        h.count[0] = 0;
        int mn = 0, mx = 0;
        for (int L = 1; L < 16; L++)
            if (h.count[L]) { if (!mn) mn = L; mx = L; }
        bool ok = true;
        if (mx) {
            int code = 0;
            for (int L = mn; L <= mx; L++) code = (code << 1) + h.count[L];
            ok = code == (1 << mx) || (code == 1 && mx == 1);
        }
        int c = 0, off = 0;
        h.first[0] = 0;
        h.offset[0] = 0;
        for (int L = 1; L < 16; L++) {
            c = (c + (L > 1 ? h.count[L - 1] : 0)) << 1;
            h.first[L] = (uint16_t)c;
            h.offset[L] = (uint16_t)off;
            h.next[L] = (uint16_t)off;
            off += h.count[L];
        }
        if (ok)
            for (int s = 0; s < n; s++)
                if (lens[s]) sorted[h.next[lens[s]]++] = (uint16_t)s;
        *s_ok = ok;
    }
    __syncthreads();
    if (!uni((uint32_t)*s_ok)) return false;
    for (int e = lane; e < (1 << rbits); e += 64) root[e] = 0;
    __syncthreads();
    const int total = h.offset[15] + h.count[15];
    for (int p = lane; p < total; p += 64) {
        const int s = sorted[p], L = lens[s];
        if (L > rbits) continue;
        const uint32_t code = h.first[L] + (uint32_t)(p - h.offset[L]);
        const uint32_t r = __brev(code) >> (32 - L);
        for (uint32_t e = r; e < (1u << rbits); e += 1u << L) root[e] = (uint16_t)(s << 4 | L);
    }
    __syncthreads();
    return true;
}

// the symbol at the head of bb (its length in *len), or -1 when no code matches (Go: "invalid code")
__device__ inline int huff_decode(uint64_t bb, const uint16_t *root, int rbits, const HuffLds &h, const uint16_t *sorted, int *len)
{
    const uint32_t e = uni(root[bb & ((1u << rbits) - 1)]);
    if (e) { *len = (int)(e & 15); return (int)(e >> 4); }
    const uint32_t rev = __brev((uint32_t)bb & 0x7FFF) >> 17;   // the next 15 bits, the first one most significant
    for (int L = rbits + 1; L <= 15; L++) {
        const uint32_t k = (rev >> (15 - L)) - uni(h.first[L]);
        if (k < uni(h.count[L])) { *len = L; return (int)uni(sorted[uni(h.offset[L]) + k]); }
    }
    *len = 0;
    return -1;
}

// One file's inflate state, the same in every lane of the wave.  The kernels drive it: zlib_header, then per block block_head and,
// for a Huffman block, the block's tokens (tokens<false>, or the parallel parse), then finish.
template <int kWin>
struct Inflater {
    InflateLds<kWin> &S;
    const int lane;
    const uint8_t *z;
    uint8_t *out;
    const uint32_t zlen, raw_len, zlast;
    const uint64_t zbits;
    uint32_t in_base = 0, bpos = 0, pos = 0, flushed = 0, a1 = 1, b1 = 0;
    uint64_t bb = 0;
    uint32_t nb = 0;
    bool err = false, final_block = false, fixed_built = false;

    __device__ __forceinline__ Inflater(InflateLds<kWin> &lds, int lane_, const PngDecDesc &d, const uint8_t *zlib, uint8_t *raw)
        : S(lds), lane(lane_), z(zlib + d.zoff), out(raw + d.roff), zlen(d.zlen), raw_len(d.raw_len), zlast(d.zlast), zbits(8ull * d.zlen)
    {
    }

    __device__ __forceinline__ void stage(uint32_t at)          // in[] <- stream bytes [at & ~15, +kInBytes), zero past the end
    {
        in_base = at & ~15u;
        for (int i = lane; i < kInBytes / 16; i += 64) {
            const uint32_t g = in_base + 16 * i;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g < zlen) v = *(const uint4 *)(z + g);
            *(uint4 *)(S.in + 16 * i) = v;
            if (g < zlen && g + 16 > zlen)
                for (uint32_t j = zlen - g; j < 16; j++) S.in[16 * i + j] = 0;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void restage() { if (bpos - in_base > (uint32_t)kInBytes - 64) stage(bpos); }
    __device__ __forceinline__ void refill()
    {
        if (nb < 32) {
            const uint32_t o = bpos - in_base;
            const uint32_t v = uni((uint32_t)S.in[o] | (uint32_t)S.in[o + 1] << 8 | (uint32_t)S.in[o + 2] << 16 | (uint32_t)S.in[o + 3] << 24);
            bb |= (uint64_t)v << nb;
            nb += 32;
            bpos += 4;
        }
    }
    __device__ __forceinline__ uint32_t take(uint32_t k) { const uint32_t v = (uint32_t)bb & ((1u << k) - 1); bb >>= k; nb -= k; return v; }
    __device__ __forceinline__ bool over() const { return (uint64_t)bpos * 8 - nb > zbits; }
    __device__ __forceinline__ uint64_t bit_at() const { return (uint64_t)bpos * 8 - nb; }       // the next unread bit of the stream
    __device__ __forceinline__ void seek(uint64_t bit)          // the reader restarts at that bit (the parallel parse hands back)
    {
        bpos = (uint32_t)(bit >> 3);
        bb = 0;
        nb = 0;
        if (bpos < in_base || bpos - in_base > (uint32_t)kInBytes - 64) stage(bpos);
        refill();
        take((uint32_t)bit & 7);
    }
    __device__ __forceinline__ void adler(uint32_t F, uint64_t A, uint64_t B)
    {
        for (int off = 32; off > 0; off >>= 1) { A += __shfl_xor(A, off, 64); B += __shfl_xor(B, off, 64); }
        b1 = (uint32_t)((b1 + (uint64_t)(F % 65521) * a1 + B % 65521) % 65521);
        a1 = (uint32_t)((a1 + A % 65521) % 65521);
    }
    __device__ __forceinline__ void flush_units()               // every whole 16 KiB unit behind pos: coalesced 16-byte stores
    {
        while (pos - flushed >= (uint32_t)kFlush) {
            const uint4 *src = (const uint4 *)(S.win + (flushed & (kWin - 1)));
            uint4 *dst = (uint4 *)(out + flushed);
            uint64_t A = 0, B = 0;
            for (int i = lane; i < kFlush / 16; i += 64) {
                const uint4 v = src[i];
                dst[i] = v;
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const uint32_t byte = (wd[k >> 2] >> (8 * (k & 3))) & 0xFF;
                    A += byte;
                    B += (uint64_t)(kFlush - (16 * i + k)) * byte;
                }
            }
            adler(kFlush, A, B);
            flushed += kFlush;
        }
    }

    __device__ __forceinline__ void zlib_header()
    {
        stage(0);
        refill();
        const uint32_t cmf = take(8), flg = take(8);
        if (zlen < 2 || (cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) err = true;
    }

    // The next block's header.  A stored block is copied here and false comes back (so does it on an error: err is set); true: a
    // Huffman block's tables stand in S and its first token is next.
    __device__ __forceinline__ bool block_head()
    {
        restage();
        refill();
        final_block = take(1);
        const uint32_t type = take(2);
        if (over()) { err = true; return false; }
        if (type == 0) {                                         // stored
            take(nb & 7);
            bpos -= nb >> 3;
            bb = 0;
            nb = 0;
            restage();
            if (bpos + 4 > zlen) { err = true; return false; }
            const uint32_t o = bpos - in_base;
            const uint32_t len = uni(S.in[o] | (uint32_t)S.in[o + 1] << 8), nlen = uni(S.in[o + 2] | (uint32_t)S.in[o + 3] << 8);
            bpos += 4;
            if (len != (~nlen & 0xFFFF) || bpos + len > zlen || pos + len > raw_len) { err = true; return false; }
            uint32_t left = len;
            while (left) {
                restage();
                const uint32_t k = min(min(left, in_base + kInBytes - 16 - bpos), (uint32_t)kFlush);
                const uint32_t o2 = bpos - in_base;
                for (uint32_t j = lane; j < k; j += 64) S.win[(pos + j) & (kWin - 1)] = S.in[o2 + j];
                pos += k;
                bpos += k;
                left -= k;
                __syncthreads();
                flush_units();
            }
            return false;
        }
        if (type == 3) { err = true; return false; }
        if (type == 1) {
            if (!fixed_built) {
                for (int s = lane; s < 320; s += 64) S.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                __syncthreads();
                huff_build(S.lens, 288, S.lit, S.lit_sorted, S.lit_root, kLitRoot, lane, &S.ok);
                huff_build(S.lens + 288, 32, S.dist, S.dist_sorted, S.dist_root, kDistRoot, lane, &S.ok);
                fixed_built = true;
            }
        } else {                                                 // dynamic: the header, the code-length code, the two codes
            fixed_built = false;
            refill();
            const uint32_t hlit = take(5) + 257, hdist = take(5) + 1, hclen = take(4) + 4;
            if (hlit > 286 || hdist > 30) { err = true; return false; }
            for (uint32_t k = 0; k < 19; k++) {
                uint32_t v = 0;
                if (k < hclen) { refill(); v = take(3); }
                if (lane == 0) S.clens[c_flate.clen_order[k]] = (uint8_t)v;
            }
            __syncthreads();
            if (over() || !huff_build(S.clens, 19, S.clen, S.clen_sorted, S.dist_root, kClenRoot, lane, &S.ok)) { err = true; return false; }
            const uint32_t n = hlit + hdist;
            for (uint32_t i = 0; i < n;) {
                restage();
                refill();
                int L;
                const int sym = huff_decode(bb, S.dist_root, kClenRoot, S.clen, S.clen_sorted, &L);
                if (sym < 0) { err = true; break; }
                take(L);
                if (sym < 16) {
                    if (lane == 0) S.lens[i] = (uint8_t)sym;
                    i++;
                } else {
                    uint32_t rep, val = 0;
                    if (sym == 16) {
                        if (i == 0) { err = true; break; }
                        rep = 3 + take(2);
                        val = uni(S.lens[i - 1]);
                    } else if (sym == 17) {
                        rep = 3 + take(3);
                    } else {
                        rep = 11 + take(7);
                    }
                    if (i + rep > n) { err = true; break; }
                    for (uint32_t j = lane; j < rep; j += 64) S.lens[i + j] = (uint8_t)val;
                    i += rep;
                }
                __syncthreads();
                if (over()) { err = true; break; }
            }
            if (err) return false;
            if (!huff_build(S.lens, hlit, S.lit, S.lit_sorted, S.lit_root, kLitRoot, lane, &S.ok) ||
                !huff_build(S.lens + hlit, hdist, S.dist, S.dist_sorted, S.dist_root, kDistRoot, lane, &S.ok)) { err = true; return false; }
        }
        return true;
    }

    // The block's tokens, one after the other, to its end-of-block symbol (true comes back).  kBounded (the parallel kernel's stretches
    // that no round can take): only the tokens that start before stream bit `until` -- false comes back when the next one does not --
    // and every token, the end-of-block symbol too, is counted in *ntok.
    template <bool kBounded>
    __device__ __forceinline__ bool tokens(uint64_t until, uint32_t *ntok)
    {
        const uint16_t *lroot = S.lit_root, *droot = S.dist_root;
        for (;;) {
            if (kBounded && bit_at() >= until) return false;
            restage();
            refill();
            int L;
            const int sym = huff_decode(bb, lroot, kLitRoot, S.lit, S.lit_sorted, &L);
            if (sym < 0) { err = true; break; }
            take(L);
            if (kBounded) ++*ntok;
            if (sym < 256) {
                if (pos >= raw_len) { err = true; break; }       // too much pixel data
                if (lane == 0) S.win[pos & (kWin - 1)] = (uint8_t)sym;
                pos++;
            } else if (sym == 256) {
                if (over()) err = true;
                break;
            } else if (sym > 285) {
                err = true;
                break;
            } else {
                const int li = sym - 257;
                const uint32_t len = c_flate.len_base[li] + take(c_flate.len_extra[li]);
                refill();
                const int ds = huff_decode(bb, droot, kDistRoot, S.dist, S.dist_sorted, &L);
                if (ds < 0 || ds >= 30) { err = true; break; }
                take(L);
                const uint32_t dist = c_flate.dist_base[ds] + take(c_flate.dist_extra[ds]);
                if (over() || dist > pos || pos + len > raw_len) { err = true; break; }
                __syncthreads();
                const uint32_t from = pos - dist;
                for (uint32_t j = lane; j < len; j += 64)
                    S.win[(pos + j) & (kWin - 1)] = S.win[(from + (dist >= len ? j : j % dist)) & (kWin - 1)];
                pos += len;
                __syncthreads();
            }
            if (over()) { err = true; break; }
            if (pos - flushed >= (uint32_t)kFlush) {
                __syncthreads();
                flush_units();
            }
        }
        return true;
    }

    // Behind the final block: the length, the last partial unit, the Adler-32 and what follows it.  true: the stream is in order (then
    // *trailing says whether bytes or an IDAT chunk follow the Adler-32); false: it breaks a rule.
    __device__ __forceinline__ bool finish(bool *trailing)
    {
        *trailing = false;
        if (!err && pos != raw_len) err = true;                  // not enough pixel data
        if (!err) {
            __syncthreads();
            const uint32_t F = pos - flushed;                    // the last partial unit, byte by byte
            uint64_t A = 0, B = 0;
            for (uint32_t j = lane; j < F; j += 64) {
                const uint32_t byte = S.win[(flushed + j) & (kWin - 1)];
                out[flushed + j] = (uint8_t)byte;
                A += byte;
                B += (uint64_t)(F - j) * byte;
            }
            adler(F, A, B);
            take(nb & 7);                                        // the Adler-32 follows at the next byte
            bpos -= nb >> 3;
            bb = 0;
            nb = 0;
            restage();
            if (bpos + 4 > zlen) {
                err = true;
            } else {
                const uint32_t o = bpos - in_base;
                const uint32_t want = uni((uint32_t)S.in[o] << 24 | (uint32_t)S.in[o + 1] << 16 | (uint32_t)S.in[o + 2] << 8 | S.in[o + 3]);
                if (want != (b1 << 16 | a1)) err = true;
                else *trailing = bpos + 4 < zlen || zlast >= bpos + 4;
            }
        }
        return !err;
    }
};

}  // namespace flate
}  // namespace ipx
