// ipx_png_dec.hip -- png.Decode (image/png reader.go, compress/zlib, compress/flate) of a batch of files on the GPU: the kernels and
// their launchers.  Kernels: the CRC of every chunk in pieces (combined with crc_shift) that also gathers the IDAT payloads
// into one zlib stream per file, the per-chunk check, the inflate (one wave per file: input, Huffman tables and the 32 KiB window in
// LDS, match copies spread over the lanes, coalesced flushes with the Adler-32) and the unfilter (a diagonal wavefront of 64 rows that
// writes the frame layout of the type Go returns; for Adam7 files, taken under IPX_PNG_ADAM7=1, one such wave per pass that scatters
// its pixels to where the pass puts them).  Every kernel takes a workgroup per file and reads the file's own descriptor, so one pass
// decodes files of any sizes and kinds.  The driver and the decode entries: ipx_png_dec_runtime.hip; the PNG-in, PNG-out legs:
// ipx_png_legs.hip; the host parse: ipx_png_dec_host.cpp.  DESIGN.md section 4.10.
#include "ipx_png.h"
#include "ipx_png_dec.h"

namespace ipx {

__constant__ PngCrcTables c_dec_crc = PngCrcTables();

// ---- CRC and gather --------------------------------------------------------------------------------------------------------------
// A workgroup per piece: each lane the CRC of a contiguous range, shifted by the bytes of the chunk after it; the XOR of the shifted
// states is the chunk's raw CRC (the initial ~0 is added by the check).  IDAT payload bytes are copied to the zlib streams on the way.
__global__ __launch_bounds__(256) void png_crc_kernel(const uint8_t *__restrict__ blob, const PngCrcPiece *__restrict__ pieces,
                                                      uint32_t *__restrict__ acc, uint8_t *__restrict__ zlib)
{
    __shared__ uint32_t s_tab[256];
    __shared__ uint32_t s_sum[4];
    const int t = threadIdx.x;
    s_tab[t] = c_dec_crc.crc[t];
    const PngCrcPiece pc = pieces[blockIdx.x];
    const uint8_t *src = blob + pc.src;
    if (pc.dst != ~0ull)
        for (uint32_t i = pc.skip + t; i < pc.len; i += 256) zlib[pc.dst + (i - pc.skip)] = src[i];
    __syncthreads();
    const uint32_t per = (pc.len + 255) / 256, b0 = min(pc.len, per * t), b1 = min(pc.len, b0 + per);
    uint32_t c = 0;
    for (uint32_t q = b0; q < b1; q++) c = s_tab[(c ^ src[q]) & 0xFF] ^ (c >> 8);
    uint32_t x = b1 > b0 ? crc_shift(c, pc.len - b1 + pc.after, c_dec_crc.x2n) : 0;
    for (int off = 32; off > 0; off >>= 1) x ^= __shfl_xor(x, off, 64);
    if ((t & 63) == 0) s_sum[t >> 6] = x;
    __syncthreads();
    if (t == 0) atomicXor(acc + pc.chunk, s_sum[0] ^ s_sum[1] ^ s_sum[2] ^ s_sum[3]);
}

__global__ __launch_bounds__(256) void png_crc_check_kernel(const uint8_t *__restrict__ blob, const PngChunk *__restrict__ chunks, int n,
                                                            const uint32_t *__restrict__ acc, uint32_t *__restrict__ status)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const PngChunk ch = chunks[k];
    const uint32_t crc = ~(crc_shift(0xFFFFFFFFu, ch.cn, c_dec_crc.x2n) ^ acc[k]);
    const uint8_t *p = blob + ch.off + ch.cn;
    const uint32_t stored = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    if (crc != stored) atomicOr(status + ch.file, kPngBadCrc);
}

hipError_t launch_png_crc(const uint8_t *blob, const PngCrcPiece *pieces, int npieces, uint32_t *acc, uint8_t *zlib, hipStream_t s)
{
    if (npieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_crc_kernel, dim3(npieces), dim3(256), 0, s, blob, pieces, acc, zlib);
    return hipGetLastError();
}

hipError_t launch_png_crc_check(const uint8_t *blob, const PngChunk *chunks, int nchunks, const uint32_t *acc, uint32_t *status,
                                hipStream_t s)
{
    if (nchunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_crc_check_kernel, dim3((nchunks + 255) / 256), dim3(256), 0, s, blob, chunks, nchunks, acc, status);
    return hipGetLastError();
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------
// One workgroup of one wave per file.  Every lane runs the same decoder on the same LDS bytes (broadcast reads; readfirstlane keeps
// the state scalar), so the symbol loop has no cross-lane hand-off; a match is copied by all 64 lanes, lane k taking bytes k, k + 64, ...
// from (k mod distance) behind the match for overlaps.  Nothing from global memory is on the per-symbol chain: the input is staged into
// LDS 8 KiB at a time, and finished window bytes leave in 16 KiB units.  Rules are Go's; every loop consumes
// input bits or produces output bytes, no write goes past raw_len, and input past the stream's end reads as zero bits that only count
// against the stream (consumed > 8 * zlen is an error).
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
__constant__ PngFlate c_flate = PngFlate();

struct HuffLds { uint16_t count[16], first[16], offset[16], next[16]; };

struct InflateLds {
    uint8_t win[kWinBytes];
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
__device__ bool huff_build(const uint8_t *lens, int n, HuffLds &h, uint16_t *sorted, uint16_t *root, int rbits, int lane, int *s_ok)
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

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t *__restrict__ zlib, const PngDecDesc *__restrict__ desc,
                                                         uint8_t *__restrict__ raw, uint32_t *__restrict__ status)
{
    __shared__ InflateLds S;
    const int lane = threadIdx.x;
    const PngDecDesc d = desc[blockIdx.x];
    const uint8_t *z = zlib + d.zoff;
    uint8_t *out = raw + d.roff;
    const uint32_t zlen = d.zlen, raw_len = d.raw_len;
    const uint64_t zbits = 8ull * zlen;
    uint32_t in_base = 0, bpos = 0, pos = 0, flushed = 0, a1 = 1, b1 = 0;
    uint64_t bb = 0;
    uint32_t nb = 0;
    bool err = false, final_block = false, fixed_built = false;
    if (status[d.slot] & kPngBadCrc) return;

    auto stage = [&](uint32_t at) {          // in[] <- stream bytes [at & ~15, +kInBytes), zero past the end
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
    };
    auto restage = [&]() { if (bpos - in_base > (uint32_t)kInBytes - 64) stage(bpos); };
    auto refill = [&]() {
        if (nb < 32) {
            const uint32_t o = bpos - in_base;
            const uint32_t v = uni((uint32_t)S.in[o] | (uint32_t)S.in[o + 1] << 8 | (uint32_t)S.in[o + 2] << 16 | (uint32_t)S.in[o + 3] << 24);
            bb |= (uint64_t)v << nb;
            nb += 32;
            bpos += 4;
        }
    };
    auto take = [&](uint32_t k) -> uint32_t { const uint32_t v = (uint32_t)bb & ((1u << k) - 1); bb >>= k; nb -= k; return v; };
    auto over = [&]() { return (uint64_t)bpos * 8 - nb > zbits; };
    auto adler = [&](uint32_t F, uint64_t A, uint64_t B) {
        for (int off = 32; off > 0; off >>= 1) { A += __shfl_xor(A, off, 64); B += __shfl_xor(B, off, 64); }
        b1 = (uint32_t)((b1 + (uint64_t)(F % 65521) * a1 + B % 65521) % 65521);
        a1 = (uint32_t)((a1 + A % 65521) % 65521);
    };
    auto flush_units = [&]() {               // every whole 16 KiB unit behind pos: coalesced 16-byte stores
        while (pos - flushed >= (uint32_t)kFlush) {
            const uint4 *src = (const uint4 *)(S.win + (flushed & (kWinBytes - 1)));
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
    };

    stage(0);
    refill();
    {
        const uint32_t cmf = take(8), flg = take(8);
        if (zlen < 2 || (cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) err = true;
    }
    while (!err && !final_block) {
        restage();
        refill();
        final_block = take(1);
        const uint32_t type = take(2);
        if (over()) { err = true; break; }
        if (type == 0) {                                         // stored
            take(nb & 7);
            bpos -= nb >> 3;
            bb = 0;
            nb = 0;
            restage();
            if (bpos + 4 > zlen) { err = true; break; }
            const uint32_t o = bpos - in_base;
            const uint32_t len = uni(S.in[o] | (uint32_t)S.in[o + 1] << 8), nlen = uni(S.in[o + 2] | (uint32_t)S.in[o + 3] << 8);
            bpos += 4;
            if (len != (~nlen & 0xFFFF) || bpos + len > zlen || pos + len > raw_len) { err = true; break; }
            uint32_t left = len;
            while (left) {
                restage();
                const uint32_t k = min(min(left, in_base + kInBytes - 16 - bpos), (uint32_t)kFlush);
                const uint32_t o2 = bpos - in_base;
                for (uint32_t j = lane; j < k; j += 64) S.win[(pos + j) & (kWinBytes - 1)] = S.in[o2 + j];
                pos += k;
                bpos += k;
                left -= k;
                __syncthreads();
                flush_units();
            }
            continue;
        }
        if (type == 3) { err = true; break; }
        const uint16_t *lroot = S.lit_root, *droot = S.dist_root;
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
            if (hlit > 286 || hdist > 30) { err = true; break; }
            for (uint32_t k = 0; k < 19; k++) {
                uint32_t v = 0;
                if (k < hclen) { refill(); v = take(3); }
                if (lane == 0) S.clens[c_flate.clen_order[k]] = (uint8_t)v;
            }
            __syncthreads();
            if (over() || !huff_build(S.clens, 19, S.clen, S.clen_sorted, S.dist_root, kClenRoot, lane, &S.ok)) { err = true; break; }
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
            if (err) break;
            if (!huff_build(S.lens, hlit, S.lit, S.lit_sorted, S.lit_root, kLitRoot, lane, &S.ok) ||
                !huff_build(S.lens + hlit, hdist, S.dist, S.dist_sorted, S.dist_root, kDistRoot, lane, &S.ok)) { err = true; break; }
        }
        for (;;) {                                               // the block's symbols
            restage();
            refill();
            int L;
            const int sym = huff_decode(bb, lroot, kLitRoot, S.lit, S.lit_sorted, &L);
            if (sym < 0) { err = true; break; }
            take(L);
            if (sym < 256) {
                if (pos >= raw_len) { err = true; break; }       // too much pixel data
                if (lane == 0) S.win[pos & (kWinBytes - 1)] = (uint8_t)sym;
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
                    S.win[(pos + j) & (kWinBytes - 1)] = S.win[(from + (dist >= len ? j : j % dist)) & (kWinBytes - 1)];
                pos += len;
                __syncthreads();
            }
            if (over()) { err = true; break; }
            if (pos - flushed >= (uint32_t)kFlush) {
                __syncthreads();
                flush_units();
            }
        }
    }
    if (!err && pos != raw_len) err = true;                      // not enough pixel data
    bool trailing = false;
    if (!err) {
        __syncthreads();
        const uint32_t F = pos - flushed;                        // the last partial unit, byte by byte
        uint64_t A = 0, B = 0;
        for (uint32_t j = lane; j < F; j += 64) {
            const uint32_t byte = S.win[(flushed + j) & (kWinBytes - 1)];
            out[flushed + j] = (uint8_t)byte;
            A += byte;
            B += (uint64_t)(F - j) * byte;
        }
        adler(F, A, B);
        take(nb & 7);                                            // the Adler-32 follows at the next byte
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
            else trailing = bpos + 4 < zlen || d.zlast >= bpos + 4;
        }
    }
    if (lane == 0 && (err || trailing)) atomicOr(status + d.slot, err ? kPngBadZlib : kPngTrailing);
}

hipError_t launch_png_inflate(const uint8_t *zlib, const PngDecDesc *desc, int n, uint8_t *raw, uint32_t *status, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(64), 0, s, zlib, desc, raw, status);
    return hipGetLastError();
}

// ---- unfilter and convert --------------------------------------------------------------------------------------------------------
// One wave per file, bands of 64 rows: lane i owns row r0 + i and at step t reconstructs its unit (bpp bytes; one byte at sub-byte
// depths) t - i.  The unit above comes from lane i - 1's result of the step before by a cross-lane shift, the one above-left from the
// step before that; lane 0 reads the band above's last row, which lane 63 wrote back in place (agent-scope loads after a release
// fence: the bytes were stored in this launch).  Each unit is converted and written to the frame at once.
// An Adam7 file is seven such images (png_unfilter_kernel<true>): a wave per pass runs the same wavefront over the pass's own rows,
// from a zero row above, and its pixel (px, py) lands at (xo + px * xf, yo + py * yf) of the frame.  The waves of a file write
// neighbouring frame bytes, so every frame store is a whole store of its own bytes, never a read-modify-write.
__device__ inline uint32_t byte_of(uint32_t u0, uint32_t u1, int k) { return ((k < 4 ? u0 : u1) >> (8 * (k & 3))) & 0xFF; }

__device__ inline void unit_load(const uint8_t *p, int bpp, uint32_t &u0, uint32_t &u1)
{
    u0 = u1 = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (k < bpp) { if (k < 4) u0 |= (uint32_t)p[k] << (8 * k); else u1 |= (uint32_t)p[k] << (8 * (k - 4)); }
}

__device__ inline uint32_t load_above_byte(const uint8_t *p)
{
    const uintptr_t a = (uintptr_t)p;
    const uint32_t wd = __hip_atomic_load((const uint32_t *)(a & ~(uintptr_t)3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (wd >> (8 * (a & 3))) & 0xFF;
}

// the unit's pixels in the frame layout of the file's kind: unit ux of a row of pw pixels, into frame row r.  kAdam7: pixel px of that
// row is the frame's column ps.xo + px * ps.xf; otherwise the row is the frame's own (pw = d.w, ps unused).
template <bool kAdam7>
__device__ inline void emit(const PngDecDesc &d, uint8_t *fr, uint32_t r, uint32_t ux, uint32_t u0, uint32_t u1, uint32_t pw, const PngPass &ps)
{
    const uint32_t w = d.w;
    if (d.depth < 8) {
        const uint32_t dep = d.depth, ppb = 8 / dep, mask = (1u << dep) - 1, scale = d.ctype == 0 ? 255 / mask : 1;
        uint8_t *o = fr + (size_t)r * w;
        for (uint32_t j = 0; j < ppb; j++) {
            const uint32_t px = ux * ppb + j;
            if (px < pw) o[kAdam7 ? ps.xo + px * ps.xf : px] = (uint8_t)(((u0 >> (8 - dep * (j + 1))) & mask) * scale);
        }
        return;
    }
    const uint32_t x = kAdam7 ? ps.xo + ux * ps.xf : ux;
    const bool t = d.trns != 0;
    if (d.depth == 8) {
        switch (d.ctype) {
        case 0: {
            const uint32_t v = u0 & 0xFF;
            if (!t) fr[(size_t)r * w + x] = (uint8_t)v;
            else ((uint32_t *)(fr + (size_t)r * w * 4))[x] = v | v << 8 | v << 16 | (v == d.tv[0] ? 0u : 0xFFu) << 24;
            return;
        }
        case 2: {
            const bool m = t && (u0 & 0xFF) == d.tv[0] && ((u0 >> 8) & 0xFF) == d.tv[1] && ((u0 >> 16) & 0xFF) == d.tv[2];
            ((uint32_t *)(fr + (size_t)r * w * 4))[x] = (u0 & 0xFFFFFF) | (m ? 0u : 0xFFu) << 24;
            return;
        }
        case 3: fr[(size_t)r * w + x] = (uint8_t)u0; return;
        case 4: {
            const uint32_t v = u0 & 0xFF;
            ((uint32_t *)(fr + (size_t)r * w * 4))[x] = v | v << 8 | v << 16 | ((u0 >> 8) & 0xFF) << 24;
            return;
        }
        default: ((uint32_t *)(fr + (size_t)r * w * 4))[x] = u0; return;
        }
    }
    uint32_t *o = (uint32_t *)(fr + (size_t)r * w * (d.kind == IPX_PNG_GRAY16 ? 2 : 8));
    switch (d.ctype) {
    case 0: {
        const uint32_t y = u0 & 0xFFFF;                          // the two bytes as stored (big-endian)
        if (!t) { ((uint16_t *)o)[x] = (uint16_t)y; return; }
        const bool m = ((y & 0xFF) << 8 | y >> 8) == d.tv[0];
        o[2 * x] = y | y << 16;
        o[2 * x + 1] = y | (m ? 0u : 0xFFFFu) << 16;
        return;
    }
    case 2: {
        const bool m = t && (byte_of(u0, u1, 0) << 8 | byte_of(u0, u1, 1)) == d.tv[0] &&
                       (byte_of(u0, u1, 2) << 8 | byte_of(u0, u1, 3)) == d.tv[1] && (byte_of(u0, u1, 4) << 8 | byte_of(u0, u1, 5)) == d.tv[2];
        o[2 * x] = u0;
        o[2 * x + 1] = (u1 & 0xFFFF) | (m ? 0u : 0xFFFFu) << 16;
        return;
    }
    case 4: {
        const uint32_t y = u0 & 0xFFFF, a = u0 >> 16;
        o[2 * x] = y | y << 16;
        o[2 * x + 1] = y | a << 16;
        return;
    }
    default: o[2 * x] = u0; o[2 * x + 1] = u1; return;
    }
}

// kAdam7: a workgroup of one wave per (file, pass) runs the same wavefront over the pass's rows, which start behind those of the passes
// before it.  The passes of a file share nothing (each starts from a zero row above), so they run side by side; an empty pass has no
// bytes and its wave leaves at once.  Not kAdam7: the file's rows are the frame's; being a template, not a shared function, keeps that
// instantiation's instructions those of a kernel without the passes (the inliner's order otherwise changes its registers).
template <bool kAdam7>
__global__ __launch_bounds__(64) void png_unfilter_kernel(const PngDecDesc *__restrict__ desc, uint8_t *__restrict__ raw,
                                                          uint8_t *__restrict__ frames, uint32_t *__restrict__ status)
{
    const PngDecDesc d = desc[kAdam7 ? blockIdx.x / 7 : blockIdx.x];
    if (status[d.slot] & (kPngBadZlib | kPngBadCrc)) return;
    const int lane = threadIdx.x;
    uint8_t *base = raw + d.roff, *fr = frames + d.foff;
    const int bpp = d.bpp;
    uint32_t rb = d.rowbytes, h = d.h, pw = d.w;
    PngPass ps = PngPass{1, 1, 0, 0};
    if constexpr (kAdam7) {
        const uint32_t bits = d.depth < 8 ? d.depth : bpp * 8u;          // per pixel
        uint32_t off = 0;
        rb = h = 0;
        for (uint32_t k = 0; k <= blockIdx.x % 7; k++) {
            off += h * rb;                                               // (an empty pass: rb is 0)
            ps = png_pass((int)k);
            pw = png_pass_dim(d.w, ps.xo, ps.xf);
            h = png_pass_dim(d.h, ps.yo, ps.yf);
            rb = pw && h ? 1 + (bits * pw + 7) / 8 : 0;
        }
        if (rb == 0) return;
        base += off;
    }
    const uint32_t units = (rb - 1) / bpp;
    bool bad = false;
    for (uint32_t r0 = 0; r0 < h; r0 += 64) {
        const uint32_t r = r0 + lane;
        const bool act = r < h;
        uint8_t *row = base + (size_t)(act ? r : 0) * rb;
        uint32_t ft = act ? row[0] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        const uint8_t *above = r0 > 0 ? base + (size_t)(r0 - 1) * rb + 1 : nullptr;
        uint32_t c0 = 0, c1 = 0, up0 = 0, up1 = 0, ul0 = 0, ul1 = 0, f0, f1;
        for (uint32_t t = 0; t < units + 63; t++) {
            const int x = (int)t - lane;
            ul0 = up0;
            ul1 = up1;
            up0 = __shfl_up(c0, 1, 64);
            up1 = __shfl_up(c1, 1, 64);
            if (lane == 0) {
                up0 = up1 = 0;
                if (above && x < (int)units) {
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (k < bpp) {
                            const uint32_t v = load_above_byte(above + (size_t)x * bpp + k);
                            if (k < 4) up0 |= v << (8 * k); else up1 |= v << (8 * (k - 4));
                        }
                }
            }
            if (act && x >= 0 && x < (int)units) {
                uint8_t *fp = row + 1 + (size_t)x * bpp;
                unit_load(fp, bpp, f0, f1);
                uint32_t n0 = 0, n1 = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (k >= bpp) break;
                    const int f = (int)byte_of(f0, f1, k);
                    const int a = x > 0 ? (int)byte_of(c0, c1, k) : 0;
                    const int b = (int)byte_of(up0, up1, k);
                    const int c = x > 0 ? (int)byte_of(ul0, ul1, k) : 0;
                    int v;
                    switch (ft) {
                    case 1: v = f + a; break;
                    case 2: v = f + b; break;
                    case 3: v = f + ((a + b) >> 1); break;
                    case 4: v = f + paeth(a, b, c); break;
                    default: v = f; break;
                    }
                    v &= 0xFF;
                    if (k < 4) n0 |= (uint32_t)v << (8 * k); else n1 |= (uint32_t)v << (8 * (k - 4));
                    if (lane == 63) fp[k] = (uint8_t)v;
                }
                c0 = n0;
                c1 = n1;
                emit<kAdam7>(d, fr, kAdam7 ? ps.yo + r * ps.yf : r, (uint32_t)x, n0, n1, pw, ps);
            }
        }
        __threadfence();
        __syncthreads();
    }
    if (__any(bad) && lane == 0) atomicOr(status + d.slot, kPngBadFilter);
}

hipError_t launch_png_unfilter(const PngDecDesc *desc, int n, uint8_t *raw, uint8_t *frames, uint32_t *status, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_unfilter_kernel<false>, dim3(n), dim3(64), 0, s, desc, raw, frames, status);
    return hipGetLastError();
}

hipError_t launch_png_unfilter_adam7(const PngDecDesc *desc, int n, uint8_t *raw, uint8_t *frames, uint32_t *status, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_unfilter_kernel<true>, dim3(7 * (unsigned)n), dim3(64), 0, s, desc, raw, frames, status);
    return hipGetLastError();
}

}  // namespace ipx
