// ipx_gif_dec_par.hip -- the code walk taken under IPX_GIF_PAR=1 (ipx_gif_dec.hip reads the switch): gif_walk_par_kernel, one wave per
// file as gif_walk_kernel, but all 64 lanes read codes.  Between two clear codes the reader's code width depends only on how many codes
// it has read since the clear, so the code at ordinal t of a segment sits at a bit offset that is a closed form of t and the literal
// width: 64 lanes read 64 consecutive codes, one ballot finds the first that ends the run (a clear code, the EOF code, the end of the
// data, a broken rule), the lanes before it resolve their strings' lengths and first bytes -- against LDS for ordinals of earlier
// rounds, by pointer jumping inside the round -- and a prefix sum of the lengths gives the output offsets.  The records are those of
// gif_walk_kernel, byte for byte.  This kernel decides no error: it accepts a file only at an EOF code that meets the serial walk's
// own rule, and hands everything else to gif_walk_kernel by the file's redo word.  DESIGN.md section 4.8; model: tests/gif_par_model.py.
#include "ipx_gif_dec.h"

namespace ipx {

namespace {

constexpr int kParWin = 4096;                  // bytes of LZW data staged in LDS at a time (a multiple of 4), plus 8 for the last read
constexpr uint32_t kParRound = 64 * 12 / 8;    // bytes a round's 64 codes span at most, less the partial byte in front
enum : uint32_t { kCont = 0, kClear = 1, kEof = 2, kEnd = 3, kBad = 4 };

__device__ inline uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// the width the reader has at ordinal t: hi = eof + t there, and the width is hi's bit length until it stays at 12
__device__ inline uint32_t par_width(uint32_t t, uint32_t eof)
{
    return min(12u, 32u - (uint32_t)__clz(eof + t));
}

// the bits of the ordinals before t.  Width lit + 1 serves the first clear - 1 ordinals, a width x above it the 1 << (x - 1) ordinals
// from (1 << (x - 1)) - eof on, width 12 every one from 2048 - eof on; with G(b) = sum of x << (x - 1) over x <= b = ((b - 1) << b) + 1.
__device__ inline uint64_t par_bits_before(uint32_t t, uint32_t lit)
{
    const uint32_t clear = 1u << lit, eof = clear + 1, w = par_width(t, eof);
    if (w == lit + 1) return (uint64_t)w * t;
    const uint32_t below = (lit + 1) * (clear - 1) + (((w - 2) << (w - 1)) + 1) - ((lit << (lit + 1)) + 1);
    return below + (uint64_t)w * (t - ((1u << (w - 1)) - eof));
}

}  // namespace

__global__ __launch_bounds__(64) void gif_walk_par_kernel(const uint8_t *__restrict__ blob, const GifDecDesc *__restrict__ desc,
                                                          GifCode *__restrict__ codes, uint32_t *__restrict__ state)
{
    __shared__ uint16_t s_len[4096];           // by ordinal of the segment: the length and first byte of the code's string
    __shared__ uint8_t s_first[4096];
    __shared__ uint32_t s_buf[kParWin / 4 + 2];
    const int lane = threadIdx.x;
    const GifDecDesc d = desc[blockIdx.x];
    const uint32_t *src = (const uint32_t *)(blob + d.data_off);      // 16-byte aligned, and padded to 16 bytes by the host
    GifCode *rec = codes + d.code_off;
    const uint32_t lit = d.lit, clear = 1u << lit, eof = clear + 1, npix = d.w * d.h;
    const uint64_t nbits = 8ull * d.data_len;
    const uint32_t nwords = (d.data_len + 3) >> 2;
    const uint32_t keep = 4095 - eof;          // ordinals below it can still be referenced: the entry eof + j reads ordinal j - 1
    // the walk's state, the same in every lane
    uint64_t bit0 = 0;                         // where the segment's first code starts
    uint32_t t0 = 0, k = 0, segb = 0, count = 0, prev_v = 0, base = 0;
    bool staged = false, accepted = false;
    // every round takes a code or ends the walk, and a code has at least lit + 1 bits
    const uint64_t max_rounds = nbits / (lit + 1) + 2;
    for (uint64_t round = 0; round < max_rounds; round++) {
        const uint32_t fb = (uint32_t)((bit0 + par_bits_before(t0, lit)) >> 3);      // <= data_len: every code so far fitted
        if (!staged || fb - base > (uint32_t)kParWin - kParRound) {
            base = fb & ~3u;
            staged = true;
            __syncthreads();
            for (int i = lane; i < kParWin / 4 + 2; i += 64) s_buf[i] = base / 4 + i < nwords ? src[base / 4 + i] : 0;
            __syncthreads();
        }
        // 1, 2: this lane's code
        const uint32_t t = t0 + lane, w = par_width(t, eof);
        const uint64_t pos = bit0 + par_bits_before(t, lit);
        const uint32_t o = (uint32_t)(pos >> 3) - base;                              // <= kParWin: both words are staged
        const uint64_t two = s_buf[o >> 2] | (uint64_t)s_buf[(o >> 2) + 1] << 32;
        const uint32_t v = (uint32_t)(two >> (8 * (o & 3) + (uint32_t)(pos & 7))) & ((1u << w) - 1);
        const bool frozen = eof + t > 4095;                                          // the table is full: no entry is added
        // 3: the first lane that ends the run; the lanes behind it hold garbage
        uint32_t kind = kCont;
        if (pos + w > nbits) kind = kEnd;
        else if (v == clear) kind = kClear;
        else if (v == eof) kind = kEof;
        else if (v < clear ? v >= d.pal_len : (!frozen && v - eof > t)) kind = kBad;
        const uint64_t stops = __ballot(kind != kCont);
        const int nvalid = stops ? __ffsll((unsigned long long)stops) - 1 : 64;
        const uint32_t stop = nvalid < 64 ? uni(__shfl(kind, nvalid, 64)) : kCont;
        const bool valid = lane < nvalid;
        // 4: L[t] = L[j - 1] + 1 and first[t] = first[j - 1] for a code eof + j (j <= t, KwKwK included); a literal is its own string
        uint32_t L = valid ? 1 : 0, F = v & 255;
        int ptr = lane;                                                              // ptr == lane: resolved
        if (valid && v > eof) {
            const uint32_t dep = v - eof - 1;
            if (dep < t0) { L = s_len[dep] + 1u; F = s_first[dep]; }
            else ptr = (int)(dep - t0);                                              // < lane; L is what to add to that lane's length
        }
        for (int s = 0; s < 6 && __ballot(ptr != lane); s++) {
            const uint32_t pl = __shfl(L, ptr, 64), pf = __shfl(F, ptr, 64);
            const int pp = __shfl(ptr, ptr, 64);
            if (ptr != lane) {
                L += pl;
                if (pp == ptr) { F = pf; ptr = lane; }
                else ptr = pp;
            }
        }
        // 5: offsets
        uint32_t incl = L;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(incl, off, 64);
            if (lane >= off) incl += u;
        }
        const uint32_t total = uni(__shfl(incl, 63, 64));
        // a string past the frame, the scratch exhausted (or a chain unresolved: cannot happen): the serial walk's
        if (__ballot(valid && (incl > npix - count || ptr != lane)) || (nvalid && k + nvalid >= d.code_cap)) break;
        // 6, 7: the table's lengths and first bytes, the records
        const uint32_t up = __shfl_up(v, 1, 64);
        if (valid) {
            if (t < keep) { s_len[t] = (uint16_t)L; s_first[t] = (uint8_t)F; }
            const uint32_t prev = t == 0 || frozen ? 0u : lane == 0 ? prev_v : up;
            rec[k + lane] = GifCode{count + incl - L, segb, v | prev << 12 | F << 24};
        }
        __syncthreads();
        if (nvalid) prev_v = uni(__shfl(v, nvalid - 1, 64));
        count += total;
        k += nvalid;
        t0 += nvalid;
        if (stop == kCont) continue;
        const uint64_t end_bit = bit0 + par_bits_before(t0, lit) + par_width(t0, eof);   // behind the code that ended the run
        if (stop == kClear) {
            bit0 = end_bit;
            t0 = 0;
            segb = k;
            continue;
        }
        if (stop == kEof) {                     // gif_walk_kernel's rule at the EOF code
            const uint64_t used = (end_bit + 7) >> 3;
            const bool close_ok = (d.flags & kGifTerminated) &&
                                  (used > d.last_start || (used == d.last_start && (d.flags & kGifLastIsOne)));
            accepted = count == npix && close_ok;
        }
        break;
    }
    if (lane == 0) {
        uint32_t *st = state + kGifStateWords * d.slot;
        if (accepted) rec[k].off = count;       // the closing offset (k < code_cap)
        st[0] = accepted ? 0 : 1;               // (a file left to the serial walk: that walk writes its own)
        st[1] = accepted ? k : 0;
        st[2] = accepted ? 0 : 1;
        st[3] = accepted ? k : 0;
    }
}

hipError_t launch_gif_walk_par(const uint8_t *blob, const GifDecDesc *desc, int n, GifCode *codes, uint32_t *state, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_walk_par_kernel, dim3(n), dim3(64), 0, s, blob, desc, codes, state);
    return hipGetLastError();
}

}  // namespace ipx
