// ipx_jpeg_dec_scans.hip -- the scans of a progressive JPEG walked on the GPU (IPX_JPEG_PROG_GPU=1): one wave per file, the scans in
// file order.  The scan program (extents, parameters, table definitions) comes from the host's marker pre-pass (jpeg_prog_prepass in
// ipx_jpeg_dec_prog.cpp); the arithmetic is that of Decoder::scan / refine / refine_nonzeroes there, which restate Go's processSOS /
// refine / refineNonZeroes, branch by branch.  What leaves is what jpeg_host_decode leaves: a.coefs [file][block][64] int16 in natural
// order with element 0 zero, the DC terms in a.dcs -- both zeroed by the driver before the launch.
//
// Why a wave per file and not a lane per scan: a refinement scan reads one bit per coefficient that earlier scans made non-zero, so the
// scans of one band form a chain, and that chain holds nine tenths of a file's entropy bytes.  The parallelism is
// across the files of the batch; the wave's lanes do what is data-parallel inside a block (lane z owns zig-zag position z: the block's
// non-zero mask is one ballot, the corrections and new coefficients of a refinement are applied and stored by all lanes at once) and
// inside the staging of the input.
//
// Structure, as in png_inflate_kernel: control flow is wave-uniform; reader and scan state go through readfirstlane so they live in
// SGPRs; the scan's tables are copied to LDS by all lanes at the start of each scan; the input is staged into LDS 1 KiB at a time with
// 16-byte loads.  Unstuffing happens WHILE STAGING: inside a scan's readable bytes every 0xff is followed by a stuffed 0x00 (the host cut
// the extent at the first 0xff that is not), so a byte is dropped iff it is 0x00 behind 0xff; the lanes compact what is left with a prefix
// sum and the bit reader sees plain bytes.
//
// Termination.  The walk is three nested loops: scans (at most IPX_JPEG_PROG_MAX_SCANS, fixed by the host), blocks of a scan (fixed by
// the frame: the iterator only advances), and per block the symbol loop.  Every iteration of a symbol loop either takes at least one
// bit from the reader (huff() takes a code of at least one bit or fails) or ends the block; the correction loop of refine_nonzeroes
// takes min(popcount, 24) >= 1 bits per turn and clears as many positions.  The reader hands out no bit beyond the scan's readable
// bytes: refill() stops at `rend`, a demand it cannot meet sets the error, and the first error ends the file (the status is written, the
// wave leaves).  An EOB run is a counter that only the blocks of the frame decrement, so it is bounded by the blocks left; what remains
// of it at the last scan's end is dropped.  stage() advances rpos by a whole chunk each call, so the refill loop ends with the scan's
// bytes.  No store goes outside the file's nblk blocks: block indices come from the iterator alone, positions are 0 .. 63.
#include "ipx_internal.h"

namespace ipx {

namespace {

constexpr int kChunk = 1024;        // raw bytes staged per turn: 64 lanes x 16

__constant__ uint8_t c_unzig[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct ProgLds {
    JpegProgHuff tab[4];            // [0..2]: the DC tables of the scan's components; [3]: the AC table (a band scan has one component)
    uint8_t in[kChunk + 16];        // unstuffed bytes: up to 7 left over from the last chunk, then the chunk's
};

__device__ inline uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline int unii(int v) { return (int)__builtin_amdgcn_readfirstlane((uint32_t)v); }
__device__ inline uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }
__device__ inline uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

}  // namespace

__global__ __launch_bounds__(64) void jpeg_prog_kernel(const JpegProgArgs a)
{
    __shared__ __attribute__((aligned(16))) ProgLds S;
    const int lane = threadIdx.x;
    const JpegProgFile f = a.files[blockIdx.x];
    const uint8_t *file = a.blob + f.blob_off;
    int16_t *coefs = a.coefs + (size_t)f.img * a.nblk * 64;
    int16_t *dcs = a.dcs + (size_t)f.img * a.nblk;
    const int unz = c_unzig[lane];
    const uint64_t lanes_below = lane ? ~0ull >> (64 - lane) : 0;

    // ---- the reader: Bits of the host decoder over the unstuffed bytes in LDS ----
    uint64_t acc = 0;
    int n = 0;
    uint32_t upos = 0, ulen = 0;                 // S.in: the next byte, the bytes held
    uint32_t rstart = 0, rend = 0, rpos = 0;     // the scan's readable bytes within the file; the next chunk (16-byte aligned)
    uint32_t carry = 0;                          // the last raw byte of the chunk before
    int st = 0;                                  // the file's status once something ended it
    bool err = false, wide = false, ask_host = false;
    uint32_t eobrun = 0;                         // NOT reset at a scan boundary (Decoder::eobrun)

    auto stage = [&]() {
        const uint32_t left = ulen - upos;       // < 8
        uint8_t lb = 0;
        if ((uint32_t)lane < left) lb = S.in[upos + lane];
        __syncthreads();
        if ((uint32_t)lane < left) S.in[lane] = lb;
        const uint32_t g = rpos + 16 * lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g < rend) v = *(const uint4 *)(file + g);
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
        uint32_t prev = __shfl_up(v.w >> 24, 1, 64);
        if (lane == 0) prev = carry;
        uint32_t keep = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (wd[j >> 2] >> (8 * (j & 3))) & 0xff, idx = g + j;
            const bool in = idx >= rstart && idx < rend;
            const bool stuffed = b == 0 && prev == 0xff && idx > rstart;
            if (in && !stuffed) keep |= 1u << j;
            prev = b;
        }
        const uint32_t cnt = __popc(keep);
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        uint32_t o = left + incl - cnt;
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (keep >> j & 1) S.in[o++] = (uint8_t)(wd[j >> 2] >> (8 * (j & 3)));
        carry = uni(__shfl(v.w >> 24, 63, 64));
        ulen = left + uni(__shfl(incl, 63, 64));
        upos = 0;
        rpos += kChunk;
        __syncthreads();
    };
    // as many bits as the accumulator takes, if the scan still holds them
    auto refill = [&]() {
        while (ulen - upos < 8 && rpos < rend) stage();
        if (n <= 32 && ulen - upos >= 4) {
            const uint8_t *p = S.in + upos;
            acc = acc << 32 | uni((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]);
            n += 32; upos += 4;
        }
        while (n <= 56 && upos < ulen) { acc = acc << 8 | uni(S.in[upos]); upos++; n += 8; }
    };
    auto bits = [&](int k) -> uint32_t {         // 1 <= k <= 32
        if (n < k) { refill(); if (n < k) { err = true; return 0; } }
        n -= k;
        return (uint32_t)((acc >> n) & ((1ull << k) - 1));
    };
    auto huff = [&](const JpegProgHuff &h) -> int {
        if (n < 16) refill();
        if (n >= 9) {
            const uint32_t e = uni(h.look[(acc >> (n - 9)) & 511]);
            if (e) { n -= (int)(e >> 8); return (int)(e & 255); }
        }
        for (int l = 1; l <= 16; l++) {
            if (l > n) { err = true; return 0; }                           // the reader ran dry inside a code
            const int32_t code = (int32_t)((acc >> (n - l)) & ((1u << l) - 1));
            const int32_t mx = unii(h.maxcode[l]), mn = unii(h.mincode[l]);
            if (mx >= 0 && code <= mx && code >= mn) { n -= l; return (int)uni(h.vals[unii(h.valptr[l]) + code - mn]); }
        }
        err = true;                                                        // "bad Huffman code"
        return 0;
    };
    auto receive_extend = [&](int t) -> int32_t {
        if (!t) return 0;
        const int32_t x = (int32_t)bits(t);
        return x < (1 << (t - 1)) ? x + (int32_t)((uint32_t)-1 << t) + 1 : x;
    };
    auto block_index = [&](int k, int bx, int by) -> int {                 // Decoder::block_index
        const int sx = k == 0 ? a.h0 - 1 : 0, sy = k == 0 ? a.v0 - 1 : 0;
        return ((by >> sy) * a.mxx + (bx >> sx)) * a.bpm + (k == 0 ? ((by & sy) << sx) + (bx & sx) : a.ybl + k - 1);
    };

    for (uint32_t si = 0; si < f.nscans && !st; si++) {
        const JpegProgScan sc = a.scans[f.scan0 + si];
        const int ns = sc.ns, zs = sc.ss, ze = sc.se, ah = sc.ah, al = sc.al;
        // (packed, so that no slot is looked up through an index into private memory)
        const uint32_t comps = (uint32_t)sc.comp[0] | (uint32_t)sc.comp[1] << 8 | (uint32_t)sc.comp[2] << 16;
        const uint64_t dc_defs = (uint64_t)sc.dc_def[0] | (uint64_t)sc.dc_def[1] << 16 | (uint64_t)sc.dc_def[2] << 32;
        auto comp_of = [&](int slot) -> int { return (int)(comps >> (8 * slot) & 255); };
        __syncthreads();                         // the scan before is through with the tables, and its stores are ordered before this one's loads
        for (int i = 0; i < ns; i++) {
            const bool dc = zs == 0 && ah == 0, ac = zs > 0;
            if (dc || ac) {
                const uint4 *src = (const uint4 *)(a.defs + f.def0 + (dc ? (uint32_t)(dc_defs >> (16 * i) & 0xffff) : (uint32_t)sc.ac_def[0]));
                uint4 *dst = (uint4 *)&S.tab[dc ? i : 3];
                for (int e = lane; e < (int)(sizeof(JpegProgHuff) / 16); e += 64) dst[e] = src[e];
            }
        }
        acc = 0; n = 0; upos = ulen = 0; carry = 0;
        rstart = sc.off; rend = sc.off + sc.len; rpos = rstart & ~15u;
        __syncthreads();

        // the blocks of the scan in its order: a non-interleaved scan walks the component's own grid and leaves out the blocks outside
        // the image, an interleaved one walks MCUs
        const int k0 = sc.comp[0];
        const int q1 = a.mxx * (k0 == 0 ? a.h0 : 1), rows = a.myy * (k0 == 0 ? a.v0 : 1);
        const int vbx = min(q1, (a.w + 7) >> 3), vby = min(rows, (a.h + 7) >> 3);
        int bx = 0, by = 0, mx = 0, my = 0, ci = 0, cj = 0;
        auto next = [&](int *slot) -> int {      // -1: the scan is through
            if (ns == 1) {
                if (by >= vby) return -1;
                const int gb = block_index(k0, bx, by);
                if (++bx == vbx) { bx = 0; by++; }
                *slot = 0;
                return gb;
            }
            if (my >= a.myy) return -1;
            const int k = comp_of(ci), hi = k == 0 ? a.h0 : 1, vi = k == 0 ? a.v0 : 1;
            const int gb = block_index(k, hi * mx + (cj & (hi - 1)), vi * my + (hi == 2 ? cj >> 1 : cj));
            *slot = ci;
            if (++cj == hi * vi) { cj = 0; if (++ci == ns) { ci = 0; if (++mx == a.mxx) { mx = 0; my++; } } }
            return gb;
        };

        if (ah == 0 && zs == 0) {
            // ---- DC, first pass: a difference per block, the prediction per component wraps as uint32
            int32_t pred[3] = {0, 0, 0};
            int slot = 0;
            for (int gb = next(&slot); gb >= 0; gb = next(&slot)) {
                const int t = huff(S.tab[slot]);
                if (err) { st = IPX_ERR_INVALID; break; }
                if (t > 16) { st = IPX_ERR_UNSUPPORTED; break; }           // "excessive DC component"
                const int k = comp_of(slot);
                const int32_t d = receive_extend(t);
                const int32_t p = (int32_t)((uint32_t)(k == 0 ? pred[0] : k == 1 ? pred[1] : pred[2]) + (uint32_t)d);
                if (k == 0) pred[0] = p; else if (k == 1) pred[1] = p; else pred[2] = p;
                const int32_t v = (int32_t)((uint32_t)p << al);
                if (v != (int32_t)(int16_t)v) wide = true;
                if (lane == 0) dcs[gb] = (int16_t)v;
                if (err) { st = IPX_ERR_INVALID; break; }
            }
        } else if (ah == 0) {
            // ---- a band, first pass: the few coefficients of a block are plain stores
            int slot = 0;
            for (int gb = next(&slot); gb >= 0; gb = next(&slot)) {
                if (eobrun > 0) { eobrun--; continue; }
                for (int zig = zs; zig <= ze; zig++) {
                    const int value = huff(S.tab[3]);
                    if (err) break;
                    const int run = value >> 4, size = value & 15;
                    if (size) {
                        zig += run;
                        if (zig > ze) break;
                        const int32_t v = (int32_t)((uint32_t)receive_extend(size) << al);
                        if (err) break;
                        if (v != (int32_t)(int16_t)v) {
                            wide = true;
                            // the host's mask says non-zero where the coefficient now reads zero: its verdict is asked for (ipx_internal.h)
                            if ((int16_t)v == 0) { st = IPX_ERR_UNSUPPORTED; ask_host = true; break; }
                        }
                        if (lane == 0) coefs[(size_t)gb * 64 + c_unzig[zig]] = (int16_t)v;
                    } else {
                        if (run != 15) {
                            eobrun = 1u << run;
                            if (run) eobrun |= bits(run);
                            eobrun = (eobrun - 1) & 0xffff;
                            break;
                        }
                        zig += 15;
                    }
                }
                if (st) break;
                if (err) { st = IPX_ERR_INVALID; break; }
            }
        } else if (zs == 0) {
            // ---- DC, refinement: one bit per block; 64 blocks at a time, lane j takes the j-th
            const int32_t delta = 1 << al;
            bool more = true;
            while (more && !st) {
                int mine = -1, cnt = 0, slot = 0;
                for (; cnt < 64; cnt++) {
                    const int gb = next(&slot);
                    if (gb < 0) { more = false; break; }
                    if (lane == cnt) mine = gb;
                }
                if (!cnt) break;
                const int k1 = min(cnt, 32), k2 = cnt - k1;
                const uint32_t v1 = bits(k1), v2 = k2 ? bits(k2) : 0;
                if (err) { st = IPX_ERR_INVALID; break; }
                const uint32_t word = lane < 32 ? v1 : v2;
                const int sh = (lane < 32 ? k1 - 1 - lane : k2 - 1 - (lane - 32)) & 31;
                const bool set = mine >= 0 && (word >> sh & 1);
                // (an int16 OR-ed with 1 << al, al <= 14 in a refinement: always an int16, nothing to flag)
                if (set) dcs[mine] = (int16_t)(dcs[mine] | delta);
            }
        } else {
            // ---- a band, refinement: every block of the band is loaded, lane z holding zig-zag position z; the ballot of the non-zero
            // ones IS the block's mask.  The uniform walk collects which positions take a correction and where the new coefficients go,
            // the lanes apply them and store the block back.  The next block of the scan is loaded while this one is walked.
            const int32_t delta = 1 << al;
            const uint64_t band = (~0ull << zs) & (~0ull >> (63 - ze));
            int slot = 0;
            int gb = next(&slot);
            int16_t c = gb >= 0 ? coefs[(size_t)gb * 64 + unz] : (int16_t)0;
            while (gb >= 0) {
                const int nb = next(&slot);
                const int16_t cn = nb >= 0 ? coefs[(size_t)nb * 64 + unz] : (int16_t)0;
                const uint64_t m = ballot(c != 0);
                uint64_t corr = 0, newm = 0, newneg = 0;
                // refine_nonzeroes: a bit per non-zero coefficient of [zig, ze] up to where the nz-th zero has been passed (nz < 0: to the end)
                auto refine_nonzeroes = [&](int zig, int nz) -> int {
                    const uint64_t range = (~0ull << zig) & band;
                    int stop = ze + 1;
                    if (nz >= 0) {
                        uint64_t z = ~m & range;
                        for (; nz > 0 && z; nz--) z &= z - 1;
                        if (z) stop = __builtin_ctzll(z);
                    }
                    uint64_t todo = m & range & (stop >= 64 ? ~0ull : (1ull << stop) - 1);
                    while (todo) {
                        const int cnt = __popcll(todo), k = cnt < 24 ? cnt : 24;
                        const uint32_t v = bits(k);
                        if (err) return 0;
                        const int rank = __popcll(todo & lanes_below);
                        const bool mine = (todo >> lane & 1) && rank < k;
                        corr |= ballot(mine && (v >> (k - 1 - rank) & 1));
                        todo &= ~ballot(mine);
                    }
                    return stop;
                };
                if (eobrun > 0 && !(m & band)) eobrun--;                  // most blocks of a run: nothing to correct, nothing read
                else {
                    int zig = zs;
                    if (eobrun == 0) {
                        for (; zig <= ze; zig++) {
                            int z = 0;
                            const int value = huff(S.tab[3]);
                            if (err) break;
                            const int run = value >> 4, size = value & 15;
                            if (size == 0) {
                                if (run != 15) {
                                    eobrun = 1u << run;
                                    if (run) eobrun |= bits(run);
                                    break;
                                }
                            } else if (size == 1) {
                                z = bits(1) ? 1 : -1;
                            } else { err = true; break; }                   // "unexpected Huffman code"
                            if (err) break;
                            zig = refine_nonzeroes(zig, run);
                            if (err) break;
                            if (zig > ze) { err = true; break; }            // "too many coefficients"
                            if (z) { newm |= 1ull << zig; if (z < 0) newneg |= 1ull << zig; }
                        }
                    }
                    if (!err && eobrun > 0) {
                        eobrun--;
                        if (zig <= ze) (void)refine_nonzeroes(zig, -1);
                    }
                    if (err) { st = IPX_ERR_INVALID; break; }
                    if (corr | newm) {
                        int32_t v = c;
                        if (corr >> lane & 1) v += c < 0 ? -delta : delta;
                        if (newm >> lane & 1) v = newneg >> lane & 1 ? -delta : delta;
                        if (ballot(v != (int32_t)(int16_t)v)) wide = true;
                        if ((corr | newm) >> lane & 1) coefs[(size_t)gb * 64 + unz] = (int16_t)v;
                    }
                }
                gb = nb; c = cn;
            }
        }
    }
    if (!st && wide) st = IPX_ERR_UNSUPPORTED;                             // Go keeps int32; the pipeline holds int16
    if (st && lane == 0)
        a.status[f.img] = jpeg_status_key(ask_host ? kJpegProgHostVerdict : 0, st);
}

int jpeg_prog_lds_bytes() { return (int)sizeof(ProgLds); }

hipError_t launch_jpeg_prog(const JpegProgArgs &a, hipStream_t s)
{
    if (a.nfiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(jpeg_prog_kernel, dim3(a.nfiles), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ipx
