// ipx_png_dec_par.hip -- the two inflate kernels taken under IPX_PNG_PAR=1 (ipx_png_dec_runtime.hip reads the switch).  png_inflate_par_kernel: the
// inflate of ipx_png_inflate.h with a Huffman block's body parsed by the 64 lanes side by side.  One workgroup of one wave per file; the
// zlib header, the block headers, stored blocks, the tables, the staging, the flushes and the end of the stream are that header's
// wave-uniform code, the serial kernel's steps.  png_inflate_redo_kernel, at the end: the serial walk for the files the first one leaves.
//
// A window of the staged bits behind the block's next token is cut into 64 sub-sequences of `sub` bits.  Lane k decodes from its
// boundary as if a literal/length code began there, up to the first token that starts at or past the next boundary, and keeps that
// exit.  Then rounds: lane k restarts from lane k - 1's exit; a lane whose start did not change is in step; the rounds end when no
// lane changed (lane 0's start is the true one and every round fixes at least one more lane, so at most 64 rounds).  A lane that meets
// the end-of-block symbol, a code outside the alphabet or the stream's end keeps that as its state, and the lanes behind it are dead.
// In step, every lane knows its tokens, bytes and matches; prefix sums give its output offset and its place in the match list.  The
// lanes up to the first end-of-block whose bytes together fit one flush unit are taken: they decode once more, writing their
// literals to the window and their matches to a list in LDS, and the matches are then copied one after the other by all 64 lanes.  The
// window of the next round starts behind the last lane taken.  When lane 0's stretch alone exceeds the unit, the serial token loop
// decodes that stretch.
//
// The ring is 64 KiB here, not 32: a round writes its literals before its matches, so up to one unit of literals lies ahead of a
// match that may still read 32 KiB back, and less than one unit waits behind for the flush.
//
// The kernel decides no error.  Whatever breaks a rule -- on the chain in step, at the end of the stream, the Adler-32, trailing
// bytes -- sets the file's redo bit; the wave writes no status and leaves, and png_inflate_redo_kernel decodes the file from scratch
// behind it.  DESIGN.md section 4.10; tests/png_par_model.py is the model.
#include "ipx_png_dec.h"
#include "ipx_png_inflate.h"

namespace ipx {

using namespace flate;

namespace {
constexpr int kParWin = 65536;
constexpr int kParMatches = kFlush / 3 + 1;     // a match is at least 3 bytes and a round at most kFlush
enum : uint32_t { kLaneCont = 0, kLaneEob = 1, kLaneErr = 2, kLaneDead = 3 };

// huff_decode for one lane's own bits (no readfirstlane)
__device__ inline int huff_decode_lane(uint32_t bits, const uint16_t *root, int rbits, const HuffLds &h, const uint16_t *sorted, uint32_t *len)
{
    const uint32_t e = root[bits & ((1u << rbits) - 1)];
    if (e) { *len = e & 15; return (int)(e >> 4); }
    const uint32_t rev = __brev(bits & 0x7FFF) >> 17;
    for (int L = rbits + 1; L <= 15; L++) {
        const uint32_t k = (rev >> (15 - L)) - h.first[L];
        if (k < h.count[L]) { *len = (uint32_t)L; return (int)sorted[h.offset[L] + k]; }
    }
    *len = 0;
    return -1;
}

__device__ inline uint32_t scan_incl(uint32_t v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    return v;
}
}  // namespace

__global__ __launch_bounds__(64) void png_inflate_par_kernel(const uint8_t *__restrict__ zlib, const PngDecDesc *__restrict__ desc,
                                                             uint8_t *__restrict__ raw, const uint32_t *__restrict__ status,
                                                             uint32_t *__restrict__ par, uint32_t sub)
{
    __shared__ InflateLds<kParWin> S;
    __shared__ uint32_t s_mld[kParMatches];     // a round's matches in stream order: length << 16 | distance - 1
    __shared__ uint16_t s_mdst[kParMatches];    // and where each starts, in bytes behind the round's first
    const int lane = threadIdx.x;
    const PngDecDesc d = desc[blockIdx.x];
    uint32_t *words = par + 2 * (size_t)d.slot;
    if (status[d.slot] & kPngBadCrc) {
        if (lane == 0) words[1] = kPngParRedo;
        return;
    }
    Inflater<kParWin> I(S, lane, d, zlib, raw);
    uint32_t tok_lanes = 0, tok_uniform = 0;

    // One lane's stretch: the tokens from bit p (relative to the staged block) that start before lim.  emit: the literals go to the
    // window from byte ob on and the matches to the list from entry mb on (r0: the round's first byte).
    uint32_t zrel = 0;
    auto run = [&](uint32_t p, uint32_t lim, bool emit, uint32_t ob, uint32_t mb, uint32_t r0, uint32_t &ex, uint32_t &st, uint32_t &nt,
                   uint32_t &nby, uint32_t &nm) {
        nt = nby = nm = 0;
        st = kLaneCont;
        while (p < lim) {
            const uint32_t *w = (const uint32_t *)S.in + (p >> 5);
            const uint32_t sh = p & 31;
            uint64_t bits = ((uint64_t)w[1] << 32 | w[0]) >> sh;
            if (sh) bits |= (uint64_t)w[2] << (64 - sh);
            uint32_t L;
            const int sym = huff_decode_lane((uint32_t)bits, S.lit_root, kLitRoot, S.lit, S.lit_sorted, &L);
            if (sym < 0 || sym > 285) { st = kLaneErr; break; }
            uint32_t used = L;
            if (sym < 256) {
                if (emit) S.win[ob & (kParWin - 1)] = (uint8_t)sym;
                ob++;
                nby++;
            } else if (sym == 256) {
                p += used;
                nt++;
                st = p > zrel ? kLaneErr : kLaneEob;
                break;
            } else {
                const int li = sym - 257;
                const uint32_t le = c_flate.len_extra[li];
                const uint32_t len = c_flate.len_base[li] + ((uint32_t)(bits >> used) & ((1u << le) - 1));
                used += le;
                const int ds = huff_decode_lane((uint32_t)(bits >> used), S.dist_root, kDistRoot, S.dist, S.dist_sorted, &L);
                if (ds < 0 || ds >= 30) { st = kLaneErr; break; }
                used += L;
                const uint32_t de = c_flate.dist_extra[ds];
                const uint32_t dist = c_flate.dist_base[ds] + ((uint32_t)(bits >> used) & ((1u << de) - 1));
                used += de;
                if (emit) {
                    s_mld[mb] = len << 16 | (dist - 1);
                    s_mdst[mb] = (uint16_t)(ob - r0);
                }
                mb++;
                nm++;
                ob += len;
                nby += len;
            }
            p += used;
            nt++;
            if (p > zrel) { st = kLaneErr; break; }
        }
        ex = p;
    };

    I.zlib_header();
    while (!I.err && !I.final_block) {
        if (!I.block_head()) continue;
        uint64_t P = I.bit_at();                                 // the next token of the block, in stream bits
        for (;;) {
            if (P > I.zbits) { I.err = true; break; }
            const uint32_t pb = (uint32_t)(P >> 3);
            if (pb < I.in_base || pb - I.in_base + 8 * sub + 32 > (uint32_t)kInBytes) I.stage(pb);
            const uint64_t base = 8ull * I.in_base;
            const uint32_t p0 = (uint32_t)(P - base);
            zrel = (uint32_t)min(I.zbits - base, (uint64_t)0x7FFFFFFF);
            const uint32_t lim = p0 + (lane + 1) * sub;
            uint32_t start = p0 + lane * sub, ex, st, nt, nby, nm;
            run(start, lim, false, 0, 0, 0, ex, st, nt, nby, nm);
            for (;;) {                                           // rounds to the fixed point
                const uint32_t pe = __shfl_up(ex, 1, 64), ps = __shfl_up(st, 1, 64);
                const uint32_t ns = lane == 0 ? start : ps == kLaneCont ? pe : ~0u;
                const bool changed = ns != start;
                if (!__any(changed)) break;
                if (changed) {
                    start = ns;
                    if (ns == ~0u) {
                        st = kLaneDead;
                        nt = nby = nm = 0;
                        ex = ~0u;
                    } else {
                        run(start, lim, false, 0, 0, 0, ex, st, nt, nby, nm);
                    }
                }
            }
            const uint64_t stopped = __ballot(st != kLaneCont);
            const int last_valid = stopped ? __ffsll((long long)stopped) - 1 : 63;
            if (__shfl(st, last_valid, 64) == kLaneErr) { I.err = true; break; }
            const bool valid = lane <= last_valid;
            const uint32_t by_incl = scan_incl(valid ? nby : 0, lane), m_incl = scan_incl(valid ? nm : 0, lane),
                           t_incl = scan_incl(valid ? nt : 0, lane);
            const int taken = __popcll(__ballot(valid && by_incl <= (uint32_t)kFlush));
            if (taken == 0) {                                    // lane 0's stretch alone exceeds the unit: the serial loop takes it
                I.seek(P);
                const bool eob = I.tokens<true>(base + p0 + sub, &tok_uniform);
                P = I.bit_at();
                if (I.err || eob) break;
                continue;
            }
            const uint32_t total = __shfl(by_incl, taken - 1, 64), nmatch = __shfl(m_incl, taken - 1, 64);
            if ((uint64_t)I.pos + total > I.raw_len) { I.err = true; break; }
            const uint32_t r0 = I.pos;
            if (lane < taken) {
                uint32_t e2, s2, t2, b2, m2;
                run(start, lim, true, r0 + by_incl - nby, m_incl - nm, r0, e2, s2, t2, b2, m2);
            }
            __syncthreads();
            for (uint32_t i = 0; i < nmatch; i++) {
                const uint32_t ld = uni(s_mld[i]), pos = r0 + uni(s_mdst[i]);
                const uint32_t len = ld >> 16, dist = (ld & 0xFFFF) + 1;
                if (dist > pos) { I.err = true; break; }
                const uint32_t from = pos - dist;
                for (uint32_t j = lane; j < len; j += 64)
                    S.win[(pos + j) & (kParWin - 1)] = S.win[(from + (dist >= len ? j : j % dist)) & (kParWin - 1)];
                __syncthreads();
            }
            if (I.err) break;
            I.pos = r0 + total;
            tok_lanes += __shfl(t_incl, taken - 1, 64);
            P = base + __shfl(ex, taken - 1, 64);
            const bool eob = __shfl(st, taken - 1, 64) == kLaneEob;
            __syncthreads();
            I.flush_units();
            if (eob) break;
        }
        if (!I.err) {
            if (P > I.zbits) I.err = true;
            else I.seek(P);
        }
    }
    bool trailing;
    const bool ok = I.finish(&trailing) && !trailing;
    if (lane == 0) {
        words[0] = ok ? tok_lanes : 0;
        words[1] = ok ? tok_uniform : kPngParRedo;
    }
}

// The serial decoder behind it, over the same descriptors: the files whose redo bit is set are decoded from scratch, one serial walk
// of every block's tokens, and get their status here; for every other file the wave leaves at once.
__global__ __launch_bounds__(64) void png_inflate_redo_kernel(const uint8_t *__restrict__ zlib, const PngDecDesc *__restrict__ desc,
                                                              uint8_t *__restrict__ raw, uint32_t *__restrict__ status,
                                                              const uint32_t *__restrict__ par)
{
    __shared__ InflateLds<kWinBytes> S;
    const int lane = threadIdx.x;
    const PngDecDesc d = desc[blockIdx.x];
    if (!(par[2 * (size_t)d.slot + 1] & kPngParRedo)) return;
    if (status[d.slot] & kPngBadCrc) return;
    Inflater<kWinBytes> I(S, lane, d, zlib, raw);
    I.zlib_header();
    while (!I.err && !I.final_block)
        if (I.block_head()) I.tokens<false>(0, nullptr);
    bool trailing;
    const bool ok = I.finish(&trailing);
    if (lane == 0 && (!ok || trailing)) atomicOr(status + d.slot, !ok ? kPngBadZlib : kPngTrailing);
}

hipError_t launch_png_inflate_redo(const uint8_t *zlib, const PngDecDesc *desc, int n, uint8_t *raw, uint32_t *status, const uint32_t *par,
                                   hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_inflate_redo_kernel, dim3(n), dim3(64), 0, s, zlib, desc, raw, status, par);
    return hipGetLastError();
}

hipError_t launch_png_inflate_par(const uint8_t *zlib, const PngDecDesc *desc, int n, uint8_t *raw, const uint32_t *status, uint32_t *par,
                                  uint32_t sub, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_inflate_par_kernel, dim3(n), dim3(64), 0, s, zlib, desc, raw, status, par, sub);
    return hipGetLastError();
}

}  // namespace ipx
