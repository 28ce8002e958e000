// ipx_png_kernels.h -- the device half of png.Encode that does not care how the frames of a launch are laid out: the filter of one row,
// the helpers of the deflate of one segment (its statements: ipx_png_deflate_body.inc), the Adler-32 chunk and IEND of one frame.  The uniform kernels (ipx_png.hip: n frames of one size, found
// by arithmetic) and the mixed-size kernels (ipx_png_mixed.hip: frames of any sizes, found through a per-frame table) call the same
// bodies, so a frame's stream is the same bytes on both.  Device code only; each translation unit that includes this keeps its own
// copy of the tables in constant memory.  DESIGN.md section 4.9.
#pragma once

#include "ipx_png.h"

namespace ipx {

// ---- tables ----------------------------------------------------------------------------------------------------------------------
struct PngTables {
    uint8_t len_sym[kPngMaxMatch + 1];   // match length -> length symbol - 257
    uint16_t len_base[29];
    uint8_t len_extra[29];
    uint16_t dist_base[30];
    constexpr PngTables() : len_sym{}, len_base{}, len_extra{}, dist_base{}
    {
        const int lb[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        for (int s = 0; s < 29; s++) {
            len_base[s] = (uint16_t)lb[s];
            len_extra[s] = (uint8_t)(s < 8 || s == 28 ? 0 : (s - 4) / 4);
            for (int l = lb[s]; l <= kPngMaxMatch; l++) len_sym[l] = (uint8_t)s;
        }
        len_sym[258] = 28;
        for (int s = 0; s < 30; s++) dist_base[s] = (uint16_t)(s < 4 ? s + 1 : (1 << ((s >> 1) - 1)) * (2 + (s & 1)) + 1);
    }
};
static __constant__ PngTables c_png = PngTables();
static __constant__ PngCrcTables c_png_crc = PngCrcTables();

__device__ inline uint32_t png_hash(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return (v * kPngHashMul) >> (32 - kPngHashBits);
}

// ---- un-premultiply and filter ---------------------------------------------------------------------------------------------------
// byte k of a raw row as the writer builds it: RGB of an opaque frame, else the fast path's un-premultiplied RGBA
__device__ inline int raw_byte(const uint8_t *row, int k, int bpp)
{
    if (bpp == 3) {
        const int x = k / 3;
        return row[4 * x + (k - 3 * x)];
    }
    const uint8_t *p = row + 4 * (k >> 2);
    const int c = k & 3;
    const uint32_t a = p[3];
    if (c == 3 || a == 0xFF) return p[c];
    if (a == 0) return 0;
    return (int)(((uint32_t)p[c] * 0x101u * 0xFFFFu / (a * 0x101u)) >> 8) & 0xFF;
}

__device__ inline int abs8(int d) { return d < 128 ? d : 256 - d; }

// the five filtered bytes of position k (filter types 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth)
__device__ inline void filter5(const uint8_t *row, const uint8_t *prev, int k, int bpp, int f[5])
{
    const int x = raw_byte(row, k, bpp);
    const int b = prev ? raw_byte(prev, k, bpp) : 0;
    const int a = k >= bpp ? raw_byte(row, k - bpp, bpp) : 0;
    const int c = k >= bpp && prev ? raw_byte(prev, k - bpp, bpp) : 0;
    f[0] = x;
    f[1] = (x - a) & 0xFF;
    f[2] = (x - b) & 0xFF;
    f[3] = (x - ((a + b) >> 1)) & 0xFF;
    f[4] = (x - paeth(a, b, c)) & 0xFF;
}

// A workgroup's row: the filter type Go's heuristic picks and the rb filtered bytes of `row` (prev: the row above, or null) -> out[0],
// out[1 ..].  Every lane of the workgroup calls it.
__device__ __forceinline__ void png_filter_row(const uint8_t *row, const uint8_t *prev, int rb, int bpp, uint8_t *out)
{
    __shared__ int part[5][4];
    const int t = threadIdx.x;
    int sum[5] = {0, 0, 0, 0, 0}, v[5];
    for (int k = t; k < rb; k += blockDim.x) {
        filter5(row, prev, k, bpp, v);
        for (int q = 0; q < 5; q++) sum[q] += abs8(v[q]);
    }
    for (int q = 0; q < 5; q++) {
        for (int o = 32; o > 0; o >>= 1) sum[q] += __shfl_xor(sum[q], o, 64);
        if ((t & 63) == 0) part[q][t >> 6] = sum[q];
    }
    __syncthreads();
    // Up, Paeth, None, Sub, Average: the first strict minimum
    const int order[5] = {2, 4, 0, 1, 3};
    int best = -1, type = 2;
    for (int q = 0; q < 5; q++) {
        const int ty = order[q];
        int s = 0;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); wv++) s += part[ty][wv];
        if (best < 0 || s < best) { best = s; type = ty; }
    }
    if (t == 0) out[0] = (uint8_t)type;
    for (int k = t; k < rb; k += blockDim.x) {
        filter5(row, prev, k, bpp, v);
        out[1 + k] = (uint8_t)v[type];
    }
}

// ---- deflate of one segment ------------------------------------------------------------------------------------------------------
constexpr int kDefThreads = 256;   // == kPngTile: one position per lane per tile
static_assert(kDefThreads == kPngTile, "one lane per tile position");
constexpr int kHashSize = 1 << kPngHashBits;
constexpr int kWalkWin = 8192;

typedef unsigned long long u64_unaligned __attribute__((aligned(1)));
// equal bytes a[k] == b[k] for k < cap: 8 at a time while 8 fit below cap (nothing past a + cap is read), then one at a time
__device__ inline int match_len(const uint8_t *a, const uint8_t *b, int cap)
{
    int k = 0;
    for (; k + 8 <= cap; k += 8) {
        const unsigned long long x = *(const u64_unaligned *)(a + k) ^ *(const u64_unaligned *)(b + k);
        if (x) return k + (__ffsll((long long)x) - 1) / 8;
    }
    while (k < cap && a[k] == b[k]) k++;
    return k;
}

// LSB-first bits of v (n <= 48) at bit position pos of the word array; the words were zeroed, only non-zero words are touched
__device__ inline void put_bits(uint32_t *words, unsigned long long pos, unsigned long long v, int n)
{
    if (n == 0 || v == 0) return;
    uint32_t *w = words + (pos >> 5);
    const int sh = (int)(pos & 31);
    const unsigned long long lo = v << sh;
    const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
    if ((uint32_t)lo) atomicOr(w, (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(w + 1, (uint32_t)(lo >> 32));
    if (hi) atomicOr(w + 2, hi);
}

// the block-wide Huffman build (every lane calls it): code lengths of nsym symbols limited to `limit`, as huffman_lengths() of the
// model.  freq: LDS, may be changed (symbols forced to 1); len: LDS out; work: LDS scratch of >= 5 * 2 * nsym words
__device__ void huff_build(uint32_t *freq, int nsym, int limit, uint8_t *len, uint32_t *work)
{
    uint32_t *sorted = work, *weight = work + nsym, *parent = weight + 2 * nsym, *bits = parent + 2 * nsym;
    __shared__ int s_m;
    const int t = threadIdx.x;
    __syncthreads();
    if (t == 0) {
        int used = 0;
        for (int s = 0; s < nsym; s++) used += freq[s] != 0;
        for (int s = 0; used < 2; s++)
            if (freq[s] == 0) { freq[s] = 1; used++; }
        s_m = used;
    }
    __syncthreads();
    const int m = s_m;
    for (int s = t; s < nsym; s += blockDim.x) {
        len[s] = 0;
        if (!freq[s]) continue;
        int r = 0;
        const uint32_t fs = freq[s];
        for (int q = 0; q < nsym; q++) r += freq[q] && (freq[q] < fs || (freq[q] == fs && q < s));
        sorted[r] = s;
    }
    __syncthreads();
    if (t == 0) {
        for (int i = 0; i < m; i++) weight[i] = freq[sorted[i]];
        int li = 0, qi = 0;
        for (int node = m; node < 2 * m - 1; node++) {
            int kid[2];
            for (int k = 0; k < 2; k++) {
                if (li < m && (qi >= node - m || weight[li] <= weight[m + qi])) kid[k] = li++;
                else kid[k] = m + qi++;
            }
            weight[node] = weight[kid[0]] + weight[kid[1]];
            parent[kid[0]] = parent[kid[1]] = node;
        }
        // depths (reuse weight): the root is node 2m - 2
        weight[2 * m - 2] = 0;
        const int nb = 2 * m + limit + 1;
        for (int i = 0; i < nb; i++) bits[i] = 0;
        for (int node = 2 * m - 3; node >= 0; node--) weight[node] = weight[parent[node]] + 1;
        for (int leaf = 0; leaf < m; leaf++) bits[weight[leaf]]++;
        for (int i = nb - 1; i > limit; i--)
            while (bits[i] > 0) {
                int j = i - 2;
                while (bits[j] == 0) j--;
                bits[i] -= 2;
                bits[i - 1] += 1;
                bits[j + 1] += 2;
                bits[j] -= 1;
            }
        int at = m - 1;
        for (int l = 1; l <= limit; l++)
            for (uint32_t k = 0; k < bits[l]; k++) len[sorted[at--]] = (uint8_t)l;
    }
    __syncthreads();
}

// canonical codes (bit-reversed) of lengths len[0..nsym) into code[]; one lane
__device__ void huff_codes(const uint8_t *len, int nsym, uint16_t *code)
{
    uint32_t count[16] = {0}, next[16];
    for (int s = 0; s < nsym; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; b++) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < nsym; s++)
        if (len[s]) code[s] = (uint16_t)(__brev(next[len[s]]++) >> (32 - len[s]));
}

__device__ inline int dist_sym(int dist)
{
    const int d = dist - 1;
    if (d < 4) return d;
    const int nb = 31 - __clz(d);
    return 2 * nb + ((d >> (nb - 1)) & 1);
}

struct DefShared {
    uint32_t lfreq[286], dfreq[30], cfreq[19];
    uint8_t llen[286], dlen[30], clen[19];
    uint16_t lcode[286], dcode[30], ccode[19];
    uint16_t cl_sym[286 + 30];          // the code-length symbols: symbol | extra << 5
    uint32_t work[5 * 2 * 286 + 32];
    unsigned long long wsum[kDefThreads / 64], wsum2[kDefThreads / 64];
    int ncl, hlit, hdist, hclen, ntok, p;
    unsigned long long hbits, total;
    int stored;
};

__device__ inline unsigned long long block_sum(unsigned long long v, unsigned long long *ws)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
    for (int i = 0; i < kDefThreads / 64; i++) s += ws[i];
    return s;
}

// the bits of token m (len << 16 | dist - 1, or a literal byte) -> value, and its bit count in *n
__device__ inline unsigned long long token_bits(uint32_t m, const DefShared &S, int *n)
{
    const int ln = (int)(m >> 16);
    if (ln == 0) {
        *n = S.llen[m & 0xFF];
        return S.lcode[m & 0xFF];
    }
    const int ls = c_png.len_sym[ln], dist = (int)(m & 0xFFFF) + 1, ds = dist_sym(dist);
    const int lx = c_png.len_extra[ls], dx = ds < 4 ? 0 : (ds >> 1) - 1;
    unsigned long long v = S.lcode[257 + ls];
    int b = S.llen[257 + ls];
    v |= (unsigned long long)(ln - c_png.len_base[ls]) << b;
    b += lx;
    v |= (unsigned long long)S.dcode[ds] << b;
    b += S.dlen[ds];
    v |= (unsigned long long)(dist - c_png.dist_base[ds]) << b;
    *n = b + dx;
    return v;
}

// ---- the tail of one frame -------------------------------------------------------------------------------------------------------
// One lane: the Adler-32 of the frame's filtered stream from its segments k0 .. k1 (their lengths and sums), as the last 4-byte IDAT
// chunk, and IEND, at p (kPngTailBytes)
__device__ inline void png_frame_tail(const PngSeg *__restrict__ segs, const uint32_t *__restrict__ adler, uint32_t k0, uint32_t k1, uint8_t *p)
{
    uint32_t A = 1, B = 0;
    for (uint32_t k = k0; k < k1; k++) {
        B = (uint32_t)((B + (unsigned long long)((segs[k].s1 - segs[k].s0) % 65521) * A + adler[2 * k + 1]) % 65521);
        A = (A + adler[2 * k]) % 65521;
    }
    const uint32_t ad = B << 16 | A;
    const uint8_t body[8] = {'I', 'D', 'A', 'T', (uint8_t)(ad >> 24), (uint8_t)(ad >> 16), (uint8_t)(ad >> 8), (uint8_t)ad};
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < 8; i++) c = c_png_crc.crc[(c ^ body[i]) & 0xFF] ^ (c >> 8);
    c = ~c;
    p[0] = p[1] = p[2] = 0;
    p[3] = 4;
    for (int i = 0; i < 8; i++) p[4 + i] = body[i];
    p[12] = (uint8_t)(c >> 24);
    p[13] = (uint8_t)(c >> 16);
    p[14] = (uint8_t)(c >> 8);
    p[15] = (uint8_t)c;
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; i++) p[16 + i] = iend[i];
}

}  // namespace ipx
