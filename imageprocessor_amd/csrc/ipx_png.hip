// ipx_png.hip -- png.Encode(w, *image.RGBA) on the GPU and the ABI entries built on it.  Kernels: the opacity reduction (colour type
// 2 or 6), the un-premultiply and filter pass (a workgroup per row: the filter of a row depends only on raw bytes), the deflate of one
// segment of whole rows per workgroup (match candidates, greedy parse, histograms, Huffman tables, bit emission by prefix sum, CRC-32
// and Adler sums), the per-frame head and tail and the pack of the finished pieces.  Host half: ipx_png_host.cpp.  The restatement and
// the stream's definition: DESIGN.md section 4.9; tests/png_model.py is the model the bytes are held to.
#include <vector>

#include "ipx_png.h"
#include "ipx_runtime_internal.h"

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
__constant__ PngTables c_png = PngTables();
__constant__ PngCrcTables c_png_crc = PngCrcTables();

__device__ inline uint32_t png_hash(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return (v * kPngHashMul) >> (32 - kPngHashBits);
}

// ---- opacity ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_opacity_kernel(const uint8_t *__restrict__ src, int w, int h, int stride, size_t frame_stride,
                                                          uint32_t *__restrict__ alpha)
{
    const uint8_t *f = src + (size_t)blockIdx.y * frame_stride;
    const size_t npix = (size_t)w * h;
    int any = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
        const size_t y = i / w, x = i - y * w;
        any |= f[y * stride + 4 * x + 3] != 0xFF;
    }
    if (__syncthreads_or(any) && threadIdx.x == 0) atomicOr(alpha + blockIdx.y, 1u);
}

hipError_t launch_png_opacity(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint32_t *alpha, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min<size_t>(512, ((size_t)w * h + 4095) / 4096);
    hipLaunchKernelGGL(png_opacity_kernel, dim3(blocks, n), dim3(256), 0, s, src, w, h, stride, frame_stride, alpha);
    return hipGetLastError();
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

__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t *__restrict__ src, int w, int stride, size_t frame_stride,
                                                         const uint32_t *__restrict__ alpha, uint8_t *__restrict__ filt, size_t fbytes)
{
    __shared__ int part[5][4];
    const int y = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    const int bpp = alpha[f] ? 4 : 3, rb = w * bpp;
    const uint8_t *row = src + (size_t)f * frame_stride + (size_t)y * stride;
    const uint8_t *prev = y > 0 ? row - stride : nullptr;
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
    uint8_t *out = filt + (size_t)f * fbytes + (size_t)y * (rb + 1);
    if (t == 0) out[0] = (uint8_t)type;
    for (int k = t; k < rb; k += blockDim.x) {
        filter5(row, prev, k, bpp, v);
        out[1 + k] = (uint8_t)v[type];
    }
}

hipError_t launch_png_filter(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, const uint32_t *alpha,
                             uint8_t *filt, size_t fbytes, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_filter_kernel, dim3(h, n), dim3(256), 0, s, src, w, stride, frame_stride, alpha, filt, fbytes);
    return hipGetLastError();
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

__global__ __launch_bounds__(kDefThreads) void png_deflate_kernel(const uint8_t *__restrict__ filt, uint32_t *__restrict__ match,
                                                                  size_t fbytes, int w, int h, const uint32_t *__restrict__ alpha,
                                                                  const PngSeg *__restrict__ segs, uint8_t *__restrict__ out,
                                                                  uint32_t *__restrict__ lens, uint32_t *__restrict__ adler)
{
    __shared__ uint32_t table[kHashSize];   // phase 1: the hash table; phase 2: the walk's window
    __shared__ DefShared S;
    const int t = threadIdx.x;
    const PngSeg sg = segs[blockIdx.x];
    const int bpp = alpha[sg.frame] ? 4 : 3, stride = 1 + w * bpp;
    const uint32_t N = (uint32_t)h * stride, s0 = sg.s0, s1 = sg.s1, L = s1 - s0;
    const bool first = sg.flags & 1, last = sg.flags & 2;
    const uint8_t *data = filt + (size_t)sg.frame * fbytes;
    uint32_t *M = match + (size_t)sg.frame * fbytes;
    uint8_t *o = out + sg.out;

    // ---- 1. candidates: the fixed distances, then the hashed one from a table filled tile by tile
    for (int i = t; i < kHashSize; i += kDefThreads) table[i] = 0;
    __syncthreads();
    for (uint32_t j = (s0 > (uint32_t)kPngWindow ? s0 - kPngWindow : 0) + t; j < s0; j += kDefThreads)
        if (j + 4 <= N) atomicMax(&table[png_hash(data + j)], j + 1);
    __syncthreads();
    int fixed[6], nfixed = 0;
    for (int d = 1; d <= 4; d++) fixed[nfixed++] = d;
    if (stride > 4 && stride <= kPngWindow) fixed[nfixed++] = stride;
    if (2 * stride <= kPngWindow) fixed[nfixed++] = 2 * stride;
    for (uint32_t t0 = s0; t0 < s1; t0 += kPngTile) {
        const uint32_t i = t0 + t;
        if (i < s1) {
            const int cap = (int)min((uint32_t)kPngMaxMatch, s1 - i);
            int best = 0, bd = 0;
            for (int k = 0; k < nfixed && best < cap; k++) {
                const int d = fixed[k];
                if ((uint32_t)d > i) break;
                const int l = match_len(data + i, data + i - d, cap);
                if (l > best) { best = l; bd = d; }
            }
            if (i + 4 <= N) {
                const uint32_t c = table[png_hash(data + i)];
                if (c && i - (c - 1) <= (uint32_t)kPngWindow) {
                    const int d = (int)(i - (c - 1));
                    if (best < cap || d < bd) {
                        const int l = match_len(data + i, data + i - d, cap);
                        if (l > best || (l == best && d < bd)) { best = l; bd = d; }
                    }
                }
            }
            M[i] = best >= kPngMinMatch ? (uint32_t)best << 16 | (uint32_t)(bd - 1) : data[i];
        }
        __syncthreads();
        if (i < s1 && i + 4 <= N) atomicMax(&table[png_hash(data + i)], i + 1);
        __syncthreads();
    }

    // ---- 2. the greedy parse: lane 0 walks windows staged in LDS; tokens go in place to M[s0 + k] (k <= position: never ahead of
    // what is still to be read)
    if (t == 0) { S.ntok = 0; S.p = (int)s0; }
    __syncthreads();
    for (;;) {
        const uint32_t base = (uint32_t)S.p;
        if (base >= s1) break;
        const uint32_t wl = min((uint32_t)kWalkWin, s1 - base);
        for (uint32_t k = t; k < wl; k += kDefThreads) table[k] = M[base + k];
        __syncthreads();
        if (t == 0) {
            uint32_t p = base, nt = (uint32_t)S.ntok;
            while (p < base + wl) {
                const uint32_t m = table[p - base];
                M[s0 + nt++] = m;
                p += m >> 16 ? m >> 16 : 1;
            }
            S.ntok = (int)nt;
            S.p = (int)p;
        }
        __syncthreads();
    }
    const int ntok = S.ntok;

    // ---- 3. histograms and tables
    for (int s = t; s < 286; s += kDefThreads) S.lfreq[s] = 0;
    if (t < 30) S.dfreq[t] = 0;
    if (t < 19) S.cfreq[t] = 0;
    __syncthreads();
    for (int k = t; k < ntok; k += kDefThreads) {
        const uint32_t m = M[s0 + k];
        if (m >> 16) {
            atomicAdd(&S.lfreq[257 + c_png.len_sym[m >> 16]], 1u);
            atomicAdd(&S.dfreq[dist_sym((int)(m & 0xFFFF) + 1)], 1u);
        } else {
            atomicAdd(&S.lfreq[m], 1u);
        }
    }
    __syncthreads();
    if (t == 0) S.lfreq[256] += 1;
    huff_build(S.lfreq, 286, 15, S.llen, S.work);
    huff_build(S.dfreq, 30, 15, S.dlen, S.work);
    if (t == 0) {
        int hlit = 286, hdist = 30;
        while (S.llen[hlit - 1] == 0) hlit--;
        while (hdist > 1 && S.dlen[hdist - 1] == 0) hdist--;
        hlit = max(hlit, 257);
        S.hlit = hlit;
        S.hdist = hdist;
        // run-length code of the hlit + hdist lengths (the model's rle_code_lengths)
        const int n = hlit + hdist;
        int ncl = 0, i = 0;
        auto lenat = [&](int k) { return k < hlit ? S.llen[k] : S.dlen[k - hlit]; };
        auto add = [&](int sym, int x) { S.cl_sym[ncl++] = (uint16_t)(sym | x << 5); S.cfreq[sym]++; };
        while (i < n) {
            const int v = lenat(i);
            int r = 1;
            while (i + r < n && lenat(i + r) == v) r++;
            i += r;
            if (v == 0) {
                while (r >= 11) { const int k = min(r, 138); add(18, k - 11); r -= k; }
                if (r >= 3) { add(17, r - 3); r = 0; }
                for (; r > 0; r--) add(0, 0);
            } else {
                add(v, 0);
                r--;
                while (r >= 3) { const int k = min(r, 6); add(16, k - 3); r -= k; }
                for (; r > 0; r--) add(v, 0);
            }
        }
        S.ncl = ncl;
    }
    huff_build(S.cfreq, 19, 7, S.clen, S.work);
    if (t == 0) {
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && S.clen[order[hclen - 1]] == 0) hclen--;
        S.hclen = hclen;
        huff_codes(S.llen, 286, S.lcode);
        huff_codes(S.dlen, 30, S.dcode);
        huff_codes(S.clen, 19, S.ccode);
        unsigned long long hb = (first ? 16 : 0) + 3 + 14 + 3 * hclen;
        for (int k = 0; k < S.ncl; k++) {
            const int sym = S.cl_sym[k] & 31;
            hb += S.clen[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        S.hbits = hb;
    }
    __syncthreads();
    unsigned long long mine = 0;
    for (int k = t; k < ntok; k += kDefThreads) {
        int n;
        (void)token_bits(M[s0 + k], S, &n);
        mine += n;
    }
    const unsigned long long tokbits = block_sum(mine, S.wsum);
    const unsigned long long dynbits = S.hbits + tokbits + S.llen[256] + 3;
    const size_t dyn_bytes = (size_t)((dynbits + 7) / 8) + 4, st_bytes = png_stored_bytes(L, first);
    const bool stored = st_bytes < dyn_bytes;
    const size_t dlen = stored ? st_bytes : dyn_bytes;
    uint8_t *d8 = o + 8;
    uint32_t *dw = (uint32_t *)d8;

    // ---- 4. the bits
    if (stored) {
        const int z = first ? 2 : 0;
        if (t == 0 && first) { d8[0] = 0x78; d8[1] = 0x9C; }
        const uint32_t nblk = (L + 65534) / 65535;
        for (uint32_t b = t; b <= nblk; b += kDefThreads) {
            const uint32_t q0 = min(b * 65535u, L), bl = b == nblk ? 0 : min(65535u, L - q0);
            uint8_t *hp = d8 + z + 5 * b + q0;
            hp[0] = b == nblk && last ? 1 : 0;
            hp[1] = (uint8_t)bl;
            hp[2] = (uint8_t)(bl >> 8);
            hp[3] = (uint8_t)~bl;
            hp[4] = (uint8_t)(~bl >> 8);
        }
        for (uint32_t q = t; q < L; q += kDefThreads) d8[z + 5 * (q / 65535 + 1) + q] = data[s0 + q];
    } else {
        if (t == 0) {
            unsigned long long pos = 0;
            if (first) { put_bits(dw, pos, 0x9C78, 16); pos = 16; }
            put_bits(dw, pos, 2 << 1, 3);   // BFINAL 0, BTYPE 10
            pos += 3;
            put_bits(dw, pos, (unsigned long long)(S.hlit - 257) | (unsigned long long)(S.hdist - 1) << 5 | (unsigned long long)(S.hclen - 4) << 10, 14);
            pos += 14;
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            for (int k = 0; k < S.hclen; k++, pos += 3) put_bits(dw, pos, S.clen[order[k]], 3);
            for (int k = 0; k < S.ncl; k++) {
                const int sym = S.cl_sym[k] & 31, x = S.cl_sym[k] >> 5, xb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                put_bits(dw, pos, S.ccode[sym] | (unsigned long long)x << S.clen[sym], S.clen[sym] + xb);
                pos += S.clen[sym] + xb;
            }
        }
        // tokens: one per lane per round, positions by an exclusive scan with a running base
        unsigned long long base = S.hbits;
        for (int k0 = 0; k0 < ntok; k0 += kDefThreads) {
            const int k = k0 + t;
            int n = 0;
            unsigned long long v = 0;
            if (k < ntok) v = token_bits(M[s0 + k], S, &n);
            unsigned long long inc = (unsigned long long)n;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long u = __shfl_up(inc, off, 64);
                if ((t & 63) >= off) inc += u;
            }
            __syncthreads();
            if ((t & 63) == 63) S.wsum2[t >> 6] = inc;
            __syncthreads();
            unsigned long long pre = 0, all = 0;
            for (int wv = 0; wv < kDefThreads / 64; wv++) {
                if (wv < (t >> 6)) pre += S.wsum2[wv];
                all += S.wsum2[wv];
            }
            if (k < ntok) put_bits(dw, base + pre + inc - n, v, n);
            base += all;
        }
        if (t == 0) {
            put_bits(dw, base, S.lcode[256], S.llen[256]);
            base += S.llen[256];
            put_bits(dw, base, last ? 1 : 0, 3);   // the empty stored block: BFINAL, BTYPE 00, then byte aligned
            base += 3;
            put_bits(dw, ((base + 7) / 8) * 8 + 16, 0xFFFF, 16);
        }
    }
    __threadfence();
    __syncthreads();

    // ---- 5. the chunk: length, type, CRC-32 of type + data (per-lane raw CRCs shifted into place), and the Adler sums of the segment
    if (t == 0) {
        o[0] = (uint8_t)(dlen >> 24);
        o[1] = (uint8_t)(dlen >> 16);
        o[2] = (uint8_t)(dlen >> 8);
        o[3] = (uint8_t)dlen;
        o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T';
    }
    __threadfence();
    __syncthreads();
    const size_t cn = dlen + 4, per = (cn + kDefThreads - 1) / kDefThreads;
    const size_t b0 = min(cn, per * t), b1 = min(cn, b0 + per);
    uint32_t c = 0;
    for (size_t q = b0; q < b1; q++) {
        const uint32_t wd = __hip_atomic_load((const uint32_t *)(o + 4) + (q >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t byte = (wd >> (8 * (q & 3))) & 0xFF;
        c = c_png_crc.crc[(c ^ byte) & 0xFF] ^ (c >> 8);
    }
    // contribution of this lane's range: shifted by the bytes after it; the initial ~0 state shifted by all of them
    const unsigned long long contrib = b1 > b0 ? crc_shift(c, (uint32_t)(cn - b1), c_png_crc.x2n) : 0;
    unsigned long long x = contrib;
    for (int off = 32; off > 0; off >>= 1) x ^= __shfl_xor(x, off, 64);
    __syncthreads();
    if ((t & 63) == 0) S.wsum[t >> 6] = x;
    __syncthreads();
    if (t == 0) {
        uint32_t crc = crc_shift(0xFFFFFFFFu, (uint32_t)cn, c_png_crc.x2n);
        for (int i = 0; i < kDefThreads / 64; i++) crc ^= (uint32_t)S.wsum[i];
        crc = ~crc;
        uint8_t *cp = o + 8 + dlen;
        cp[0] = (uint8_t)(crc >> 24);
        cp[1] = (uint8_t)(crc >> 16);
        cp[2] = (uint8_t)(crc >> 8);
        cp[3] = (uint8_t)crc;
        lens[blockIdx.x] = (uint32_t)(dlen + 12);
    }
    const uint32_t per2 = (L + kDefThreads - 1) / kDefThreads, a0 = min(L, per2 * t), a1 = min(L, a0 + per2);
    unsigned long long sa = 0, sb = 0;
    for (uint32_t q = a0; q < a1; q++) {
        const uint32_t byte = data[s0 + q];
        sa += byte;
        sb += (unsigned long long)(a1 - q) * byte;
    }
    sb += (unsigned long long)(L - a1) * sa;
    const unsigned long long A = block_sum(sa, S.wsum), B = block_sum(sb, S.wsum2);
    if (t == 0) {
        adler[2 * blockIdx.x] = (uint32_t)(A % 65521);
        adler[2 * blockIdx.x + 1] = (uint32_t)(B % 65521);
    }
}

hipError_t launch_png_deflate(const uint8_t *filt, uint32_t *match, size_t fbytes, int w, int h, const uint32_t *alpha, const PngSeg *segs,
                              int nseg, uint8_t *out, uint32_t *lens, uint32_t *adler, hipStream_t s)
{
    if (nseg <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_deflate_kernel, dim3(nseg), dim3(kDefThreads), 0, s, filt, match, fbytes, w, h, alpha, segs, out, lens, adler);
    return hipGetLastError();
}

// ---- head, tail, pack ------------------------------------------------------------------------------------------------------------
__global__ void png_frame_kernel(const uint8_t *__restrict__ heads, const uint32_t *__restrict__ alpha, const uint32_t *__restrict__ item0,
                                 const PngSeg *__restrict__ segs, const uint32_t *__restrict__ adler, uint8_t *__restrict__ out,
                                 size_t region, size_t tail)
{
    const int f = blockIdx.x, t = threadIdx.x;
    uint8_t *o = out + (size_t)f * region;
    const uint8_t *hd = heads + (alpha[f] ? kPngHeadBytes : 0);
    for (int i = t; i < kPngHeadBytes; i += blockDim.x) o[i] = hd[i];
    if (t != 0) return;
    uint32_t A = 1, B = 0;
    for (uint32_t k = item0[f]; k < item0[f + 1]; k++) {
        B = (uint32_t)((B + (unsigned long long)((segs[k].s1 - segs[k].s0) % 65521) * A + adler[2 * k + 1]) % 65521);
        A = (A + adler[2 * k]) % 65521;
    }
    const uint32_t ad = B << 16 | A;
    uint8_t *p = o + tail;
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

hipError_t launch_png_frame(const uint8_t *heads, const uint32_t *alpha, const uint32_t *item0, const PngSeg *segs, const uint32_t *adler,
                            int n, uint8_t *out, size_t region, size_t tail, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_frame_kernel, dim3(n), dim3(64), 0, s, heads, alpha, item0, segs, adler, out, region, tail);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void png_pack_kernel(const uint8_t *__restrict__ out, const PngPiece *__restrict__ pieces,
                                                       uint8_t *__restrict__ dst)
{
    const PngPiece pc = pieces[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < pc.len; i += blockDim.x) dst[pc.dst + i] = out[pc.src + i];
}

hipError_t launch_png_pack(const uint8_t *out, const PngPiece *pieces, int npieces, uint8_t *dst, hipStream_t s)
{
    if (npieces <= 0) return hipSuccess;
    hipLaunchKernelGGL(png_pack_kernel, dim3(npieces), dim3(256), 0, s, out, pieces, dst);
    return hipGetLastError();
}

}  // namespace ipx

// ---- the entries -----------------------------------------------------------------------------------------------------------------

static int png_check(const char *who, const void *src, int w, int h, long long stride, int n)
{
    if (!src || n < 0 || w <= 0 || h <= 0 || stride < (long long)w * 4) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    if (!frame_span_ok(w, h, (long long)w * 4, 4)) { set_error("%s: %dx%d is beyond the frames the encoder addresses", who, w, h); return IPX_ERR_UNSUPPORTED; }
    return IPX_OK;
}

namespace {
// where the pieces of a frame's stream sit in its region of the output: the head at 0, the segments' chunks from kSegBase (each in
// a slot of its stored bound, 4-byte aligned), the tail at `tail` (the same for both colour types)
constexpr size_t kSegBase = 36;
inline size_t slot_bytes(size_t len, bool first) { return (12 + png_stored_bytes(len, first) + 3) & ~(size_t)3; }
size_t segs_bytes(int w, int h, int bpp)
{
    const PngSegs g(w, h, bpp);
    size_t b = 0;
    for (int s = 0; s < g.nseg; s++) b += slot_bytes((size_t)(g.row0(s + 1, h) - g.row0(s, h)) * g.stride, s == 0);
    return b;
}
}  // namespace

// n frames in HBM -> streams in one pinned block (ipx_host_alloc), everything on stream s; returns once the block is filled
int ipx::png_encode_core(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                           uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    uint8_t heads[2][kPngHeadBytes];
    png_write_heads(w, h, heads);
    std::vector<uint32_t> alpha(n), item0(n + 1), sl;
    std::vector<PngSeg> segs;
    std::vector<PngPiece> pieces;
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    const size_t fbytes = align256((size_t)h * (1 + 4 * (size_t)w));
    const size_t tail = kSegBase + std::max(segs_bytes(w, h, 3), segs_bytes(w, h, 4)), region = align256(tail + kPngTailBytes);
    uint32_t *dalpha;
    IPX_HIP(mem.get(&dalpha, (size_t)n * 4));
    IPX_HIP(hipMemsetAsync(dalpha, 0, (size_t)n * 4, s));
    IPX_HIP(launch_png_opacity(src, w, h, stride, frame_stride, n, dalpha, s));
    IPX_HIP(hipMemcpyAsync(alpha.data(), dalpha, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // the segments of every frame, by its colour type
    for (int f = 0; f < n; f++) {
        item0[f] = (uint32_t)segs.size();
        const PngSegs g(w, h, alpha[f] ? 4 : 3);
        size_t at = (size_t)f * region + kSegBase;
        for (int k = 0; k < g.nseg; k++) {
            PngSeg sg;
            sg.frame = (uint32_t)f;
            sg.s0 = (uint32_t)((size_t)g.row0(k, h) * g.stride);
            sg.s1 = (uint32_t)((size_t)g.row0(k + 1, h) * g.stride);
            sg.flags = (k == 0 ? 1u : 0u) | (k == g.nseg - 1 ? 2u : 0u);
            sg.out = at;
            at += slot_bytes(sg.s1 - sg.s0, k == 0);
            segs.push_back(sg);
        }
    }
    item0[n] = (uint32_t)segs.size();
    const int nseg = (int)segs.size();
    uint8_t *dfilt, *dout, *dheads;
    uint32_t *dmatch, *dlens, *dadler, *ditem0;
    PngSeg *dsegs;
    IPX_HIP(mem.get(&dfilt, fbytes * n));
    IPX_HIP(mem.get(&dmatch, fbytes * n * 4));
    IPX_HIP(mem.get(&dout, region * n));
    IPX_HIP(mem.get(&dheads, sizeof heads));
    IPX_HIP(mem.get(&dlens, (size_t)nseg * 4));
    IPX_HIP(mem.get(&dadler, (size_t)nseg * 8));
    IPX_HIP(mem.get(&ditem0, (size_t)(n + 1) * 4));
    IPX_HIP(mem.get(&dsegs, (size_t)nseg * sizeof(PngSeg)));
    IPX_HIP(hipMemcpyAsync(dheads, heads, sizeof heads, hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(ditem0, item0.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(dsegs, segs.data(), (size_t)nseg * sizeof(PngSeg), hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemsetAsync(dout, 0, region * n, s));
    IPX_HIP(launch_png_filter(src, w, h, stride, frame_stride, n, dalpha, dfilt, fbytes, s));
    IPX_HIP(launch_png_deflate(dfilt, dmatch, fbytes, w, h, dalpha, dsegs, nseg, dout, dlens, dadler, s));
    IPX_HIP(launch_png_frame(dheads, dalpha, ditem0, dsegs, dadler, n, dout, region, tail, s));
    sl.resize(nseg);
    IPX_HIP(hipMemcpyAsync(sl.data(), dlens, (size_t)nseg * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // the pieces: head, the segments' chunks, tail, frame after frame, each stream starting 16-byte aligned
    pieces.reserve(nseg + 2 * (size_t)n);
    size_t total = 0;
    for (int f = 0; f < n; f++) {
        offs[f] = total;
        size_t at = total;
        pieces.push_back({(unsigned long long)f * region, at, (uint32_t)kPngHeadBytes, 0});
        at += kPngHeadBytes;
        for (uint32_t k = item0[f]; k < item0[f + 1]; k++) {
            if (sl[k] > slot_bytes(segs[k].s1 - segs[k].s0, k == item0[f])) { set_error("png: segment %u overran its bound", k); return IPX_ERR_INVALID; }
            pieces.push_back({segs[k].out, at, sl[k], 0});
            at += sl[k];
        }
        pieces.push_back({(unsigned long long)f * region + tail, at, (uint32_t)kPngTailBytes, 0});
        at += kPngTailBytes;
        lens[f] = at - total;
        total = (at + 15) & ~(size_t)15;
    }
    uint8_t *dpack;
    PngPiece *dpieces;
    IPX_HIP(mem.get(&dpack, total));
    IPX_HIP(mem.get(&dpieces, pieces.size() * sizeof(PngPiece)));
    IPX_HIP(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(PngPiece), hipMemcpyHostToDevice, s));
    IPX_HIP(launch_png_pack(dout, dpieces, (int)pieces.size(), dpack, s));
    uint8_t *host = (uint8_t *)ipx_host_alloc(ctx, total);
    if (!host) return IPX_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(host, dpack, total, hipMemcpyDeviceToHost, s);
    { const hipError_t e2 = hipStreamSynchronize(s); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) { (void)ipx_host_free(ctx, host); set_error("png stream download failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
    *blob = host;
    return IPX_OK;
}

extern "C" {

int ipx_png_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                             size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    if (!blob || !offs || !lens) { set_error("ipx_png_encode_batch_dev: bad argument"); return IPX_ERR_INVALID; }
    *blob = nullptr;
    int rc = png_check("ipx_png_encode_batch_dev", src, w, h, stride, n);
    if (rc) return rc;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_png_encode_batch_dev: at most 65535 frames per call"); return IPX_ERR_UNSUPPORTED; }
    LaneLease lane(ctx);
    return png_encode_core(ctx, lane->stream, src, w, h, stride, frame_stride, n, blob, offs, lens);
}
IPX_CATCH_STATUS

int ipx_png_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, uint8_t **out, size_t *len) try
{
    IPX_ENTER(ctx);
    if (!out || !len) { set_error("ipx_png_encode_rgba8: bad argument"); return IPX_ERR_INVALID; }
    *out = nullptr;
    *len = 0;
    int rc = png_check("ipx_png_encode_rgba8", pix, w, h, stride, 1);
    if (rc) return rc;
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    const size_t fbytes = (size_t)w * h * 4;
    uint8_t *blob = nullptr;
    size_t off = 0, n = 0;
    {
        AsyncFree mem{s, {}};
        uint8_t *dsrc;
        IPX_HIP(mem.get(&dsrc, fbytes));
        IPX_HIP(hipMemcpy2DAsync(dsrc, (size_t)w * 4, pix, stride, (size_t)w * 4, h, hipMemcpyHostToDevice, s));
        rc = png_encode_core(ctx, s, dsrc, w, h, w * 4, fbytes, 1, &blob, &off, &n);
        if (rc) return rc;
    }
    uint8_t *m = (uint8_t *)malloc(n);
    if (!m) { (void)ipx_host_free(ctx, blob); set_error("ipx_png_encode_rgba8: out of memory"); return IPX_ERR_NOMEM; }
    memcpy(m, blob + off, n);
    (void)ipx_host_free(ctx, blob);
    *out = m;
    *len = n;
    return IPX_OK;
}
IPX_CATCH_STATUS

// The PNG task's GPU leg (resize.go:83, thumbnail.go:73, watermark.go:71 with png.Encode): chunks of RGBA frames go up, the operators
// run, every output is PNG-encoded in HBM; only the streams come back, into pinned blocks owned by *result.
int ipx_plan_run_host_png(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                          ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (!result) { set_error("ipx_plan_run_host_png: bad argument"); return IPX_ERR_INVALID; }
    *result = nullptr;
    const BatchSrc host = packed_src(kSrcRGBA, src, sstride, src_frame_stride);
    const int rc0 = src_check("ipx_plan_run_host_png", pl, host, n, false);
    if (rc0 || n == 0) return rc0;
    const SrcLayout L = src_layout(pl, host);
    const size_t fsrc = L.frame_bytes();
    const PlanOutputs outs(pl, resize_out, thumb_out, wm_out, Codec::Png, Codec::Png, Codec::Png);
    const size_t per_frame = fsrc + outs.frame_bytes();
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)env_int("IPX_HOST_CHUNK_PNG", 64),
                                                                 ((size_t)1 << 30) / per_frame}));
    ResultOwner res(ctx);
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        StreamSync sync{s};
        AsyncFree mem{s, {}};
        uint8_t *dsrc, *dout = nullptr;
        IPX_HIP(mem.get(&dsrc, fsrc * m));
        if (outs.frame_bytes()) IPX_HIP(mem.get(&dout, outs.frame_bytes() * m));
        BatchSrc d;
        IPX_HIP(src_upload(host, L, i0, m, dsrc, m, s, kCopyFrameRows, &d));
        const int rc = run_chunk(ctx, s, pl, outs, dout, m, d, all_files(n), i0, m, nullptr, nullptr, 0, nullptr, res);
        if (rc) return rc;
    }
    *result = res.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

}  // extern "C"
