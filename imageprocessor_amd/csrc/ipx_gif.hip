// ipx_gif.hip -- gif.Encode(w, *image.RGBA, nil) on the GPU (image/gif writer.go, image/draw drawPaletted, compress/lzw writer.go) and
// the ABI entries built on it.  Kernels: the Plan 9 / Floyd-Steinberg dither (a wavefront, rows in flight across lanes), LZW (one wave
// per frame, one lane coding, the dictionary in LDS) and the packing of the finished streams into one block.  Host half:
// ipx_gif_host.cpp.  DESIGN.md section 4.7 has the restatement and the numbers.
#include <memory>
#include <vector>

#include "ipx_gif.h"
#include "ipx_runtime_internal.h"

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
__constant__ Plan9Taps c_plan9 = Plan9Taps();

__device__ inline int clamp16(int v) { return min(max(v, 0), 0xffff); }
// d * d for d <= 0xffff on the 24-bit multiplier (full rate); HIP's __umul24 returns int, and the product may exceed INT_MAX
__device__ inline uint32_t sq24(uint32_t d) { return (uint32_t)__umul24(d, d); }

// One workgroup per frame, R = blockDim.x rows in flight: thread r codes rows r, r + R, ... ("bands" of R rows); within a band row r
// handles pixel x = t - 2r at step t, so pixel (x, y) runs after (x - 1, y) and (x - 1 .. x + 1, y - 1), which is every error term it
// reads.  drawPaletted's quantErrorCurr[x + 1] for (x, y) is 3 e(x+1, y-1) + 5 e(x, y-1) + e(x-1, y-1) + 7 e(x-1, y): each thread keeps
// its last three errors (h1 h2 h3: steps t-1 .. t-3) and hands the row below 3 h1 + 5 h2 + h3 through a lane shuffle, through LDS at a
// wave boundary (one barrier per step, double-buffered by step parity), and through `carry` (global scratch, one int4 per column) from
// the last row of a band to the first row of the next.  All of it is int32 arithmetic: the order of the adds changes nothing, and the
// truncating division by 16 is applied once per pixel to the complete sum, as Go applies it.
// The search: the first minimum of sqDiff(r) + sqDiff(g) + sqDiff(b) + sqDiff(a) over the 256 entries.  Every entry has alpha 0xffff,
// so the alpha term is the same for all of them; every sum stays below 2^32 (four terms of at most 0x3fff8000), so dropping that term
// changes no comparison.  |d| <= 0xffff: d * d is the 24-bit multiplier's low 32 bits exactly.
__global__ __launch_bounds__(1024) void gif_dither_kernel(const uint8_t *__restrict__ src, int w, int h, int stride, size_t frame_stride,
                                                          uint8_t *__restrict__ index, int4 *__restrict__ carry)
{
    __shared__ int4 link[2][16];   // [step parity][wave]: what the last row of a wave hands the first row of the next
    const int R = blockDim.x;
    const int r = threadIdx.x, lane = r & 63, wv = r >> 6;
    const uint8_t *fs = src + (size_t)blockIdx.x * frame_stride;
    uint8_t *fi = index + (size_t)blockIdx.x * w * h;
    int4 *cy = carry + (size_t)blockIdx.x * w;
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

hipError_t launch_gif_dither(const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t *index, int4 *carry,
                             int rows_in_flight, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_dither_kernel, dim3(n), dim3(rows_in_flight), 0, s, src, w, h, stride, frame_stride, index, carry);
    return hipGetLastError();
}

// ---- LZW -------------------------------------------------------------------------------------------------------------------------
// compress/lzw's writer (LSB, literal width 8) inside image/gif's blockWriter.  The codes it writes are fixed by the algorithm -- greedy
// longest match, a clear code first, width 9 at hi = 257 growing when hi reaches overflow, a clear code and an empty table when hi reaches
// 4095 (that key is not inserted), the saved code, incHi, EOF on Close -- not by Go's hash table, which only finds the matches.  Here the
// dictionary is an open-addressing table in LDS: 8192 entries of (key << 12 | code), key = prefix code << 8 | byte, 0 = empty; at most
// 3838 entries live between clears (load factor <= 0.47).  Lane 0 codes; the wave stages 4 KiB of indices in LDS at a time, clears the
// table and copies the header.  Bytes go into 255-byte sub-blocks as they come; nothing is written at or past `region`.
constexpr int kLzwTab = 8192, kLzwChunk = 4096;

__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t *__restrict__ index, size_t npix, const uint8_t *__restrict__ header,
                                                     uint8_t *__restrict__ out, size_t region, uint32_t *__restrict__ lens)
{
    __shared__ uint32_t table[kLzwTab];
    __shared__ uint8_t chunk[kLzwChunk];
    __shared__ int s_clear;
    const int lane = threadIdx.x;
    const uint8_t *src = index + (size_t)blockIdx.x * npix;
    uint8_t *o = out + (size_t)blockIdx.x * region;
    for (int i = lane; i < kGifHeaderBytes; i += 64) o[i] = header[i];
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
        lens[blockIdx.x] = over || pos > region ? 0xffffffffu : (uint32_t)pos;
    }
}

hipError_t launch_gif_lzw(const uint8_t *index, size_t npix, int n, const uint8_t *header, uint8_t *out, size_t region, uint32_t *lens,
                          hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_lzw_kernel, dim3(n), dim3(64), 0, s, index, npix, header, out, region, lens);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gif_pack_kernel(const uint8_t *__restrict__ out, size_t region, const uint32_t *__restrict__ lens,
                                                       const unsigned long long *__restrict__ obase, uint8_t *__restrict__ dst)
{
    const int f = blockIdx.y;
    const size_t n16 = ((size_t)lens[f] + 15) / 16;
    const uint4 *s = (const uint4 *)(out + (size_t)f * region);
    uint4 *d = (uint4 *)(dst + obase[f]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

hipError_t launch_gif_pack(const uint8_t *out, size_t region, const uint32_t *lens, const unsigned long long *obase, int n, size_t max_len,
                           uint8_t *dst, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    const int blocks = (int)std::min<size_t>(64, (max_len / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(gif_pack_kernel, dim3(blocks, n), dim3(256), 0, s, out, region, lens, obase, dst);
    return hipGetLastError();
}

}  // namespace ipx

// ---- the entries -----------------------------------------------------------------------------------------------------------------

static int gif_check(const char *who, const void *src, int w, int h, long long stride, int n)
{
    if (!src || n < 0 || w <= 0 || h <= 0 || stride < (long long)w * 4) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    if (w >= 1 << 16 || h >= 1 << 16) { set_error("gif: image is too large to encode"); return IPX_ERR_INVALID; }
    return IPX_OK;
}

// rows in flight per frame: a wave per 64 rows, more waves per frame while the batch alone would leave the CUs idle (a band's 2R-step
// ramp costs idle lanes, which only matters once every SIMD has a frame)
static int gif_rows_in_flight(int h, int n)
{
    const int waves = std::min({16, (h + 63) / 64, 2048 / std::max(n, 1)});
    return 64 * std::max(1, std::min(16, env_int("IPX_GIF_WAVES", waves)));   // IPX_GIF_WAVES: for measurements
}

// Asynchronous: the scratch is a stream-ordered allocation of s.
static int gif_dither(hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t *index)
{
    AsyncFree mem{s, {}};
    int4 *carry;
    IPX_HIP(mem.get(&carry, (size_t)n * w * sizeof(int4)));
    IPX_HIP(launch_gif_dither(src, w, h, stride, frame_stride, n, index, carry, gif_rows_in_flight(h, n), s));
    return IPX_OK;
}

// n frames in HBM -> streams in one pinned block (ipx_host_alloc), everything on stream s; returns once the block is filled
int gif_encode_core(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                           uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    uint8_t hdr[kGifHeaderBytes];
    gif_write_header(w, h, hdr);
    std::vector<uint32_t> hl(n);
    std::vector<unsigned long long> ob(n);
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    const size_t npix = (size_t)w * h, region = align256(gif_stream_bound(w, h));
    uint8_t *didx, *dout, *dhdr;
    uint32_t *dlens;
    unsigned long long *dob;
    IPX_HIP(mem.get(&didx, npix * n));
    IPX_HIP(mem.get(&dout, region * n));
    IPX_HIP(mem.get(&dhdr, sizeof hdr));
    IPX_HIP(mem.get(&dlens, (size_t)n * 4));
    IPX_HIP(mem.get(&dob, (size_t)n * 8));
    IPX_HIP(hipMemcpyAsync(dhdr, hdr, sizeof hdr, hipMemcpyHostToDevice, s));
    int rc = gif_dither(s, src, w, h, stride, frame_stride, n, didx);
    if (rc) return rc;
    IPX_HIP(launch_gif_lzw(didx, npix, n, dhdr, dout, region, dlens, s));
    IPX_HIP(hipMemcpyAsync(hl.data(), dlens, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    size_t total = 0, max_len = 0;
    for (int i = 0; i < n; i++) {
        if (hl[i] == 0xffffffffu || hl[i] > region) { set_error("gif: stream of frame %d overran its bound", i); return IPX_ERR_INVALID; }
        offs[i] = total;
        lens[i] = hl[i];
        ob[i] = total;
        total += align16(hl[i]);
        max_len = std::max<size_t>(max_len, hl[i]);
    }
    uint8_t *dpack;
    IPX_HIP(mem.get(&dpack, total));
    IPX_HIP(hipMemcpyAsync(dob, ob.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    IPX_HIP(launch_gif_pack(dout, region, dlens, dob, n, max_len, dpack, s));
    return download_streams(ctx, s, dpack, total, "gif ", blob);
}

extern "C" {

int ipx_dev_gif_dither_rgba8(ipx_ctx *ctx, void *stream, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                             uint8_t *index) try
{
    IPX_ENTER(ctx);
    int rc = gif_check("ipx_dev_gif_dither_rgba8", src, w, h, stride, n);
    if (rc) return rc;
    if (!index) { set_error("ipx_dev_gif_dither_rgba8: bad argument"); return IPX_ERR_INVALID; }
    if (n == 0) return IPX_OK;
    return gif_dither(stream ? (hipStream_t)stream : ctx->stream, src, w, h, stride, frame_stride, n, index);
}
IPX_CATCH_STATUS

int ipx_gif_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                             size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    if (!blob || !offs || !lens) { set_error("ipx_gif_encode_batch_dev: bad argument"); return IPX_ERR_INVALID; }
    *blob = nullptr;
    int rc = gif_check("ipx_gif_encode_batch_dev", src, w, h, stride, n);
    if (rc) return rc;
    if (n == 0) return IPX_OK;
    LaneLease lane(ctx);
    return gif_encode_core(ctx, lane->stream, src, w, h, stride, frame_stride, n, blob, offs, lens);
}
IPX_CATCH_STATUS

int ipx_gif_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, uint8_t **out, size_t *len) try
{
    IPX_ENTER(ctx);
    return encode_one_rgba8("ipx_gif_encode_rgba8", ctx, gif_check, gif_encode_core, pix, w, h, stride, out, len);
}
IPX_CATCH_STATUS

// The GIF task's GPU leg (resize.go:78-91, thumbnail.go:68-81 with gif.Encode; watermark.go:66-79, where a GIF watermark becomes a JPEG):
// chunks of paletted frames go up, the operators run, resize and thumbnail outputs are GIF-encoded and the
// watermark output JPEG-encoded, all in HBM; only the streams come back, into pinned blocks owned by *result.
int ipx_plan_run_host_paletted_gif(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *index, int stride, size_t frame_stride,
                                   const uint8_t *palettes, int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out,
                                   ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    return run_host_streams("ipx_plan_run_host_paletted_gif", ctx, pl, n, packed_src(kSrcPaletted, index, stride, frame_stride, palettes), Codec::Gif,
                            Codec::Gif, Codec::Jpeg, "IPX_HOST_CHUNK_GIF", 64, quality, resize_out, thumb_out, wm_out, result);
}
IPX_CATCH_STATUS

}  // extern "C"
