// ipx_gif_dec.hip -- gif.Decode (image/gif reader.go, compress/lzw reader.go) of the first image of a batch of files on the GPU, and
// the ABI entries built on it: the decode entries for files of one size and of any sizes, the uniform GIF-in, GIF-out leg and what GIF
// supplies to the mixed-size one (ipx_run_gif_gif_mixed: the walk is mixed_leg in ipx_mixed_leg.h).  Kernels: the code walk (one lane per file reads the codes, keeps the live dictionary's lengths and
// first bytes in LDS and checks every rule of the reader, O(1) work per code) and the expansion (every lane of a grid takes one code and
// writes its string backwards along the entry -> code-ordinal map of its segment, straight into the de-interlaced row).  Host half:
// ipx_gif_dec_host.cpp.  Under IPX_GIF_PAR=1 the walk is gif_walk_par_kernel (ipx_gif_dec_par.hip: all 64 lanes read codes) with the walk
// of this file behind it for the files it leaves.  DESIGN.md section 4.8 has the restatement and the numbers.
#include <algorithm>
#include <vector>

#include "ipx_gif_dec.h"
#include "ipx_mixed_leg.h"

namespace ipx {

// ---- code walk -----------------------------------------------------------------------------------------------------------------
// One wave per file; the wave stages the LZW bytes in LDS 4 KiB at a time, lane 0 reads the codes.  Per code that outputs bytes it
// writes a GifCode record (its output offset, its segment, its value, the previous code's value, its first byte).  It stops at the EOF
// code, at the end of the data, or at the first rule broken: an invalid code, a byte past the frame, a literal >= len(palette) (every
// pixel is a copy of some literal code's value, and every literal code's own byte lands in the frame, so the set of pixel values is the
// set of literal codes read: Go's per-pixel "invalid pixel value" check and this per-code one fail on the same files).  At the EOF code,
// blockReader.close's rule: the code's last byte lies in the last sub-block, or the data ended exactly on a sub-block boundary and one
// sub-block of one byte follows; either way a block terminator comes next.  Records are bounded by the host's code_cap.
// redo (under IPX_GIF_PAR=1, behind gif_walk_par_kernel): the files' redo words, redo[kGifStateWords * slot]; only the files whose word
// is set are walked, from scratch.  nullptr: every file.
constexpr int kWalkChunk = 4096;

__global__ __launch_bounds__(64) void gif_walk_kernel(const uint8_t *__restrict__ blob, const GifDecDesc *__restrict__ desc,
                                                      GifCode *__restrict__ codes, uint32_t *__restrict__ state,
                                                      const uint32_t *__restrict__ redo)
{
    __shared__ uint16_t s_len[4096];
    __shared__ uint8_t s_first[4096];
    __shared__ uint8_t s_buf[kWalkChunk + 4];
    __shared__ uint32_t s_base;
    __shared__ int s_done;
    const int lane = threadIdx.x;
    const GifDecDesc d = desc[blockIdx.x];
    if (redo && redo[kGifStateWords * d.slot] == 0) return;
    const uint8_t *src = blob + d.data_off;
    GifCode *rec = codes + d.code_off;
    const uint32_t clear = 1u << d.lit, eof = clear + 1, npix = d.w * d.h;
    const uint64_t nbits = 8ull * d.data_len;
    // the reader (meaningful in lane 0)
    uint64_t bit = 0;
    uint32_t width = d.lit + 1, hi = eof, overflow = 1u << width;
    bool have_last = false;
    uint32_t last = 0, last_len = 0, last_first = 0, count = 0, k = 0, segb = 0, st = 0;
    if (lane == 0) { s_base = 0; s_done = 0; }
    __syncthreads();
    for (;;) {
        const uint32_t base = s_base;
        for (int i = lane; i < kWalkChunk + 4; i += 64) s_buf[i] = base + (uint32_t)i < d.data_len ? src[base + i] : 0;
        __syncthreads();
        if (lane == 0) {
            bool done = false;
            while ((uint32_t)(bit >> 3) - base < (uint32_t)kWalkChunk) {
                if (bit + width > nbits) {        // the data end without an EOF code: accepted once the frame is complete
                    st = (d.flags & kGifTerminated) && count == npix ? 0 : 1;
                    done = true;
                    break;
                }
                const uint32_t o = (uint32_t)(bit >> 3) - base;
                const uint32_t raw = s_buf[o] | (uint32_t)s_buf[o + 1] << 8 | (uint32_t)s_buf[o + 2] << 16;
                const uint32_t v = (raw >> (bit & 7)) & ((1u << width) - 1);
                bit += width;
                if (v == clear) {
                    width = d.lit + 1; hi = eof; overflow = 1u << width; have_last = false; segb = k;
                    continue;
                }
                if (v == eof) {
                    const uint64_t used = (bit + 7) >> 3;
                    const bool close_ok = (d.flags & kGifTerminated) &&
                                          (used > d.last_start || (used == d.last_start && (d.flags & kGifLastIsOne)));
                    st = count == npix && close_ok ? 0 : 1;
                    done = true;
                    break;
                }
                uint32_t L, f;
                if (v < clear) {
                    if (v >= d.pal_len) { st = 1; done = true; break; }     // invalid pixel value
                    L = 1; f = v;
                } else if (v < hi || (v == hi && !have_last)) {             // (the second: a full table, entry 4095)
                    L = s_len[v]; f = s_first[v];
                } else if (v == hi) {                                       // KwKwK
                    L = last_len + 1; f = last_first;
                } else {                                                    // invalid code
                    st = 1; done = true; break;
                }
                if (L > npix - count) { st = 1; done = true; break; }       // too much image data
                if (k + 1 >= d.code_cap) { st = 2; done = true; break; }
                rec[k] = GifCode{count, segb, v | (have_last ? last : 0u) << 12 | f << 24};
                if (have_last) { s_len[hi] = (uint16_t)(last_len + 1); s_first[hi] = (uint8_t)last_first; }
                count += L;
                k++;
                have_last = true; last = v; last_len = L; last_first = f;
                if (++hi >= overflow) {
                    if (width == 12) { have_last = false; hi--; }           // no entry is added until a clear code
                    else { width++; overflow <<= 1; }
                }
            }
            if (done) s_done = 1;
            else s_base = (uint32_t)(bit >> 3);
        }
        __syncthreads();
        if (s_done) break;
    }
    if (lane == 0) {
        rec[k].off = count;                     // the closing offset (k < code_cap)
        state[kGifStateWords * d.slot] = st;
        state[kGifStateWords * d.slot + 1] = k;
    }
}

hipError_t launch_gif_walk(const uint8_t *blob, const GifDecDesc *desc, int n, GifCode *codes, uint32_t *state, const uint32_t *redo,
                           hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_walk_kernel, dim3(n), dim3(64), 0, s, blob, desc, codes, state, redo);
    return hipGetLastError();
}

// ---- expansion -----------------------------------------------------------------------------------------------------------------
// Lane per record.  The entry E > eof of a code in segment b was defined by record j = b + (E - eof): E's last byte is j's first byte
// and the rest is the string of the code before j, whose value j carries.  Each step moves to a record strictly before the last, so a
// string of L bytes costs L steps and nothing is shared between lanes.  Writes stay inside [off, next off) of the frame's own pixels
// (checked against the frame size, whatever the records say); files whose walk failed are skipped.
__global__ __launch_bounds__(256) void gif_expand_kernel(const GifDecDesc *__restrict__ desc, const GifCode *__restrict__ codes,
                                                         const uint32_t *__restrict__ state, uint8_t *__restrict__ frames)
{
    const GifDecDesc d = desc[blockIdx.y];
    if (state[kGifStateWords * d.slot] != 0) return;
    const uint32_t nrec = min(state[kGifStateWords * d.slot + 1], d.code_cap - 1);
    const GifCode *rec = codes + d.code_off;
    uint8_t *out = frames + d.frame_off;
    const uint32_t w = d.w, h = d.h, npix = w * h, clear = 1u << d.lit, eof = clear + 1;
    const bool il = (d.flags & kGifInterlaced) != 0;
    const uint32_t n0 = (h + 7) / 8, n1 = (h + 3) / 8, n2 = (h + 1) / 4;
    auto row = [&](uint32_t r) -> uint32_t {      // the interlaced passes (8, 0), (8, 4), (4, 2), (2, 1)
        if (!il) return r;
        if (r < n0) return 8 * r;
        r -= n0;
        if (r < n1) return 8 * r + 4;
        r -= n1;
        if (r < n2) return 4 * r + 2;
        return 2 * (r - n2) + 1;
    };
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nrec; k += gridDim.x * blockDim.x) {
        const GifCode me = rec[k];
        const uint32_t end = rec[k + 1].off;
        if (end > npix || end <= me.off) continue;
        uint32_t pos = end - 1, r = pos / w, x = pos - r * w, y = row(r);
        uint32_t v = me.packed & 4095, lim = k;
        for (;;) {
            uint32_t byte, next = 0;
            const bool lit = v < clear;
            if (lit) {
                byte = v;
            } else {
                const uint32_t j = me.segb + (v - eof);
                if (v <= eof || j > lim) break;
                const uint32_t p = rec[j].packed;
                byte = p >> 24;
                next = (p >> 12) & 4095;
                lim = j - 1;
            }
            out[(size_t)y * w + x] = (uint8_t)byte;
            if (lit || pos == me.off) break;
            pos--;
            if (x == 0) { x = w - 1; r--; y = row(r); }
            else x--;
            v = next;
        }
    }
}

hipError_t launch_gif_expand(const GifDecDesc *desc, int n, const GifCode *codes, const uint32_t *state, uint8_t *frames,
                             int blocks_per_file, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gif_expand_kernel, dim3(blocks_per_file, n), dim3(256), 0, s, desc, codes, state, frames);
    return hipGetLastError();
}

}  // namespace ipx

// ---- the decode core -------------------------------------------------------------------------------------------------------------

// parse n files (a thread per eight of them); status[i] from the container
static int gif_parse_all(const ipx_bytes *files, int n, std::vector<GifFileInfo> &info, int *status)
{
    return parallel_light(n, [&](int i) { status[i] = gif_parse(files[i].data, files[i].data ? files[i].len : 0, &info[i]); }, "gif decode: host parse failed");
}

// gif_parse_all, then the batch's size: *w x *h, or the first parsed file's when *w == 0 (files of another size: IPX_ERR_UNSUPPORTED)
static int gif_parse_batch(const ipx_bytes *files, int n, int *w, int *h, std::vector<GifFileInfo> &info, int *status)
{
    const int rc = gif_parse_all(files, n, info, status);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        if (*w <= 0) { *w = info[i].w; *h = info[i].h; }
        if (info[i].w != *w || info[i].h != *h) status[i] = IPX_ERR_UNSUPPORTED;
    }
    return IPX_OK;
}

// Decodes the files with status IPX_OK, of any sizes, into frames + at.off[i] (w x h, rows w bytes apart) and their palettes into
// palettes + at.pal_slot[i] * 1024 (every slot of the layout is written; zero for a file that is not decoded), all on stream s; the
// walk's verdict lands in status[].  The code scratch is cut into groups of at most ~4 GiB (IPX_GIF_DEC_SCRATCH_MB); one read-back of
// the per-file words at the end.  A launch's records are ordered longest data first when the layout asks for it (files of different
// sizes): the walk is one wave per file and a launch ends with its longest file; what is written depends on nothing but a file's
// own record.
static int gif_decode_files(ipx_ctx *ctx, hipStream_t s, const ipx_bytes *files, int n, const std::vector<GifFileInfo> &info,
                            const GifFrameLayout &at, uint8_t *frames, uint8_t *palettes, int *status)
{
    PinnedBlocks pinned(ctx, s);
    AsyncFree mem{s, {}};
    // IPX_GIF_PAR=1 in the environment, read on every call: the walk is gif_walk_par_kernel with the serial walk behind it for the files
    // it leaves; anything else keeps the serial walk alone
    const bool par = env_int("IPX_GIF_PAR", 0) == 1;
    uint32_t *dstate;
    IPX_HIP(mem.get(&dstate, (size_t)n * kGifStateWords * 4));
    // palettes: one upload of every slot
    uint8_t *hpal = pinned.get((size_t)std::max(at.pal_slots, 1) * 1024);
    if (!hpal) return IPX_ERR_NOMEM;
    for (int i = 0; i < n; i++) {
        if (at.pal_slot[i] < 0) continue;
        if (status[i] == IPX_OK) memcpy(hpal + (size_t)at.pal_slot[i] * 1024, info[i].pal, 1024);
        else memset(hpal + (size_t)at.pal_slot[i] * 1024, 0, 1024);
    }
    if (at.pal_slots) IPX_HIP(hipMemcpyAsync(palettes, hpal, (size_t)at.pal_slots * 1024, hipMemcpyHostToDevice, s));
    const size_t budget = (size_t)env_int("IPX_GIF_DEC_SCRATCH_MB", 4096) << 20;
    auto run_group = [&](std::vector<int> group) -> int {
        const int m = (int)group.size();
        if (at.longest_first) std::stable_sort(group.begin(), group.end(), [&](int a, int b) { return info[a].data_len > info[b].data_len; });
        size_t data_bytes = 0, codes = 0;
        uint32_t max_cap = 0;
        std::vector<GifDecDesc> desc(m);
        for (int g = 0; g < m; g++) {
            const GifFileInfo &f = info[group[g]];
            GifDecDesc &d = desc[g];
            memset(&d, 0, sizeof d);
            d.data_off = data_bytes;
            d.code_off = codes;
            d.frame_off = at.off[group[g]];
            d.data_len = f.data_len;
            d.last_start = f.last_start;
            d.code_cap = gif_code_cap(f);
            d.w = (uint32_t)f.w;
            d.h = (uint32_t)f.h;
            d.pal_len = std::min<uint32_t>(f.pal_len, 256);
            d.slot = (uint32_t)group[g];
            d.lit = (uint16_t)f.lit;
            d.flags = (uint8_t)((f.terminated ? kGifTerminated : 0) | (f.last_is_one ? kGifLastIsOne : 0) | (f.interlaced ? kGifInterlaced : 0));
            data_bytes += align16(f.data_len);
            codes += d.code_cap;
            max_cap = std::max(max_cap, d.code_cap);
        }
        const size_t desc_bytes = align256(sizeof(GifDecDesc) * m);
        uint8_t *hblob = pinned.get(desc_bytes + data_bytes);
        if (!hblob) return IPX_ERR_NOMEM;
        memcpy(hblob, desc.data(), sizeof(GifDecDesc) * m);
        const int rc = parallel_light(m, [&](int g) {
            const int i = group[g];
            gif_gather(files[i].data, files[i].len, info[i], hblob + desc_bytes + desc[g].data_off);
        }, "gif decode: host gather failed");
        if (rc) return rc;
        uint8_t *dblob;
        GifCode *dcodes;
        IPX_HIP(mem.get(&dblob, desc_bytes + data_bytes));
        IPX_HIP(mem.get(&dcodes, codes * sizeof(GifCode)));
        IPX_HIP(hipMemcpyAsync(dblob, hblob, desc_bytes + data_bytes, hipMemcpyHostToDevice, s));
        const GifDecDesc *ddesc = (const GifDecDesc *)dblob;
        if (par) {
            IPX_HIP(launch_gif_walk_par(dblob + desc_bytes, ddesc, m, dcodes, dstate, s));
            IPX_HIP(launch_gif_walk(dblob + desc_bytes, ddesc, m, dcodes, dstate, dstate + 2, s));
        } else {
            IPX_HIP(launch_gif_walk(dblob + desc_bytes, ddesc, m, dcodes, dstate, nullptr, s));
        }
        const int bpf = (int)std::max<uint32_t>(1, std::min<uint32_t>((max_cap + 255) / 256, (uint32_t)std::max(1, 16384 / m)));
        IPX_HIP(launch_gif_expand(ddesc, m, dcodes, dstate, frames, bpf, s));
        return IPX_OK;
    };
    std::vector<int> ok;
    for (int i = 0; i < n; i++) if (status[i] == IPX_OK) ok.push_back(i);
    const int rc = for_groups_under(ok, budget, [&](int i) { return (size_t)gif_code_cap(info[i]) * sizeof(GifCode) + info[i].data_len; }, run_group);
    if (rc) return rc;
    std::vector<uint32_t> st((size_t)n * kGifStateWords);
    IPX_HIP(hipMemcpyAsync(st.data(), dstate, st.size() * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    if (par) {                                                   // ipx_gif_decode_counts
        long long c[4] = {0, 0, 0, 0};
        for (int i = 0; i < n; i++) {
            if (status[i] != IPX_OK) continue;
            c[0]++;
            if (st[(size_t)kGifStateWords * i + 2]) { c[2]++; continue; }
            c[1]++;
            c[3] += st[(size_t)kGifStateWords * i + 3];
        }
        for (int k = 0; k < 4; k++) ctx->gif_counts[k] += c[k];
    }
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        const uint32_t v = st[(size_t)kGifStateWords * i];
        status[i] = v == 0 ? IPX_OK : v == 1 ? IPX_ERR_INVALID : IPX_ERR_UNSUPPORTED;   // 2: scratch too small (cannot happen)
    }
    return IPX_OK;
}

// ---- the entries -----------------------------------------------------------------------------------------------------------------
extern "C" {

int ipx_gif_decode_counts(ipx_ctx *ctx, long long counts[4])
{
    clear_error();
    if (!ctx || !counts) { set_error("ipx_gif_decode_counts: bad argument"); return IPX_ERR_INVALID; }
    for (int k = 0; k < 4; k++) counts[k] = ctx->gif_counts[k].load();
    return IPX_OK;
}

void ipx_gif_frames_free(ipx_ctx *ctx, ipx_gif_frames *o) { dev_blocks_free(ctx, o); }

int ipx_gif_decode_batch(ipx_ctx *ctx, void *stream, const ipx_bytes *gifs, int n, int *w, int *h, ipx_paletted_batch *frames,
                         int *status, ipx_gif_frames **owner) try
{
    IPX_ENTER(ctx);
    if (!gifs || n < 0 || !w || !h || !frames || !status || !owner || *w < 0 || *h < 0 || (*w == 0) != (*h == 0)) {
        set_error("ipx_gif_decode_batch: bad argument");
        return IPX_ERR_INVALID;
    }
    *owner = nullptr;
    memset(frames, 0, sizeof *frames);
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_gif_decode_batch: at most 65535 files per call"); return IPX_ERR_UNSUPPORTED; }
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<GifFileInfo> info(n);
    int bw = *w, bh = *h;
    int rc = gif_parse_batch(gifs, n, &bw, &bh, info, status);
    if (rc) return rc;
    if (!any_ok(status, n)) return IPX_OK;
    OwnedBlocks<ipx_gif_frames> o(ctx, s);
    const size_t fs = align256((size_t)bw * bh);
    uint8_t *dframes = nullptr, *dpal = nullptr;
    hipError_t e = o.alloc(&dframes, fs * n);
    if (e == hipSuccess) e = o.alloc(&dpal, (size_t)n * 1024);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("ipx_gif_decode_batch: device allocation failed: %s", hipGetErrorString(e));
        return IPX_ERR_NOMEM;
    }
    rc = gif_decode_files(ctx, s, gifs, n, info, gif_layout_strided(n, fs), dframes, dpal, status);
    if (rc) return rc;
    *w = bw;
    *h = bh;
    if (!any_ok(status, n)) return IPX_OK;     // every image failed in its data: no frames
    frames->index = dframes;
    frames->stride = bw;
    frames->frame_stride = fs;
    frames->palettes = dpal;
    *owner = o.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

// n files of any sizes: every file that parses goes through ONE gif_decode_files call -- one upload, one walk launch (two under
// IPX_GIF_PAR=1) and one expand launch per scratch group -- its frame at an offset of its own in one block (256-byte aligned, rows
// tight) and its palette in the next free slot of a second block
int ipx_gif_decode_mixed(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, ipx_gif_frame *frames, int *status,
                         ipx_gif_frames **owner) try
{
    IPX_ENTER(ctx);
    if (n < 0 || !owner || (n && (!files || !frames || !status))) { set_error("ipx_gif_decode_mixed: bad argument"); return IPX_ERR_INVALID; }
    *owner = nullptr;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_gif_decode_mixed: at most 65535 files per call"); return IPX_ERR_UNSUPPORTED; }
    memset(frames, 0, (size_t)n * sizeof *frames);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<GifFileInfo> info(n);
    int rc = gif_parse_all(files, n, info, status);
    if (rc) return rc;
    if (!any_ok(status, n)) return IPX_OK;
    const GifFrameLayout at = gif_layout_packed(n, [&](int i) { return status[i] == IPX_OK; }, [&](int i) { return (size_t)info[i].w * info[i].h; });
    OwnedBlocks<ipx_gif_frames> o(ctx, s);
    uint8_t *dframes = nullptr, *dpal = nullptr;
    hipError_t e = o.alloc(&dframes, at.bytes);
    if (e == hipSuccess) e = o.alloc(&dpal, (size_t)at.pal_slots * 1024);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("ipx_gif_decode_mixed: device allocation failed: %s", hipGetErrorString(e));
        return IPX_ERR_NOMEM;
    }
    rc = gif_decode_files(ctx, s, files, n, info, at, dframes, dpal, status);
    if (rc) return rc;
    if (!any_ok(status, n)) return IPX_OK;     // every image failed in its data: no frames
    for (int i = 0; i < n; i++)
        if (status[i] == IPX_OK) frames[i] = ipx_gif_frame{info[i].w, info[i].h, dframes + at.off[i], info[i].w, dpal + (size_t)at.pal_slot[i] * 1024};
    *owner = o.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

// The GIF task's GPU leg from the uploads on: per chunk of files, the host parse and the upload of the LZW data, the walk and the
// expansion into HBM, then the chunk step (run_chunk): the operators, gif.Encode of the resize and thumbnail outputs and jpeg.Encode of the
// watermark output (a GIF watermark becomes a JPEG, watermark.go:73).  Chunks are bounded as in ipx_plan_run_host_paletted_gif.  The operators run
// on every slot of a chunk (a failed file's slot holds whatever its frame holds); only OK files' streams are handed out.
// (the body of ipx_plan_run_gif_gif -- texts == NULL: no text launch -- and of ipx_plan_run_gif_gif_texts, where texts[i] is drawn on
// file i's watermark frame between the operators and the encoders: one text set per call, the selection is the whole call and chunk i0
// is its slots i0 .. i0 + m)
static int run_gif_gif(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                       ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result)
{
    *result = nullptr;
    const int sw = pl->p.sw, sh = pl->p.sh;
    const PlanOutputs outs(pl, resize_out, thumb_out, wm_out, Codec::Gif, Codec::Gif, Codec::Jpeg);
    int rc = outs.check_gif();
    if (rc) return rc;
    outs.clear(n);
    if (n == 0) return IPX_OK;
    if (!frame_span_ok(sw, sh, sw, 1)) {
        for (int i = 0; i < n; i++) status[i] = IPX_ERR_UNSUPPORTED;
        return IPX_OK;
    }
    const size_t fsrc = align256((size_t)sw * sh);
    const size_t per_frame = fsrc + 1024 + outs.frame_bytes();
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)env_int("IPX_HOST_CHUNK_GIF", 64),
                                                                 ((size_t)1 << 30) / per_frame}));
    ResultOwner res(ctx);
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    std::vector<GifFileInfo> info(chunk);
    LegTexts lt;
    if ((rc = lt.build(s, who, pl, outs, texts, all_files(n), true))) return rc;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        int bw = sw, bh = sh;
        rc = gif_parse_batch(files + i0, m, &bw, &bh, info, status + i0);
        if (rc) return rc;
        if (!any_ok(status + i0, m)) continue;
        StreamSync sync{s};
        AsyncFree mem{s, {}};
        uint8_t *didx, *dpal, *dout = nullptr;
        IPX_HIP(mem.get(&didx, fsrc * m));
        IPX_HIP(mem.get(&dpal, (size_t)1024 * m));
        if (outs.frame_bytes()) IPX_HIP(mem.get(&dout, outs.frame_bytes() * m));
        rc = gif_decode_files(ctx, s, files + i0, m, info, gif_layout_strided(m, fsrc), didx, dpal, status + i0);
        if (rc) return rc;
        if (!any_ok(status + i0, m)) continue;
        rc = run_chunk(ctx, s, pl, outs, dout, m, packed_src(kSrcPaletted, didx, sw, fsrc, dpal), all_files(n), i0, m, &lt, nullptr, quality, status, res);
        if (rc) return rc;
    }
    *result = res.release();
    return IPX_OK;
}

int ipx_plan_run_gif_gif(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, int quality, ipx_bytes *resize_out,
                         ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (const int rc = leg_entry_check("ipx_plan_run_gif_gif", pl, n, files, status, result, false, nullptr)) return rc;
    return run_gif_gif("ipx_plan_run_gif_gif", ctx, pl, n, files, nullptr, quality, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

int ipx_plan_run_gif_gif_texts(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                               ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (const int rc = leg_entry_check("ipx_plan_run_gif_gif_texts", pl, n, files, status, result, true, texts)) return rc;
    return run_gif_gif("ipx_plan_run_gif_gif_texts", ctx, pl, n, files, texts, quality, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

}  // extern "C"

// ---- the mixed-size GIF leg: what GIF supplies to the walk of ipx_mixed_leg.h ------------------------------------------------------

namespace {
struct GifMixed {
    static constexpr const char *kWho = "ipx_run_gif_gif_mixed";
    static constexpr const char *kGroupEnv = "IPX_GIF_MIXED_GROUP", *kChunkEnv = "IPX_GIF_MIXED_CHUNK_MB";
    // the dither gives a frame one workgroup and the coder one wave, so a chunk wants some hundreds of frames; DESIGN.md section 4.8
    // has what was measured beside these
    static constexpr int kGroupFiles = 256, kChunkMB = 4096;
    static constexpr bool kRunsWithoutOutputs = false;      // a run no output is made for is left out
    // a file the walk failed is left out of its run and, with its status, out of every encode
    bool decoded(int i) const { return status[i] == IPX_OK; }

    int quality;
    const int *status = nullptr;            // the caller's
    std::vector<GifFileInfo> info;
    // a group's frames and palettes: stream-ordered, they go back with the group
    struct Group {
        AsyncFree mem;
        GifFrameLayout at;                  // by the file's place in the group
        uint8_t *dfr = nullptr, *dpal = nullptr;
        Group(ipx_ctx *, hipStream_t s) : mem{s, {}} {}
    };
    // three arenas of frames, and the watermark frames' coefficient scratch
    struct Chunk : ChunkFrames {
        uint8_t *coefs = nullptr;
        std::vector<size_t> coef_off;       // file p's coefficients at coefs + coef_off[p]
    };

    int refuse(const ipx_pool_ops *ops, int n, const ipx_text *texts) const
    {
        if (texts && (ops->glyphs || ops->n_glyphs)) {
            set_error("%s: a text per file needs ops->glyphs == NULL: the plan copies the frame and the texts are drawn behind it", kWho);
            return IPX_ERR_INVALID;
        }
        if (n > 65535) { set_error("%s: at most 65535 files per call", kWho); return IPX_ERR_UNSUPPORTED; }
        return IPX_OK;
    }
    int parse(const ipx_bytes *files, int n, int *st)
    {
        status = st;
        info.resize(n);
        return gif_parse_all(files, n, info, st);
    }
    std::pair<int, int> size(int i) const { return {info[i].w, info[i].h}; }
    int kind(int) const { return 0; }       // every frame is *image.Paletted
    // a GIF output of 65536 or more on a side is that file's refusal alone (the uniform leg's check_gif refuses the call)
    int admit(const MixedCall &c, int i) const
    {
        for (int k : {kOutResize, kOutThumb})
            if (c.has(i, k) && (c.shape(i, k).w >= 1 << 16 || c.shape(i, k).h >= 1 << 16)) return IPX_ERR_INVALID;
        return IPX_OK;
    }
    // bytes a file costs its decode group: the frame, the palette, the LZW data and the code scratch
    size_t decode_cost(int i) const
    {
        return align256((size_t)info[i].w * info[i].h) + 1024 + align16(info[i].data_len) + (size_t)gif_code_cap(info[i]) * sizeof(GifCode);
    }
    static size_t coef_bytes(const OutShape &sh) { return align256(ipx_jpeg_coef_count(sh.w, sh.h) * sizeof(int16_t)); }
    // What output k costs a chunk: the frame and what the encoder allocates behind it.  A GIF output (resize, thumbnail): the index
    // bytes, the region and the carry row.  The JPEG output (watermark): its coefficients, and the encoder's streams (about the
    // coefficients again).
    size_t out_cost(const OutShape &sh, int k) const
    {
        if (k == kOutWm) return align256(sh.bytes) + 2 * coef_bytes(sh);
        return align256(sh.bytes) + align256((size_t)sh.w * sh.h) + align256(gif_stream_bound(sh.w, sh.h)) + (size_t)sh.w * sizeof(int4);
    }
    void trace(int n, const MixCut &cut) const
    {
        if (env_int("IPX_DEBUG_G2G", 0) != 0)
            fprintf(stderr, "[ipx] %s: %d files, %zu groups, %zu chunks, %zu runs\n", kWho, n, cut.groups.size(), cut.chunks.size(), cut.runs.size());
    }

    // ONE gif_decode_files call for every size of the group: the group's files are gathered for it, their verdicts go back
    int decode(const MixedCall &c, Lane &, hipStream_t s, const ipx_bytes *files, const int *idx, int m, Group &g)
    {
        std::vector<ipx_bytes> gfiles(m);
        std::vector<GifFileInfo> ginfo(m);
        std::vector<int> gstatus(m);
        for (int q = 0; q < m; q++) { gfiles[q] = files[idx[q]]; ginfo[q] = info[idx[q]]; gstatus[q] = c.status[idx[q]]; }
        g.at = gif_layout_packed(m, [&](int q) { return gstatus[q] == IPX_OK; }, [&](int q) { return (size_t)ginfo[q].w * ginfo[q].h; });
        IPX_HIP(g.mem.get(&g.dfr, g.at.bytes));
        IPX_HIP(g.mem.get(&g.dpal, (size_t)1024 * std::max(g.at.pal_slots, 1)));
        const int rc = gif_decode_files(c.ctx, s, gfiles.data(), m, ginfo, g.at, g.dfr, g.dpal, gstatus.data());
        for (int q = 0; q < m; q++) c.status[idx[q]] = gstatus[q];
        return rc;
    }
    // the frames from file i, which sits in slot `slot` of the group's layout, on: the files of its size that follow it lie one frame
    // stride apart, their palettes in the slots that follow
    BatchSrc src(const Group &g, int i, int slot) const
    {
        const GifFileInfo &f = info[i];
        return packed_src(kSrcPaletted, g.dfr + g.at.off[slot], f.w, align256((size_t)f.w * f.h), g.dpal + (size_t)g.at.pal_slot[slot] * 1024);
    }
    int chunk_memory(const MixedCall &c, Lane &, AsyncFree &omem, const int *file, int n, Chunk &b) const
    {
        size_t any = 0;
        for (int k = 0; k < kOuts; k++)
            if (const size_t total = b.lay(c, file, n, k, 0)) { IPX_HIP(omem.get(&b.base[k], total)); any += total; }
        size_t bytes = 0;
        b.coef_off.resize(n);
        for (int p = 0; p < n; p++) { b.coef_off[p] = bytes; if (c.has(file[p], kOutWm)) bytes += coef_bytes(c.shape(file[p], kOutWm)); }
        if (bytes) IPX_HIP(omem.get(&b.coefs, bytes));
        b.empty = !any;
        return IPX_OK;
    }
    // nothing per run: the chunk's frames are encoded together once its runs have all been through the operators
    int encode_run(const MixedCall &, hipStream_t, const int *, int, int, const Chunk &, ResultOwner &) const { return IPX_OK; }
    // ONE gif_encode_mixed_core over every present resize and thumbnail frame of the chunk's files that are still IPX_OK.  Then the
    // watermark frames as JPEG (watermark.go:73): when every file of the chunk is IPX_OK and has that output at one size, one
    // jpeg_encode_sets call over the chunk; else one jpeg_encode_mixed_core over the frames of the files that are IPX_OK.
    int encode_chunk(const MixedCall &c, hipStream_t s, const int *file, int n, const Chunk &b, ResultOwner &res) const
    {
        std::vector<GifMixSrc> gf;
        std::vector<std::pair<int, int>> owner_of;          // (file, output) of a frame
        for (int k : {kOutResize, kOutThumb})
            for (int p = 0; p < n; p++) {
                if (c.status[file[p]] != IPX_OK || !c.has(file[p], k)) continue;
                const OutShape sh = c.shape(file[p], k);
                gf.push_back(GifMixSrc{b.at(k, p), sh.w, sh.h, sh.w * 4});
                owner_of.emplace_back(file[p], k);
            }
        if (!gf.empty()) {
            std::vector<size_t> offs(gf.size()), lens(gf.size());
            uint8_t *blob = nullptr;
            const int rc = gif_encode_mixed_core(c.ctx, s, gf.data(), (int)gf.size(), &blob, offs.data(), lens.data());
            if (rc) return rc;
            res.add(blob);
            for (size_t j = 0; j < gf.size(); j++) c.publish(owner_of[j].first, owner_of[j].second, blob + offs[j], lens[j]);
        }
        bool uniform = true;
        std::vector<JpegEncSrc> jf;
        std::vector<int> jowner;
        for (int p = 0; p < n; p++) {
            const bool take = c.status[file[p]] == IPX_OK && c.has(file[p], kOutWm);
            uniform = uniform && take && c.shape(file[p], kOutWm).w == c.shape(file[0], kOutWm).w && c.shape(file[p], kOutWm).h == c.shape(file[0], kOutWm).h;
            if (!take) continue;
            const OutShape sh = c.shape(file[p], kOutWm);
            jf.push_back(JpegEncSrc{b.at(kOutWm, p), (int16_t *)(b.coefs + b.coef_off[p]), sh.w, sh.h, sh.w * 4});
            jowner.push_back(file[p]);
        }
        if (jf.empty()) return IPX_OK;
        std::vector<size_t> offs(jf.size()), lens(jf.size());
        uint8_t *blob = nullptr;
        int rc;
        if (uniform) {
            const OutShape sh = c.shape(file[0], kOutWm);
            const JpegEncSet set{(int16_t *)b.coefs, b.at(kOutWm, 0), sh.w, sh.h, sh.w * 4, c.out_fs(file[0], kOutWm), offs.data(), lens.data()};
            rc = jpeg_encode_sets(c.ctx, s, &set, 1, n, quality, &blob);
        } else {
            rc = jpeg_encode_mixed_core(c.ctx, s, jf.data(), (int)jf.size(), quality, &blob, offs.data(), lens.data());
        }
        if (rc) return rc;
        res.add(blob);
        for (size_t j = 0; j < jf.size(); j++) c.publish(jowner[j], kOutWm, blob + offs[j], lens[j]);
        return IPX_OK;
    }
};
}  // namespace

extern "C" int ipx_run_gif_gif_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                                     ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    GifMixed cx;
    cx.quality = quality;
    return mixed_leg(cx, ctx, ops, n, files, texts, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS
