// ipx_png_dec_runtime.hip -- the driver of png.Decode for batches of files and the ABI entries built on it: the host parse of every
// file (ipx_png_dec_host.cpp), then png_decode_files: the upload, the CRC, the inflate and the unfilter of a selection of files of any
// sizes and kinds, into the frame and palette blocks a PngFrameLayout (ipx_png_layout.h) describes.  Kernels: ipx_png_dec.hip,
// ipx_png_dec_par.hip; the compressed-in, compressed-out legs on top of this: ipx_png_legs.hip.  DESIGN.md section 4.10.
#include <numeric>
#include <vector>

#include "ipx_png_dec.h"
#include "ipx_decode_common.h"

// ---- the decode core -------------------------------------------------------------------------------------------------------------

// parse n files (a thread per eight of them); status[i] from the container.  IPX_PNG_ADAM7=1 in the environment, read on every call,
// lets Adam7 files through to the GPU; anything else keeps them UNSUPPORTED.
int png_parse_all(const ipx_bytes *files, int n, std::vector<PngFileInfo> &info, int *status)
{
    const bool adam7 = env_int("IPX_PNG_ADAM7", 0) == 1;
    return parallel_light(n, [&](int i) { status[i] = png_parse(files[i].data, files[i].data ? files[i].len : 0, adam7, &info[i]); }, "png decode: host parse failed");
}

namespace {
constexpr uint32_t kCrcPiece = 16384;

// the batch's size and kind: *w x *h (or the first parsed file's when *w == 0) and *kind (or the first's when -1); others UNSUPPORTED
void png_select(const std::vector<PngFileInfo> &info, int n, int *w, int *h, int *kind, int *status)
{
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        if (*w <= 0) { *w = info[i].w; *h = info[i].h; }
        if (*kind < 0 && info[i].w == *w && info[i].h == *h) *kind = info[i].kind;
        if (info[i].w != *w || info[i].h != *h || info[i].kind != *kind) status[i] = IPX_ERR_UNSUPPORTED;
    }
}

size_t png_group_bytes(const PngFileInfo &f) { return align256(f.file_len) + align256(f.idat_len + 32) + align256(f.raw_len); }
}  // namespace

// Decodes files[at.idx[g]] (status IPX_OK, of any sizes and kinds: the kernels read everything from the file's descriptor) into
// frames + at.off[g] and, when palettes is set, the palette of a file with at.pal_slot[g] >= 0 to palettes + at.pal_slot[g] * 1024, on
// stream s; the verdicts land in status[at.idx[g]].  All of them go through the same launches.  The scratch (the files' pinned upload
// block and, in HBM, the files, zlib streams, filtered rows and tables) is cut into groups of at most IPX_PNG_DEC_SCRATCH_MB, and each
// group's scratch is released before the next group takes its own; one read-back of the per-file words at the end.
int png_decode_files(ipx_ctx *ctx, hipStream_t s, const ipx_bytes *files, const PngFrameLayout &at, const std::vector<PngFileInfo> &info,
                     uint8_t *frames, uint8_t *palettes, int *status)
{
    const std::vector<int> &idx = at.idx;
    const int n = (int)idx.size();
    if (n == 0) return IPX_OK;
    PinnedBlocks pinned(ctx, s);
    AsyncFree mem{s, {}};
    // IPX_PNG_PAR=1 in the environment, read on every call: the inflate is png_inflate_par_kernel with the serial decoder behind it for
    // the files it leaves; anything else keeps the serial kernel alone.  IPX_PNG_PAR_SUB: its sub-sequence size in bits (tests).
    const bool par = env_int("IPX_PNG_PAR", 0) == 1;
    const uint32_t par_sub = (uint32_t)std::min(kPngParSubMax, std::max(kPngParSubMin, env_int("IPX_PNG_PAR_SUB", kPngParSub)));
    const size_t words = par ? (size_t)n * 3 : (size_t)n;        // the status words, then the parallel kernel's word pairs
    uint32_t *dstate;
    IPX_HIP(mem.get(&dstate, words * 4));
    IPX_HIP(hipMemsetAsync(dstate, 0, words * 4, s));
    uint32_t *dpar = dstate + n;
    const int npal = at.pal_slots;
    if (palettes && npal > 0) {     // one upload of every slot up to the last (zero for slots not decoded here)
        uint8_t *hpal = pinned.get((size_t)npal * 1024);
        if (!hpal) return IPX_ERR_NOMEM;
        memset(hpal, 0, (size_t)npal * 1024);
        for (int g = 0; g < n; g++)
            if (at.pal_slot[g] >= 0) memcpy(hpal + (size_t)at.pal_slot[g] * 1024, info[idx[g]].pal, 1024);
        IPX_HIP(hipMemcpyAsync(palettes, hpal, (size_t)npal * 1024, hipMemcpyHostToDevice, s));
    }
    const size_t budget = (size_t)env_int("IPX_PNG_DEC_SCRATCH_MB", 8192) << 20;
    auto run_group = [&](const std::vector<int> &group) -> int {     // positions in idx
        const int m = (int)group.size();
        // this group's scratch: the device blocks go back (stream-ordered) first, then the pinned block once the stream is past its copy
        PinnedBlocks gpinned(ctx, s);
        AsyncFree gmem{s, {}};
        std::vector<PngDecDesc> desc(m);
        std::vector<PngCrcPiece> pieces;
        std::vector<PngChunk> chunks;
        std::vector<size_t> foff(m);
        size_t fbytes = 0, zbytes = 0, rbytes = 0;
        for (int g = 0; g < m; g++) {
            const PngFileInfo &f = info[idx[group[g]]];
            PngDecDesc &d = desc[g];
            memset(&d, 0, sizeof d);
            foff[g] = fbytes;
            d.zoff = zbytes;
            d.roff = rbytes;
            d.foff = (uint64_t)at.off[group[g]];
            d.zlen = f.idat_len;
            d.zlast = f.idat_last;
            d.raw_len = (uint32_t)f.raw_len;
            d.w = (uint32_t)f.w;
            d.h = (uint32_t)f.h;
            d.rowbytes = f.rowbytes;
            d.slot = (uint32_t)group[g];
            d.ctype = (uint16_t)f.ctype;
            d.depth = (uint16_t)f.depth;
            d.kind = (uint16_t)f.kind;
            d.trns = f.trns ? 1 : 0;
            for (int k = 0; k < 3; k++) d.tv[k] = f.trns_v[k];
            d.bpp = (uint16_t)f.bpp;
            d.interlace = f.interlace ? 1 : 0;
            // the chunks' CRC pieces; IDAT payloads land back to back at zoff
            size_t zat = zbytes;
            uint32_t ii = 0;
            for (const PngSpan &c : f.crc) {
                const uint32_t k = (uint32_t)chunks.size();
                chunks.push_back(PngChunk{foff[g] + c.off, c.len, (uint32_t)group[g]});
                const bool is_idat = ii < f.idat.size() && f.idat[ii].off == c.off + 4;
                for (uint32_t p0 = 0; p0 < c.len; p0 += kCrcPiece) {
                    const uint32_t p1 = std::min(c.len, p0 + kCrcPiece);
                    PngCrcPiece pc;
                    pc.src = foff[g] + c.off + p0;
                    pc.len = p1 - p0;
                    pc.chunk = k;
                    pc.after = c.len - p1;
                    pc.skip = p0 < 4 ? 4 - p0 : 0;
                    pc.dst = is_idat && pc.len > pc.skip ? zat + (p0 + pc.skip - 4) : ~0ull;
                    pieces.push_back(pc);
                }
                if (is_idat) { zat += f.idat[ii].len; ii++; }
            }
            fbytes += align256(f.file_len);
            zbytes += align256((size_t)f.idat_len + 32);
            rbytes += align256(f.raw_len);
        }
        uint8_t *hblob = gpinned.get(fbytes);
        if (!hblob) return IPX_ERR_NOMEM;
        const int rc = parallel_light(m, [&](int g) {
            const int i = idx[group[g]];
            memcpy(hblob + foff[g], files[i].data, info[i].file_len);
        }, "png decode: host gather failed");
        if (rc) return rc;
        // the Adam7 files' descriptors go behind the others: each unfilter kernel takes its own run of the table
        const int m0 = (int)(std::stable_partition(desc.begin(), desc.end(), [](const PngDecDesc &d) { return !d.interlace; }) - desc.begin());
        uint8_t *dblob, *dz, *draw;
        uint32_t *dacc;
        PngCrcPiece *dpieces;
        PngChunk *dchunks;
        PngDecDesc *ddesc;
        IPX_HIP(gmem.get(&dblob, fbytes));
        IPX_HIP(gmem.get(&dz, zbytes));
        IPX_HIP(gmem.get(&draw, rbytes));
        IPX_HIP(gmem.get(&dacc, chunks.size() * 4));
        IPX_HIP(gmem.get(&dpieces, pieces.size() * sizeof(PngCrcPiece)));
        IPX_HIP(gmem.get(&dchunks, chunks.size() * sizeof(PngChunk)));
        IPX_HIP(gmem.get(&ddesc, (size_t)m * sizeof(PngDecDesc)));
        IPX_HIP(hipMemcpyAsync(dblob, hblob, fbytes, hipMemcpyHostToDevice, s));
        IPX_HIP(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(PngCrcPiece), hipMemcpyHostToDevice, s));
        IPX_HIP(hipMemcpyAsync(dchunks, chunks.data(), chunks.size() * sizeof(PngChunk), hipMemcpyHostToDevice, s));
        IPX_HIP(hipMemcpyAsync(ddesc, desc.data(), (size_t)m * sizeof(PngDecDesc), hipMemcpyHostToDevice, s));
        IPX_HIP(hipMemsetAsync(dacc, 0, chunks.size() * 4, s));
        IPX_HIP(launch_png_crc(dblob, dpieces, (int)pieces.size(), dacc, dz, s));
        IPX_HIP(launch_png_crc_check(dblob, dchunks, (int)chunks.size(), dacc, dstate, s));
        if (par) {
            IPX_HIP(launch_png_inflate_par(dz, ddesc, m, draw, dstate, dpar, par_sub, s));
            IPX_HIP(launch_png_inflate_redo(dz, ddesc, m, draw, dstate, dpar, s));
        } else {
            IPX_HIP(launch_png_inflate(dz, ddesc, m, draw, dstate, s));
        }
        IPX_HIP(launch_png_unfilter(ddesc, m0, draw, frames, dstate, s));
        IPX_HIP(launch_png_unfilter_adam7(ddesc + m0, m - m0, draw, frames, dstate, s));
        // the host vectors must outlive the copies: wait before they go
        IPX_HIP(hipStreamSynchronize(s));
        return IPX_OK;
    };
    std::vector<int> all(n);
    std::iota(all.begin(), all.end(), 0);
    const int rc = for_groups_under(all, budget, [&](int g) { return png_group_bytes(info[idx[g]]); }, run_group);
    if (rc) return rc;
    std::vector<uint32_t> st(words);
    IPX_HIP(hipMemcpyAsync(st.data(), dstate, words * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    if (par) {                                                   // ipx_png_decode_counts
        long long c[5] = {n, 0, 0, 0, 0};
        for (int g = 0; g < n; g++) {
            const uint32_t a = st[n + 2 * g], b = st[n + 2 * g + 1];
            if (b & kPngParRedo) { c[2]++; continue; }
            c[1]++;
            c[3] += a;
            c[4] += b;
        }
        for (int k = 0; k < 5; k++) ctx->png_counts[k] += c[k];
    }
    for (int g = 0; g < n; g++) {
        const uint32_t v = st[g];
        status[idx[g]] = v == 0 ? IPX_OK : (v & ~kPngTrailing) ? IPX_ERR_INVALID : IPX_ERR_UNSUPPORTED;
    }
    return IPX_OK;
}

// ---- the entries -----------------------------------------------------------------------------------------------------------------
extern "C" {

int ipx_png_decode_counts(ipx_ctx *ctx, long long counts[5])
{
    clear_error();
    if (!ctx || !counts) { set_error("ipx_png_decode_counts: bad argument"); return IPX_ERR_INVALID; }
    for (int k = 0; k < 5; k++) counts[k] = ctx->png_counts[k].load();
    return IPX_OK;
}

void ipx_png_frames_free(ipx_ctx *ctx, ipx_png_frames *o) { dev_blocks_free(ctx, o); }

int ipx_png_decode_batch(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, int *w, int *h, int *kind, ipx_png_batch *frames,
                         int *status, ipx_png_frames **owner) try
{
    IPX_ENTER(ctx);
    if (!files || n < 0 || !w || !h || !kind || !frames || !status || !owner || *w < 0 || *h < 0 || (*w == 0) != (*h == 0) ||
        *kind < -1 || *kind >= kPngKinds) {
        set_error("ipx_png_decode_batch: bad argument");
        return IPX_ERR_INVALID;
    }
    *owner = nullptr;
    memset(frames, 0, sizeof *frames);
    if (n == 0) return IPX_OK;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<PngFileInfo> info(n);
    int rc = png_parse_all(files, n, info, status);
    if (rc) return rc;
    int bw = *w, bh = *h, bk = *kind;
    png_select(info, n, &bw, &bh, &bk, status);
    std::vector<int> idx;
    for (int i = 0; i < n; i++)
        if (status[i] == IPX_OK) idx.push_back(i);
    if (idx.empty()) return IPX_OK;
    OwnedBlocks<ipx_png_frames> o(ctx, s);
    const int kb = png_kind_bpp(bk);
    const size_t fs = align256((size_t)bw * bh * kb);
    uint8_t *dframes = nullptr, *dpal = nullptr;
    hipError_t e = o.alloc(&dframes, fs * n);
    if (e == hipSuccess && bk == IPX_PNG_PALETTED) e = o.alloc(&dpal, (size_t)n * 1024);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("ipx_png_decode_batch: device allocation failed: %s", hipGetErrorString(e));
        return IPX_ERR_NOMEM;
    }
    if (dpal) IPX_HIP(hipMemsetAsync(dpal, 0, (size_t)n * 1024, s));
    rc = png_decode_files(ctx, s, files, png_layout_strided(std::move(idx), fs, true), info, dframes, dpal, status);     // frame i of file i
    if (rc) return rc;
    *w = bw;
    *h = bh;
    *kind = bk;
    if (!any_ok(status, n)) return IPX_OK;
    frames->pix = dframes;
    frames->stride = bw * kb;
    frames->frame_stride = fs;
    frames->palettes = dpal;
    *owner = o.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

// n files of any sizes and kinds: every file that parses goes through ONE png_decode_files call, its frame at an offset of its own in
// one block (256-byte aligned, rows tight) and, for a paletted file, its palette in the next free slot of a second block
int ipx_png_decode_mixed(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, ipx_png_frame *frames, int *status,
                         ipx_png_frames **owner) try
{
    IPX_ENTER(ctx);
    if (n < 0 || !owner || (n && (!files || !frames || !status))) { set_error("ipx_png_decode_mixed: bad argument"); return IPX_ERR_INVALID; }
    *owner = nullptr;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_png_decode_mixed: at most 65535 files per call"); return IPX_ERR_UNSUPPORTED; }
    memset(frames, 0, (size_t)n * sizeof *frames);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    std::vector<PngFileInfo> info(n);
    int rc = png_parse_all(files, n, info, status);
    if (rc) return rc;
    std::vector<int> idx;
    for (int i = 0; i < n; i++)
        if (status[i] == IPX_OK) idx.push_back(i);
    if (idx.empty()) return IPX_OK;
    const PngFrameLayout at = png_layout_packed(std::move(idx), [&](int i) { return png_frame_need(info[i]); });
    OwnedBlocks<ipx_png_frames> o(ctx, s);
    uint8_t *dframes = nullptr, *dpal = nullptr;
    hipError_t e = o.alloc(&dframes, at.bytes);
    if (e == hipSuccess && at.pal_slots) e = o.alloc(&dpal, (size_t)at.pal_slots * 1024);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("ipx_png_decode_mixed: device allocation failed: %s", hipGetErrorString(e));
        return IPX_ERR_NOMEM;
    }
    rc = png_decode_files(ctx, s, files, at, info, dframes, dpal, status);
    if (rc) return rc;
    if (!any_ok(status, n)) return IPX_OK;
    for (size_t g = 0; g < at.idx.size(); g++) {
        const int i = at.idx[g];
        if (status[i] != IPX_OK) continue;
        const PngFileInfo &f = info[i];
        frames[i] = ipx_png_frame{f.w, f.h, f.kind, dframes + at.off[g], f.w * png_kind_bpp(f.kind),
                                  at.pal_slot[g] >= 0 ? dpal + (size_t)at.pal_slot[g] * 1024 : nullptr};
    }
    *owner = o.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

}  // extern "C"
