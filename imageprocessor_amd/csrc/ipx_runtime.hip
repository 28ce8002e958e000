// ipx_runtime.hip -- a plan on a batch of frames: the one-pass kernel's launch (run_dev_any), the input side (BatchSrc: check, layout,
// upload, dispatch by source type) and the output side (BatchDst: direct stores or downloads) every batch leg shares, the pipelined host
// leg (run_host_packed) and the twelve pixel-out ipx_plan_run_* entries.  The context: ipx_context.hip; plans: ipx_plan.hip; the
// single-image operators the runner falls back on: ipx_image_ops.hip; the text: ipx_text.hip.  DESIGN.md section 4.11.
#include <chrono>

#include "ipx_runtime_internal.h"

#ifndef IPX_DIAG
#define IPX_DIAG 0
#endif

// what the compressed-in / compressed-out entries (ipx_jpeg_legs.hip, the PNG and GIF legs) check before anything else
int leg_entry_check(const char *who, const ipx_plan *pl, int n, const ipx_bytes *files, const int *status, ipx_jpeg_result **result,
                    bool texts_entry, const ipx_text *texts)
{
    const bool ok = pl && n >= 0 && files && status && result;
    if (ok) *result = nullptr;
    if (!ok || (texts_entry && !texts)) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    if (!texts_entry) return IPX_OK;
    if (pl->p.glyphs) {
        set_error("%s: the plan carries a glyph set of its own; per-file texts need a plan created with glyphs == NULL (copy only)", who);
        return IPX_ERR_INVALID;
    }
    return texts_check(who, texts, n);
}

// ---- one batch of decoded frames of any source type through a plan --------------------------------------------------------------------
// The one-pass kernel where it is built for the source type and the shapes; else per output: draw.Draw into the watermark frames
// (launch_draw*), the text, and one generic Scale per scaled output -- the crop thumbnail (thumbnail.go:128-131) reads the source
// through the `_CROP` tap kind of its type (ipx_ks.h), which is its 8-bit crop copy without the copy.
static hipError_t composite_text(const ipx_plan *pl, uint8_t *wm, size_t wm_frame_stride, int n, hipStream_t s)
{
    if (!wm || pl->glyphs.n <= 0 || !pl->p.glyphs) return hipSuccess;
    const uint8_t *c = pl->p.glyphs->col;
    return launch_composite(wm, pl->p.sw * 4, wm_frame_stride, n, pl->glyphs.dev, pl->glyphs.n, pl->glyphs.bbox, c[0] * 0x101u, c[1] * 0x101u,
                            c[2] * 0x101u, c[3] * 0x101u, s);
}

static int run_dev_any(ipx_ctx *ctx, hipStream_t s, const ipx_plan *pl, int n, const DevSrc &src, const BatchDst &dst)
{
    const int sw = pl->p.sw, sh = pl->p.sh;
    uint8_t *outs[2] = {pl->sc[0].on ? dst.out[kOutResize] : nullptr, pl->sc[1].on ? dst.out[kOutThumb] : nullptr};
    const size_t *ostr = dst.frame_stride;      // ([kOutResize], [kOutThumb]: the indices of pl->sc)
    uint8_t *wm = pl->p.do_watermark ? dst.out[kOutWm] : nullptr;
    const size_t wm_frame_stride = dst.frame_stride[kOutWm];
    for (int k = 0; k < 2; k++)
        if (pl->sc[k].dw <= 0 || pl->sc[k].dh <= 0) outs[k] = nullptr;
    if (!wm && !outs[0] && !outs[1]) return IPX_OK;
    int kinds[2] = {src.kind, pl->p.crop_to_fit ? ks_crop_kind(src.kind) : src.kind};

    const bool gray = src.kind == IPX_SRC_YCBCR && src.cstride == 0;
    const KsFusedPlan &fp = pl->fused[src.kind == IPX_SRC_RGBA ? 0 : gray ? 2 : 1];
    if (fp.ok && env_int("IPX_FUSED", 1)) {
        KsFusedArgs a{};
        a.src = src.pix; a.src_fs = src.frame_stride; a.sstride = src.stride; a.sw = sw; a.sh = sh;
        a.src_kind = src.kind; a.cb = src.cb; a.cr = src.cr; a.cstride = src.cstride; a.ratio = src.ratio; a.c_fs = src.c_frame_stride;
        a.wm = wm; a.wm_fs = wm_frame_stride; a.wm_stride = sw * 4;
        a.nframes = n;
        a.taps_le_alpha = src.le_alpha;
        for (int k = 0; k < 2; k++) {
            if (!outs[k]) continue;
            const PlanScale &ps = pl->sc[k];
            KsFusedOut &o = a.o[a.nout++];
            o.out = outs[k]; o.frame_stride = ostr[k]; o.ostride = ps.dw * 4; o.obytes = ps.dw * ps.dh * 4;
            o.dw = ps.dw; o.dh = ps.dh; o.sr_x0 = ps.sr.x0; o.sr_y0 = ps.sr.y0;
            o.kind = kinds[k]; o.pk = k;
        }
        // RGBA frames: the speculative opaque pass first (IPX_KS_SPEC=0: the general kernel alone), one flag per item.  RGBA, YCbCr and
        // Gray frames: the float pass (IPX_KS_FAST=0: float64 throughout) with a list per frame for the pixels it cannot decide --
        // 1 / 96 of the output's pixels each, twenty times what photographs put there (IPX_KS_STATS=1 prints the fill); a frame that fills
        // its list is redone in float64.
        // One stream-ordered block: [flags][counts][lists].
        AsyncFree mem{s, {}};
        int *redo = nullptr;
        KsFix fixv, *fix = nullptr;
        const int max_items = n * fp.nstrips * std::max(fp.whole.nseg, fp.split.nseg);
        const bool spec = src.kind == IPX_SRC_RGBA && env_int("IPX_KS_SPEC", 1);
        // (two more launches and a memset; measured faster than float64 throughout at every size from one 640x360 frame to 8K frames)
        const bool fast = (spec || src.kind == IPX_SRC_YCBCR || src.kind == IPX_SRC_NRGBA || (src.kind == IPX_SRC_TAP64 && src.le_alpha)) &&
                          env_int("IPX_KS_FAST", 1) != 0;
        if (spec || fast) {
            const int cap_env = env_int("IPX_KS_FIX_CAP", 0);     // test knob: tiny lists, so that frames fill them
            int cap[2] = {0, 0};
            for (int k = 0; k < 2; k++)
                if (fast && outs[k]) cap[k] = cap_env > 0 ? cap_env : (int)std::min<size_t>(std::max<size_t>((size_t)pl->sc[k].dw * pl->sc[k].dh / 96, 256), (size_t)1 << 20);
            const size_t flags = align256((size_t)max_items * sizeof(int)), counts = fast ? align256((size_t)n * 2 * sizeof(int)) : 0;
            IPX_HIP(mem.get(&redo, flags + counts + (size_t)n * (cap[0] + cap[1]) * sizeof(uint2)));
            if (fast) {
                fixv.count = (int *)((uint8_t *)redo + flags);
                fixv.list = (uint2 *)((uint8_t *)redo + flags + counts);
                fixv.cap[0] = cap[0]; fixv.cap[1] = cap[1];
                for (int k = 0; k < 2; k++) { fixv.ax[k] = pl->sc[k].ax[0]; fixv.ay[k] = pl->sc[k].ax[1]; }
                IPX_HIP(hipMemsetAsync(fixv.count, 0, (size_t)n * 2 * sizeof(int), s));
                fix = &fixv;
            }
        }
        a.redo = redo;
#if IPX_DIAG
        static unsigned long long *stamp_buf = nullptr;   // IPX_STAMPS=1: phase stamps, never in a timed run
        if (env_int("IPX_STAMPS", 0)) {
            if (!stamp_buf) IPX_HIP(hipMalloc((void **)&stamp_buf, 24 * sizeof(unsigned long long)));
            IPX_HIP(hipMemsetAsync(stamp_buf, 0, 24 * sizeof(unsigned long long), s));
            a.stamps = stamp_buf;
        }
#endif
        // the text goes along: behind a float pass it is part of the tail launch (ipx_ks_tail.hip) instead of a launch of its own
        KsText text{}, *txt = nullptr;
        if (wm && pl->glyphs.n > 0 && pl->p.glyphs) {
            const uint8_t *c = pl->p.glyphs->col;
            text = KsText{pl->glyphs.dev, pl->glyphs.n, pl->glyphs.bbox, c[0] * 0x101u, c[1] * 0x101u, c[2] * 0x101u, c[3] * 0x101u};
            txt = &text;
        }
        bool matched = false, text_done = false;
        hipError_t e = launch_ks_fused(fp, a, fix, txt, ctx->cus, s, &matched, &text_done);
        if (fix && matched && e == hipSuccess && env_int("IPX_KS_STATS", 0)) {   // diagnostic: how full the float pass's lists got, how many items went to float64
            // (only the items of the segmentation that ran have a flag: the block holds max_items of them and is not cleared)
            std::vector<int> cnt((size_t)n * 2), flags((size_t)n * a.nstrips * a.nseg);
            (void)hipMemcpyAsync(cnt.data(), fixv.count, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, s);
            (void)hipMemcpyAsync(flags.data(), redo, flags.size() * sizeof(int), hipMemcpyDeviceToHost, s);
            (void)hipStreamSynchronize(s);
            long long tot[2] = {0, 0}; int mx[2] = {0, 0}, nredo = 0;
            for (int i = 0; i < n; i++) for (int k = 0; k < 2; k++) { tot[k] += cnt[2 * i + k]; mx[k] = std::max(mx[k], cnt[2 * i + k]); }
            for (int f : flags) nredo += f != 0;
            fprintf(stderr, "[ipx ks stats] %d frames: undecided pixels per frame resize mean %.1f max %d (room %d), thumbnail mean %.1f max %d (room %d); %d of %d items redone in float64\n", n,
                    (double)tot[0] / n, mx[0], fixv.cap[0], (double)tot[1] / n, mx[1], fixv.cap[1], nredo, (int)flags.size());
        }
#if IPX_DIAG
        if (a.stamps && matched) {
            unsigned long long h[24];
            IPX_HIP(hipMemcpyAsync(h, a.stamps, sizeof h, hipMemcpyDeviceToHost, s));
            IPX_HIP(hipStreamSynchronize(s));
            const char *who[3] = {"resize waves", "thumbnail waves", "idle waves"};
            for (int r = 0; r < 3; r++) {
                double tot = 0;
                for (int i = 0; i < 6; i++) tot += (double)h[r * 8 + i];
                if (tot > 0)
                    fprintf(stderr, "[ipx stamps] %-16s share of wave time: wait-loads %.1f%%  drain %.1f%%  barrier %.1f%%  issue %.1f%%  scaleX %.1f%%  scaleY %.1f%%  (%.3g cycles)\n", who[r],
                            100 * h[r * 8] / tot, 100 * h[r * 8 + 1] / tot, 100 * h[r * 8 + 2] / tot, 100 * h[r * 8 + 3] / tot, 100 * h[r * 8 + 4] / tot, 100 * h[r * 8 + 5] / tot, tot);
            }
        }
#endif
        if (e != hipSuccess) { set_error("one-pass kernel launch failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
        if (matched) {
            if (!text_done) IPX_HIP(composite_text(pl, wm, wm_frame_stride, n, s));   // no float pass (no lists), or IPX_KS_TAIL=0
            return IPX_OK;
        }
    }

    if (wm) {   // draw.Draw(result, bounds, img, ZP, draw.Src) for the batch
        const int rc = dev_draw_src(s, wm, sw, sh, sw * 4, Rect{0, 0, sw, sh}, src, 0, 0, IPX_OP_SRC, wm_frame_stride);
        if (rc) return rc;
        IPX_HIP(composite_text(pl, wm, wm_frame_stride, n, s));
    }
    for (int k = 0; k < 2; k++) {   // Over onto the zeroed frame of image.NewRGBA == Src
        if (!outs[k]) continue;
        const PlanScale &ps = pl->sc[k];
        const int rc = dev_scale_src(ctx, s, nullptr, outs[k], ps.dw, ps.dh, ps.dw * 4, Rect{0, 0, ps.dw, ps.dh}, src, ps.sr, IPX_OP_SRC, ostr[k],
                                     kinds[k], ps.ax);
        if (rc) return rc;
    }
    return IPX_OK;
}

// ---- the input side of the plan entries: one description of a source batch (BatchSrc), checked, laid out, uploaded and dispatched here ----

int src_check(const char *who, const ipx_plan *pl, const BatchSrc &b, int n, bool in_hbm)
{
    if (b.type < 0 || b.type >= kSrcTypes) { set_error("%s: unknown source type", who); return IPX_ERR_INVALID; }
    const int bpp = src_bpp(b.type);
    bool ok = pl && n >= 0 && b.plane[0] && (long long)b.stride[0] >= (long long)pl->p.sw * bpp;
    if (ok && b.type == kSrcYCbCr) {
        int cw = 0, ch = 0;
        chroma_size(b.ratio, pl->p.sw, pl->p.sh, &cw, &ch);
        ok = b.plane[1] && b.plane[2] && ycbcr_ratio_ok(b.ratio) && b.stride[1] >= cw;
    }
    if (ok && b.type == kSrcPaletted) ok = b.palettes && !(in_hbm && ((uintptr_t)b.palettes & 3));
    if (ok && in_hbm && b.type >= kSrcNRGBA64)       // the expansion reads whole 16-bit samples (CMYK: whole pixels)
        ok = !(((uintptr_t)b.plane[0] | (uintptr_t)b.stride[0] | b.frame_stride[0]) & (b.type == kSrcCMYK ? 3 : 1));
    if (!ok) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    const int sw = pl->p.sw, sh = pl->p.sh;
    if (!frame_span_ok(sw, sh, b.stride[0], bpp) || (b.type == kSrcYCbCr && !frame_span_ok(sw, sh, b.stride[1], 1)) ||
        (b.type >= kSrcNRGBA64 && !frame_span_ok(sw, sh, (long long)sw * 8, 8))) {
        set_error("%s: %dx%d frames with row strides of %d / %d bytes are beyond the 2 GiB span the kernels address", who, sw, sh, b.stride[0], b.stride[1]);
        return IPX_ERR_UNSUPPORTED;
    }
    if (in_hbm && n > 65535) { set_error("%s: at most 65535 frames per call", who); return IPX_ERR_UNSUPPORTED; }
    return IPX_OK;
}

SrcLayout src_layout(const ipx_plan *pl, const BatchSrc &b, size_t (*frame_rule)(size_t))
{
    SrcLayout L{};
    int cw = 0, ch = 0;
    if (b.type == kSrcYCbCr) chroma_size(b.ratio, pl->p.sw, pl->p.sh, &cw, &ch);
    L.planes = b.type == kSrcYCbCr ? 3 : 1;
    L.row[0] = (size_t)pl->p.sw * src_bpp(b.type); L.h[0] = pl->p.sh; L.fs[0] = frame_rule(L.row[0] * L.h[0]);
    L.row[1] = cw; L.h[1] = ch; L.fs[1] = frame_rule((size_t)cw * ch);
    L.pal = b.type == kSrcPaletted ? 1024 : 0;
    return L;
}

hipError_t src_upload(const BatchSrc &host, const SrcLayout &L, int i0, int m, uint8_t *scratch, int slots, hipStream_t s, const CopyPolicy &cp,
                      BatchSrc *in_hbm)
{
    *in_hbm = host;
    hipError_t e = hipSuccess;
    uint8_t *d = scratch;
    for (int p = 0; p < L.planes && e == hipSuccess; p++) {
        const int k = p ? 1 : 0;
        const size_t row = L.row[k], dfs = L.fs[k], hfs = host.frame_stride[k], bytes = dfs * m;
        const uint8_t *h = host.plane[p] + hfs * i0;
        const bool tight_rows = (size_t)host.stride[k] == row;
        if (cp.join_frames && tight_rows && hfs == dfs) {
            const size_t piece = cp.piece ? cp.piece : bytes;
            for (size_t o = 0; o < bytes && e == hipSuccess; o += piece) e = hipMemcpyAsync(d + o, h + o, std::min(piece, bytes - o), hipMemcpyHostToDevice, s);
        } else {
            for (int i = 0; i < m && e == hipSuccess; i++)
                e = cp.join_rows && tight_rows ? hipMemcpyAsync(d + dfs * i, h + hfs * i, row * L.h[k], hipMemcpyHostToDevice, s)
                                               : hipMemcpy2DAsync(d + dfs * i, row, h + hfs * i, host.stride[k], row, L.h[k], hipMemcpyHostToDevice, s);
        }
        in_hbm->plane[p] = d; in_hbm->stride[k] = (int)row; in_hbm->frame_stride[k] = dfs;
        d += dfs * slots;
    }
    if (L.pal && e == hipSuccess) {
        e = hipMemcpyAsync(d, host.palettes + L.pal * i0, L.pal * m, hipMemcpyHostToDevice, s);
        in_hbm->palettes = d;
    }
    return e;
}

int run_dev_src(ipx_ctx *ctx, hipStream_t s, const ipx_plan *pl, int m, const BatchSrc &b, const BatchDst &dst)
{
    // (a leg's chunk size may come from an environment knob: the limit of one launch is held here too)
    if (m > 65535) { set_error("at most 65535 frames per device call"); return IPX_ERR_UNSUPPORTED; }
    const int sw = pl->p.sw, sh = pl->p.sh;
    AsyncFree mem{s, {}};
    DevSrc d;
    d.pix = b.plane[0]; d.stride = b.stride[0]; d.frame_stride = b.frame_stride[0]; d.w = sw; d.h = sh; d.nframes = m;
    switch (b.type) {
    case kSrcRGBA: break;
    case kSrcNRGBA: d.kind = IPX_SRC_NRGBA; break;
    case kSrcYCbCr:
        d.kind = IPX_SRC_YCBCR; d.cb = b.plane[1]; d.cr = b.plane[2]; d.cstride = b.stride[1]; d.ratio = b.ratio; d.c_frame_stride = b.frame_stride[1];
        break;
    case kSrcGray:
        // scaleX_Gray / drawGray read a pixel as (y, y, y, 0xff), tmp alpha 1.  A YCbCr pixel with Cb = Cr = 128 converts to exactly that in both of the
        // reference's conversions -- color.YCbCrToRGB: (y*0x10101) >> 16 = y; color.YCbCr.RGBA: (y*0x10101) >> 8 = y*0x101 = color.Gray.RGBA -- and
        // scaleX_YCbCr4xx writes the same tmp alpha, so the batch runs as 4:4:4 planes with a stride-0 row of 128s as both chroma planes.
        if ((size_t)sw + 8 > ipx_ctx::kFlatChromaBytes) { set_error("Gray frames wider than %zu pixels", ipx_ctx::kFlatChromaBytes - 8); return IPX_ERR_UNSUPPORTED; }
        d.kind = IPX_SRC_YCBCR; d.cb = d.cr = ctx->flat_chroma; d.ratio = IPX_YCBCR_444;
        break;
    case kSrcPaletted: {    // Paletted.At(x, y) is the palette's color.NRGBA: one expansion pass, then the NRGBA route
        const size_t fs = align256((size_t)sw * sh * 4);
        uint8_t *nrgba = nullptr;
        IPX_HIP(mem.get(&nrgba, fs * m));
        const hipError_t e = launch_palette_expand(nrgba, fs, b.plane[0], b.stride[0], b.frame_stride[0], b.palettes, sw, sh, m, s);
        if (e != hipSuccess) { set_error("palette expansion failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
        d.kind = IPX_SRC_NRGBA; d.pix = nrgba; d.stride = sw * 4; d.frame_stride = fs;
        break;
    }
    default: {
        // The deep source types: one expansion pass to frames of 16-bit taps (what every consumer of these types reads: At(x, y).RGBA()), then
        // the batch runner on them: top bytes into the watermark frames (drawRGBA / drawCMYK with Src), the scales from the taps.
        const size_t tfs = align256((size_t)sw * sh * 8);
        uint8_t *taps = nullptr;
        IPX_HIP(mem.get(&taps, tfs * m));
        const hipError_t e = launch_deep_expand(taps, tfs, b.plane[0], b.stride[0], b.frame_stride[0], b.type - kSrcNRGBA64, sw, sh, m, s);
        if (e != hipSuccess) { set_error("tap expansion failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
        d.kind = IPX_SRC_TAP64; d.pix = taps; d.stride = sw * 8; d.frame_stride = tfs;
        d.le_alpha = b.type != kSrcRGBA64;     // (a premultiplied RGBA64 file may hold a colour above its alpha; the others cannot)
        break;
    }
    }
    return run_dev_any(ctx, s, pl, m, d, dst);
}

// an entry on frames in HBM: the check, then the operators on the caller's stream (null: the context's)
static int run_dev_entry(const char *who, ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, const BatchSrc &b, const BatchDst &dst)
{
    const int rc = src_check(who, pl, b, n, true);
    if (rc) return rc;
    for (int k = 0; k < kOuts; k++) IPX_DEV_OUT(who, out_shape(pl->info, k).name, dst.out[k], 0, dst.frame_stride[k]);
    if (n == 0) return rc;
    return run_dev_src(ctx, stream ? (hipStream_t)stream : ctx->stream, pl, n, b, dst);
}

// ---- the output side of the pixel-out host legs: one description of a batch's outputs (BatchDst), laid out in scratch, stored into by
// the kernels themselves where they can (dst_direct), downloaded where they cannot ----

bool dst_direct(const DstLayout &L, const BatchDst &host, int m, BatchDst *view)
{
    *view = BatchDst{};
    bool direct = env_int("IPX_HOST_DIRECT", 1) != 0;
    for (int k = 0; k < kOuts; k++)
        if (L.bytes[k] && (((uintptr_t)host.out[k] | host.frame_stride[k]) & 15)) direct = false;
    for (int k = 0; k < kOuts && direct; k++) {
        if (!L.bytes[k]) continue;
        view->out[k] = pinned_device_view(host.out[k], host.frame_stride[k] * (m - 1) + L.bytes[k]);
        view->frame_stride[k] = host.frame_stride[k];
        direct = view->out[k] != nullptr;
    }
    return direct;
}

hipError_t dst_download(const BatchDst &host, const BatchDst &dev, const DstLayout &L, int i0, int m, hipStream_t s, const CopyPolicy &cp)
{
    hipError_t e = hipSuccess;
    auto frame = [&](int k, int i) {
        return hipMemcpyAsync(host.out[k] + (size_t)(i0 + i) * host.frame_stride[k], dev.out[k] + dev.frame_stride[k] * i, L.bytes[k], hipMemcpyDeviceToHost, s);
    };
    if (!cp.join_frames) {
        for (int i = 0; i < m; i++)
            for (int k = 0; k < kOuts && e == hipSuccess; k++)
                if (L.bytes[k]) e = frame(k, i);
        return e;
    }
    for (int k = 0; k < kOuts && e == hipSuccess; k++) {
        const size_t hs = host.frame_stride[k], ds = dev.frame_stride[k];
        if (!L.bytes[k]) continue;
        if (hs == ds && (L.bytes[k] == ds || m == 1)) {   // tight on both sides: the chunk as one run of bytes (equal strides with a gap: the gap is the caller's)
            const size_t bytes = ds * (m - 1) + L.bytes[k], piece = cp.piece ? cp.piece : bytes;
            for (size_t o = 0; o < bytes && e == hipSuccess; o += piece)
                e = hipMemcpyAsync(host.out[k] + (size_t)i0 * hs + o, dev.out[k] + o, std::min(piece, bytes - o), hipMemcpyDeviceToHost, s);
        } else {
            for (int i = 0; i < m && e == hipSuccess; i++) e = frame(k, i);
        }
    }
    return e;
}

// device-side frame strides of run_host_packed: tight when that keeps rows 16-byte aligned (then a whole chunk moves with one copy per
// direction and buffer), padded to 256 otherwise
static size_t tight16_or_align256(size_t bytes) { return (bytes & 15) == 0 ? bytes : align256(bytes); }

// Frames in host memory, any single-plane source type: chunks over the lanes so that H2D of one chunk, the kernel of another and D2H of
// a third overlap.
static int run_host_packed(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const BatchSrc &host, const BatchDst &dst)
{
    int rc = src_check(who, pl, host, n, false);
    if (rc || n == 0) return rc;
    const SrcLayout L = src_layout(pl, host, tight16_or_align256);
    const DstLayout D(pl, dst, tight16_or_align256);
    const size_t fsrc = L.frame_bytes();       // (the palette included)
    const size_t per_frame = fsrc + D.frame_bytes();
    // chunk the batch so that H2D of one chunk, the kernel of another and D2H of a third overlap on
    // different lanes (one stream each); several chunks per lane keep all three engines busy
    const int nl = (int)ctx->lanes.size();
    int chunk = std::max(1, (n + 4 * nl - 1) / (4 * nl));
    chunk = (int)std::min<size_t>((size_t)chunk, std::max<size_t>(1, ctx->lane_bytes / per_frame));
    chunk = std::max(1, std::min(chunk, env_int("IPX_HOST_CHUNK", 16)));

    // This call is the pipeline: it takes the lanes -- all but one when the context has three or more, so that a single-frame call
    // (the per-operator seam: one chunk, one lane) is served WHILE a batch runs instead of behind it; a call of one chunk takes one.
    const int nchunks = (n + chunk - 1) / chunk;
    const int want = nchunks <= 1 ? 1 : std::max(1, nl >= 3 ? nl - 1 : nl);
    std::vector<Lane *> lanes;
    const bool trace = want == 1 && env_int("IPX_DEBUG_SEAM", 0);
    const auto t_in = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
    {
        std::unique_lock<std::mutex> lk(ctx->mu);
        auto free_lanes = [&] { int k = 0; for (auto &l : ctx->lanes) k += !l.busy; return k; };
        ctx->cv.wait(lk, [&] { return free_lanes() >= want; });
        if (want == 1) {   // a single chunk: the last free lane (the high-priority one when it is free)
            for (size_t i = ctx->lanes.size(); i-- > 0;) if (!ctx->lanes[i].busy) { ctx->lanes[i].busy = true; lanes.push_back(&ctx->lanes[i]); break; }
        } else {
            for (auto &l : ctx->lanes) if (!l.busy && (int)lanes.size() < want) { l.busy = true; lanes.push_back(&l); }
        }
    }
    hipError_t e = hipSuccess;
    const double t_lock = trace ? ms_since(t_in) : 0;
    for (auto *l : lanes) {
        rc = lane_reserve(*l, per_frame * chunk + 256);
        if (rc) break;
    }
    const double t_res = trace ? ms_since(t_in) : 0;
    // A single small frame in PAGEABLE memory (the per-operator seam from a caller that does not pin): the runtime's staged path for
    // small pageable copies blocks the enqueueing thread behind other streams' work every few contexts (a 640x360 call then takes as
    // long as the batch running beside it; tools/seam_hunt.py), larger ones it pins on the fly and never did.  Such a call goes
    // through a pinned bounce buffer of its lane instead: two host memcpys of < 1 ms.
    bool bounce = false;
    if (!rc && nchunks == 1 && n == 1 && !L.pal && per_frame <= ((size_t)8 << 20)) {
        hipPointerAttribute_t at;
        const bool pinned = hipPointerGetAttributes(&at, host.plane[0]) == hipSuccess && at.type == hipMemoryTypeHost;
        (void)hipGetLastError();
        if (!pinned) {
            Lane &l = *lanes[0];
            if (l.pin_bytes < per_frame) {
                if (l.pin) (void)hipHostFree(l.pin);
                l.pin = nullptr; l.pin_bytes = 0;
                if (hipHostMalloc((void **)&l.pin, per_frame + (per_frame >> 2), hipHostMallocDefault) == hipSuccess) l.pin_bytes = per_frame + (per_frame >> 2);
                else (void)hipGetLastError();
            }
            bounce = l.pin != nullptr;
        }
    }
    // The host link moves both directions at once only when uploads and downloads sit on streams of their own AND go in pieces: the
    // runtime picks a copy engine per hipMemcpyAsync, and two large copies enqueued together share one (tools/link_streams.py,
    // ipx_link_probe: 2 x 512 MiB as single copies 28.7 + 28.7 GB/s, in 32 MiB pieces 47.9 + 47.9).  So the call is a three-stage
    // pipeline over the lanes it took: every upload on the first lane's stream, every kernel on the third's, every download on the
    // second's, the lanes' scratch buffers as the slots chunks rotate through, events between the stages.
    const size_t piece = (size_t)std::max(1, env_int("IPX_COPY_PIECE_MB", 32)) << 20;
    const CopyPolicy join_policy{true, false, piece};
    // Outputs in pinned memory are written by the kernels themselves (dst_direct): uploads are then the only copies in flight, so the
    // two directions cannot land on one engine, and a chunk has two stages instead of three.
    BatchDst view;
    const bool direct = !bounce && dst_direct(D, dst, n, &view);
    if (getenv("IPX_KS_DEBUG")) fprintf(stderr, "[ipx host] outputs %s\n", direct ? "stored by the kernels" : "copied from scratch");
    const size_t S = lanes.size();
    const hipStream_t s_up = lanes[0]->stream, s_down = lanes[S > 1 ? 1 : 0]->stream, s_run = lanes[S > 2 ? 2 : 0]->stream;
    const bool staged = S > 1 && env_int("IPX_HOST_STAGED", 1) != 0;
    if (staged)
        for (auto *l : lanes)
            for (auto &ev : l->ev)
                if (!ev && e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    for (int i0 = 0, c = 0; !rc && e == hipSuccess && i0 < n; i0 += chunk, c++) {
        Lane &l = *lanes[c % S];
        const hipStream_t up = staged ? s_up : l.stream, run = staged ? s_run : l.stream, down = staged ? s_down : l.stream;
        const int m = std::min(chunk, n - i0);
        uint8_t *dsrc = (uint8_t *)(((uintptr_t)l.dev + 255) & ~(uintptr_t)255);
        const BatchDst dout = direct ? view.from(i0) : D.place(dsrc + fsrc * chunk, chunk);
        // reuse of a lane's scratch: chunk c waits until chunk c - S has been downloaded (stream order when one stream does it all)
        if (staged && c >= (int)S) e = hipStreamWaitEvent(up, l.ev[2], 0);
        if (e != hipSuccess) break;
        BatchSrc d;
        if (bounce) {
            for (int y = 0; y < L.h[0]; y++) memcpy(l.pin + y * L.row[0], host.plane[0] + (size_t)y * host.stride[0], L.row[0]);
            e = hipMemcpyAsync(dsrc, l.pin, L.row[0] * L.h[0], hipMemcpyHostToDevice, up);
            d = packed_src(host.type, dsrc, (int)L.row[0], L.fs[0]);
        } else {
            e = src_upload(host, L, i0, m, dsrc, chunk, up, join_policy, &d);
        }
        if (e == hipSuccess && staged) e = hipEventRecord(l.ev[0], up);
        if (e == hipSuccess && staged) e = hipStreamWaitEvent(run, l.ev[0], 0);
        if (e != hipSuccess) break;
        rc = run_dev_src(ctx, run, pl, m, d, dout);
        if (rc) break;
        if (direct) {          // the outputs are where they belong when the kernels have finished
            if (staged) e = hipEventRecord(l.ev[2], run);
            continue;
        }
        if (staged) {
            e = hipEventRecord(l.ev[1], run);
            if (e == hipSuccess) e = hipStreamWaitEvent(down, l.ev[1], 0);
            if (e != hipSuccess) break;
        }
        if (bounce) {          // one copy of the three outputs (they follow the source in the lane's scratch), handed out after the sync below
            if (D.frame_bytes()) e = hipMemcpyAsync(l.pin + fsrc, dsrc + fsrc, D.frame_bytes(), hipMemcpyDeviceToHost, down);
            continue;
        }
        e = dst_download(dst, dout, D, i0, m, down, join_policy);
        if (e == hipSuccess && staged) e = hipEventRecord(l.ev[2], down);
    }
    const double t_enq = trace ? ms_since(t_in) : 0;
    for (auto *l : lanes) {
        hipError_t e2 = hipStreamSynchronize(l->stream);
        if (e == hipSuccess) e = e2;
    }
    if (bounce && !rc && e == hipSuccess) {
        const BatchDst p = D.place(lanes[0]->pin + fsrc, 1);
        for (int k = 0; k < kOuts; k++)
            if (p.out[k]) memcpy(dst.out[k], p.out[k], D.bytes[k]);
    }
    if (trace)
        fprintf(stderr, "[ipx seam] lane %d of %d: lock %.2f ms, reserve %.2f, enqueued %.2f, done %.2f\n", (int)(lanes[0] - &ctx->lanes[0]), nl, t_lock, t_res,
                t_enq, ms_since(t_in));
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto *l : lanes) l->busy = false;
    }
    ctx->cv.notify_all();
    if (!rc && e != hipSuccess) { set_error("%s: %s", who, hipGetErrorString(e)); rc = IPX_ERR_HIP; }
    return rc;
}

extern "C" {

// The twelve pixel-out batch entries: each describes its source (BatchSrc) and its outputs (BatchDst, abi_dst) and hands them on --
// frames in HBM to run_dev_entry, frames in host memory to run_host_packed (YCbCr planes: the entry's own single-lane schedule), which
// check them by the one rule (src_check).  The alignment the kernels need of a deep type's pixels and of palettes is asked of HBM
// sources only: host frames are re-packed into aligned scratch on their way up.

int ipx_plan_run_dev(ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                     uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                     size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_dev_entry("ipx_plan_run_dev", ctx, stream, pl, n, packed_src(kSrcRGBA, src, sstride, src_frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_host(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                      uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                      size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_host_packed("ipx_plan_run_host", ctx, pl, n, packed_src(kSrcRGBA, src, sstride, src_frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_dev_nrgba(ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                           uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                           size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_dev_entry("ipx_plan_run_dev_nrgba", ctx, stream, pl, n, packed_src(kSrcNRGBA, src, sstride, src_frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_host_nrgba(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                            uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                            size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_host_packed("ipx_plan_run_host_nrgba", ctx, pl, n, packed_src(kSrcNRGBA, src, sstride, src_frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_dev_gray(ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, const uint8_t *gray, int stride, size_t frame_stride,
                          uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                          size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_dev_entry("ipx_plan_run_dev_gray", ctx, stream, pl, n, packed_src(kSrcGray, gray, stride, frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_host_gray(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *gray, int stride, size_t frame_stride,
                           uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                           size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_host_packed("ipx_plan_run_host_gray", ctx, pl, n, packed_src(kSrcGray, gray, stride, frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_dev_paletted(ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, const uint8_t *index, int stride, size_t frame_stride,
                              const uint8_t *palettes,
                              uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                              size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_dev_entry("ipx_plan_run_dev_paletted", ctx, stream, pl, n, packed_src(kSrcPaletted, index, stride, frame_stride, palettes),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_host_paletted(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *index, int stride, size_t frame_stride,
                               const uint8_t *palettes,
                               uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                               size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_host_packed("ipx_plan_run_host_paletted", ctx, pl, n, packed_src(kSrcPaletted, index, stride, frame_stride, palettes),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_dev_deep(ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, int kind, const uint8_t *src, int sstride, size_t src_frame_stride,
                          uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                          size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_dev_entry("ipx_plan_run_dev_deep", ctx, stream, pl, n, packed_src(src_of_deep(kind), src, sstride, src_frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

int ipx_plan_run_host_deep(ipx_ctx *ctx, const ipx_plan *pl, int n, int kind, const uint8_t *src, int sstride, size_t src_frame_stride,
                           uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                           size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_host_packed("ipx_plan_run_host_deep", ctx, pl, n, packed_src(src_of_deep(kind), src, sstride, src_frame_stride),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

// ---- decoded JPEG batches ---------------------------------------------------------------------------
// The reference treats a *image.YCbCr source differently per operator: resize and the non-crop thumbnail convert
// every tap to 16 bit and then interpolate; the crop thumbnail scales an RGBA8 copy; the watermark is drawn on an RGBA8 conversion.  All
// three are arms of the one-pass kernel (or of the per-output kernels behind it) chosen by tap kind in run_dev_any: IPX_SRC_YCBCR for
// the first, its _CROP kind for the second, the draw of the source into the watermark frames for the third.
int ipx_plan_run_dev_ycbcr(ipx_ctx *ctx, void *stream, const ipx_plan *pl, int n, const ipx_ycbcr_batch *src,
                           uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                           size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    return run_dev_entry("ipx_plan_run_dev_ycbcr", ctx, stream, pl, n, ycbcr_src(src),
                           abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride));
}
IPX_CATCH_STATUS

// One leased lane and one stream: every frame up, the operators, every output down.  (Not the pipeline of run_host_packed.)
int ipx_plan_run_host_ycbcr(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_ycbcr_batch *src,
                            uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                            size_t wm_frame_stride) try
{
    IPX_ENTER(ctx);
    const BatchSrc host = ycbcr_src(src);
    int rc = src_check("ipx_plan_run_host_ycbcr", pl, host, n, false);
    if (rc || n == 0) return rc;
    const BatchDst dst = abi_dst(resize_out, resize_frame_stride, thumb_out, thumb_frame_stride, wm_out, wm_frame_stride);
    const SrcLayout L = src_layout(pl, host);
    const DstLayout D(pl, dst);
    LaneLease lane(ctx);
    rc = lane_reserve(lane.get(), (L.frame_bytes() + D.frame_bytes()) * n + 1024);
    if (rc) return rc;
    hipStream_t s = lane->stream;
    const BatchDst dout = D.place(lane->dev + L.frame_bytes() * n, n);
    BatchSrc d;
    // (from the first queued copy on, no way out before the stream has been waited for: the copies read and write the caller's memory)
    hipError_t e = src_upload(host, L, 0, n, lane->dev, n, s, kCopyFrameRows, &d);
    if (e == hipSuccess) rc = run_dev_src(ctx, s, pl, n, d, dout);
    if (e == hipSuccess && !rc) e = dst_download(dst, dout, D, 0, n, s, kCopyFrames);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (!rc && e != hipSuccess) { set_error("ipx_plan_run_host_ycbcr: %s", hipGetErrorString(e)); rc = IPX_ERR_HIP; }
    return rc;
}
IPX_CATCH_STATUS

}  // extern "C"
