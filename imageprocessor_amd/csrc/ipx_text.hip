// ipx_text.hip -- the watermark text: glyph sets (one text, clipped per frame size and cached) and text sets (one text per frame of a
// batch), their clipping and packing, and the entries that composite them.  Kernels: ipx_kernels.hip.
#include <new>

#include "ipx_runtime_internal.h"

namespace {

// image/draw's clipping of each glyph's dr against a dw x dh frame and its mask, mp moved with it (draw_clip): the surviving glyphs
// are appended to *tab with their masks at masks_dev + mask_off; returns their bounding box (all zeros when none survives).  The one
// clipper of glyph sets (glyphs_for_frame) and text sets (textset_build).
Rect clip_glyphs(const GlyphHost *g, size_t n, const uint8_t *masks_dev, int dw, int dh, std::vector<DevGlyph> *tab)
{
    Rect bb{0, 0, 0, 0};
    const size_t before = tab->size();
    for (size_t i = 0; i < n; i++) {
        Rect r = g[i].dr;
        int spx = 0, spy = 0, mpx = g[i].mpx, mpy = g[i].mpy;
        if (!draw_clip(r, dw, dh, false, 0, 0, spx, spy, true, g[i].mw, g[i].mh, mpx, mpy)) continue;
        DevGlyph d;
        d.mask = masks_dev + g[i].mask_off + (size_t)mpy * g[i].mw + mpx;
        d.mstride = g[i].mw;
        d.x0 = r.x0; d.y0 = r.y0; d.x1 = r.x1; d.y1 = r.y1;
        if (tab->size() == before) bb = r;
        else {
            bb.x0 = std::min(bb.x0, r.x0); bb.y0 = std::min(bb.y0, r.y0);
            bb.x1 = std::max(bb.x1, r.x1); bb.y1 = std::max(bb.y1, r.y1);
        }
        tab->push_back(d);
    }
    return bb;
}

// one glyph of the ABI into the packed blob (rows tight): false for a bad mask
bool pack_glyph(const ipx_glyph &g, std::vector<uint8_t> *blob, GlyphHost *h)
{
    if (g.mw < 0 || g.mh < 0 || (g.mw && g.mh && (!g.mask || g.mstride < g.mw))) return false;
    h->mask_off = blob->size();
    h->mw = g.mw; h->mh = g.mh; h->dr = to_rect(g.dr); h->mpx = g.mpx; h->mpy = g.mpy;
    for (int y = 0; y < g.mh; y++) blob->insert(blob->end(), g.mask + (size_t)y * g.mstride, g.mask + (size_t)y * g.mstride + g.mw);
    return true;
}

}  // namespace

int glyphs_for_frame(const ipx_glyphset *gs, int dw, int dh, ClippedGlyphs *out)
{
    std::lock_guard<std::mutex> lk(gs->mu);
    auto it = gs->clipped.find({dw, dh});
    if (it != gs->clipped.end()) { *out = it->second; return IPX_OK; }
    std::vector<DevGlyph> tab;
    const Rect bb = clip_glyphs(gs->g.data(), gs->g.size(), gs->masks_dev, dw, dh, &tab);
    ClippedGlyphs c;
    c.n = (int)tab.size();
    c.bbox = bb;
    if (c.n) {
        IPX_HIP(hipMalloc((void **)&c.dev, tab.size() * sizeof(DevGlyph)));
        IPX_HIP(hipMemcpy(c.dev, tab.data(), tab.size() * sizeof(DevGlyph), hipMemcpyHostToDevice));
    }
    gs->clipped[{dw, dh}] = c;
    *out = c;
    return IPX_OK;
}

static int dev_composite(hipStream_t s, uint8_t *dst, int dw, int dh, int dstride, size_t frame_stride,
                         int nframes, const ipx_glyphset *gs)
{
    ClippedGlyphs c;
    int rc = glyphs_for_frame(gs, dw, dh, &c);
    if (rc) return rc;
    IPX_HIP(launch_composite(dst, dstride, frame_stride, nframes, c.dev, c.n, c.bbox,
                             gs->col[0] * 0x101u, gs->col[1] * 0x101u, gs->col[2] * 0x101u,
                             gs->col[3] * 0x101u, s));
    return IPX_OK;
}

// ---- text sets: one text per frame of a batch -------------------------------------------------------------
int texts_check(const char *who, const ipx_text *texts, int n)
{
    if (n < 0 || (n && !texts)) { set_error("%s: bad text list", who); return IPX_ERR_INVALID; }
    for (int t = 0; t < n; t++) {
        const ipx_text &x = texts[t];
        if (x.n_glyphs < 0 || (x.n_glyphs && !x.glyphs)) { set_error("%s: text %d has a bad glyph list", who, t); return IPX_ERR_INVALID; }
        if (x.n_glyphs > kMaxGlyphs) { set_error("%s: text %d has %d glyphs, the limit is %d", who, t, x.n_glyphs, kMaxGlyphs); return IPX_ERR_UNSUPPORTED; }
        for (int i = 0; i < x.n_glyphs; i++) {
            const ipx_glyph &g = x.glyphs[i];
            if (g.mw < 0 || g.mh < 0 || (g.mw && g.mh && (!g.mask || g.mstride < g.mw))) { set_error("%s: glyph %d of text %d has a bad mask", who, i, t); return IPX_ERR_INVALID; }
        }
    }
    return IPX_OK;
}

int textset_build(hipStream_t s, const char *who, const ipx_text *texts, int n, int w, int h, ipx_textset *ts)
{
    int rc = texts_check(who, texts, n);
    if (rc) return rc;
    if (w < 0 || h < 0) { set_error("%s: bad frame size", who); return IPX_ERR_INVALID; }
    std::vector<uint8_t> blob;
    std::vector<GlyphHost> gh;
    std::vector<int> start(n + 1, 0);
    for (int t = 0; t < n; t++) {
        for (int i = 0; i < texts[t].n_glyphs; i++) {
            GlyphHost g;
            (void)pack_glyph(texts[t].glyphs[i], &blob, &g);      // (texts_check has seen the masks)
            gh.push_back(g);
        }
        start[t + 1] = (int)gh.size();
    }
    ts->mem.s = s;
    ts->w = w; ts->h = h; ts->n = n;
    uint8_t *masks_dev = nullptr;
    IPX_HIP(ts->mem.get(&masks_dev, blob.size()));
    std::vector<DevGlyph> tab;
    std::vector<DevText> desc(n);
    ts->bbox.assign(n, Rect{0, 0, 0, 0});
    for (int t = 0; t < n; t++) {
        DevText &d = desc[t];
        d.first = (int)tab.size();
        d.bbox = ts->bbox[t] = clip_glyphs(gh.data() + start[t], (size_t)(start[t + 1] - start[t]), masks_dev, w, h, &tab);
        d.n = (int)tab.size() - d.first;
        for (int c = 0; c < 4; c++) d.col[c] = (uint16_t)(texts[t].col[c] * 0x101u);
    }
    IPX_HIP(ts->mem.get(&ts->glyphs_dev, tab.size() * sizeof(DevGlyph)));
    IPX_HIP(ts->mem.get(&ts->texts_dev, desc.size() * sizeof(DevText)));
    if (!blob.empty()) IPX_HIP(hipMemcpyAsync(masks_dev, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    if (!tab.empty()) IPX_HIP(hipMemcpyAsync(ts->glyphs_dev, tab.data(), tab.size() * sizeof(DevGlyph), hipMemcpyHostToDevice, s));
    if (!desc.empty()) IPX_HIP(hipMemcpyAsync(ts->texts_dev, desc.data(), desc.size() * sizeof(DevText), hipMemcpyHostToDevice, s));
    IPX_HIP(hipStreamSynchronize(s));
    return IPX_OK;
}

int dev_composite_texts(hipStream_t s, AsyncFree *mem, uint8_t *dst, int dstride, size_t frame_stride, int n_frames, const ipx_textset &ts,
                        int first, const int *map)
{
    if (n_frames <= 0) return IPX_OK;
    if (!map && (first < 0 || (long long)first + n_frames > ts.n)) {
        set_error("composite texts: frames %d .. %lld of a set of %d texts", first, (long long)first + n_frames, ts.n);
        return IPX_ERR_INVALID;
    }
    int bw = 0, bh = 0;
    for (int z = 0; z < n_frames; z++) {
        const int t = map ? map[z] : first + z;
        if (t < 0 || t >= ts.n) { set_error("composite texts: frame %d names text %d of %d", z, t, ts.n); return IPX_ERR_INVALID; }
        const Rect &b = ts.bbox[t];
        if (b.empty()) continue;
        bw = std::max(bw, b.dx()); bh = std::max(bh, b.dy());
    }
    if (!bw || !bh) return IPX_OK;
    int *map_dev = nullptr;
    if (map) {
        if (!mem) { set_error("composite texts: a frame-to-text map needs scratch"); return IPX_ERR_INVALID; }
        IPX_HIP(mem->get(&map_dev, (size_t)n_frames * sizeof(int)));
        IPX_HIP(hipMemcpyAsync(map_dev, map, (size_t)n_frames * sizeof(int), hipMemcpyHostToDevice, s));
    }
    for (int z0 = 0; z0 < n_frames; z0 += 65535)       // (the grid's z)
        IPX_HIP(launch_composite_texts(dst + (size_t)z0 * frame_stride, dstride, frame_stride, std::min(65535, n_frames - z0), ts.texts_dev,
                                       ts.glyphs_dev, map_dev ? map_dev + z0 : nullptr, first + z0, bw, bh, s));
    return IPX_OK;
}

// =============================================================================================
extern "C" {

int ipx_glyphset_create(ipx_ctx *ctx, const ipx_glyph *glyphs, int n, const uint8_t col[4],
                        ipx_glyphset **out) try
{
    IPX_ENTER(ctx);
    if (!out || n < 0 || (n && !glyphs) || !col) { set_error("ipx_glyphset_create: bad argument"); return IPX_ERR_INVALID; }
    if (n > kMaxGlyphs) { set_error("ipx_glyphset_create: %d glyphs exceed the limit of %d", n, kMaxGlyphs); return IPX_ERR_UNSUPPORTED; }
    *out = nullptr;
    ipx_glyphset *gs = new (std::nothrow) ipx_glyphset;
    if (!gs) { set_error("out of memory"); return IPX_ERR_NOMEM; }
    gs->device = ctx->device;
    memcpy(gs->col, col, 4);
    std::vector<uint8_t> blob;
    for (int i = 0; i < n; i++) {
        const ipx_glyph &g = glyphs[i];
        GlyphHost h;
        if (!pack_glyph(g, &blob, &h)) {
            set_error("ipx_glyphset_create: glyph %d has a bad mask", i);
            delete gs;
            return IPX_ERR_INVALID;
        }
        gs->g.push_back(h);
    }
    gs->masks_bytes = blob.size();
    if (!blob.empty()) {
        hipError_t e = hipMalloc((void **)&gs->masks_dev, blob.size());
        if (e == hipSuccess) e = hipMemcpy(gs->masks_dev, blob.data(), blob.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("glyph mask upload failed: %s", hipGetErrorString(e));
            ipx_glyphset_destroy(ctx, gs);
            return IPX_ERR_HIP;
        }
    }
    *out = gs;
    return IPX_OK;
}
IPX_CATCH_STATUS

void ipx_glyphset_destroy(ipx_ctx *ctx, ipx_glyphset *gs)
{
    if (!gs) return;
    (void)hipSetDevice(ctx ? ctx->device : gs->device);
    for (auto &kv : gs->clipped) if (kv.second.dev) (void)hipFree(kv.second.dev);
    if (gs->masks_dev) (void)hipFree(gs->masks_dev);
    delete gs;
}

int ipx_dev_composite_glyphs_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int dw, int dh,
                                   int dstride, const ipx_glyphset *gs) try
{
    IPX_ENTER(ctx);
    if (!gs) { set_error("ipx_dev_composite_glyphs_rgba8: bad argument"); return IPX_ERR_INVALID; }
    IPX_FRAME("ipx_dev_composite_glyphs_rgba8", "destination", dst, dw, dh, dstride);
    IPX_DEV_OUT("ipx_dev_composite_glyphs_rgba8", "destination", dst, (unsigned)dstride);
    return dev_composite(stream ? (hipStream_t)stream : ctx->stream, dst, dw, dh, dstride, 0, 1, gs);
}
IPX_CATCH_STATUS

int ipx_textset_create(ipx_ctx *ctx, void *stream, const ipx_text *texts, int n, int w, int h, ipx_textset **out) try
{
    IPX_ENTER(ctx);
    if (!out) { set_error("ipx_textset_create: bad argument"); return IPX_ERR_INVALID; }
    *out = nullptr;
    ipx_textset *ts = new (std::nothrow) ipx_textset;
    if (!ts) { set_error("out of memory"); return IPX_ERR_NOMEM; }
    ts->device = ctx->device;
    const int rc = textset_build(stream ? (hipStream_t)stream : ctx->stream, "ipx_textset_create", texts, n, w, h, ts);
    if (rc) { delete ts; return rc; }
    *out = ts;
    return IPX_OK;
}
IPX_CATCH_STATUS

void ipx_textset_destroy(ipx_ctx *ctx, ipx_textset *ts)
{
    if (!ts) return;
    (void)hipSetDevice(ctx ? ctx->device : ts->device);
    delete ts;       // (its memory is freed in the order of the stream it was created on)
}

int ipx_dev_composite_texts_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int w, int h, int dstride, size_t frame_stride, int n_frames,
                                  const ipx_textset *ts, int first, const int32_t *map) try
{
    IPX_ENTER(ctx);
    if (!ts || n_frames < 0) { set_error("ipx_dev_composite_texts_rgba8: bad argument"); return IPX_ERR_INVALID; }
    if (w != ts->w || h != ts->h) { set_error("ipx_dev_composite_texts_rgba8: the text set was clipped for %dx%d frames, not %dx%d", ts->w, ts->h, w, h); return IPX_ERR_INVALID; }
    IPX_FRAME("ipx_dev_composite_texts_rgba8", "destination", dst, w, h, dstride);
    IPX_DEV_OUT("ipx_dev_composite_texts_rgba8", "destination", dst, (unsigned)dstride, frame_stride);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    AsyncFree mem{s, {}};
    const int rc = dev_composite_texts(s, &mem, dst, dstride, frame_stride, n_frames, *ts, first, (const int *)map);
    if (map) (void)hipStreamSynchronize(s);     // the caller's map is read by a copy on the stream: done with it on return
    return rc;
}
IPX_CATCH_STATUS

// host pointers: staged through a lane with a glyph set that lives for the call (no source: the lane's scratch holds the frame alone)
int ipx_composite_glyphs_rgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride,
                               const ipx_glyph *glyphs, int n, const uint8_t col[4]) try
{
    IPX_ENTER(ctx);
    // deliberate ABI behaviour: the glyph list and the colour are judged before the frame, and a bad mask only behind the early-out
    if (n < 0 || (n && !glyphs) || !col) { set_error("ipx_composite_glyphs_rgba8: bad argument"); return IPX_ERR_INVALID; }
    IPX_FRAME("ipx_composite_glyphs_rgba8", "destination", dst, dw, dh, dstride);
    if (!n || !dw || !dh) return IPX_OK;
    ipx_glyphset *gs = nullptr;
    int rc = ipx_glyphset_create(ctx, glyphs, n, col, &gs);
    if (rc) return rc;
    rc = stage_and_run(ctx, dst, dw, dh, dstride, 0, [&](hipStream_t s, int *, uint8_t *ddst, uint8_t *) -> int {
        return dev_composite(s, ddst, dw, dh, dw * 4, 0, 1, gs);
    });
    ipx_glyphset_destroy(ctx, gs);
    return rc;
}
IPX_CATCH_STATUS

}  // extern "C"
