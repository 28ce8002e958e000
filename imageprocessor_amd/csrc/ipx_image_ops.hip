// ipx_image_ops.hip -- the single-image operators: xdraw.BiLinear.Scale and draw.Draw on one frame of any source type, on frames in
// HBM (dev_scale_src, dev_draw_src: the batch runner of ipx_runtime.hip falls back on them too) and, staged through a lane's scratch,
// on frames in host memory.  Kernels: ipx_kernels.hip, ipx_ks_generic.hip.
#include "ipx_runtime_internal.h"

namespace {

// Scale's argument checks, shared by host- and device-pointer entries (kernelScaler.Scale's preamble: adr, empty rectangles)
struct ScalePrep {
    bool empty;
    Rect adr;       // relative to dr.Min
};

int scale_prepare(int dw, int dh, const Rect &dr, int sw, int sh, const Rect &sr, int op, ScalePrep *o)
{
    if (op != IPX_OP_OVER && op != IPX_OP_SRC) { set_error("scale: unknown op %d", op); return IPX_ERR_INVALID; }
    o->empty = false;
    Rect adr = Rect{0, 0, dw, dh}.intersect(dr);
    if (adr.empty() || sr.empty() || dr.dx() <= 0 || dr.dy() <= 0) { o->empty = true; return IPX_OK; }
    if (sr.x0 < 0 || sr.y0 < 0 || sr.x1 > sw || sr.y1 > sh) {
        set_error("scale: source rectangle (%d,%d)-(%d,%d) leaves the %dx%d source; the reference's "
                  "generic Image path is not covered", sr.x0, sr.y0, sr.x1, sr.y1, sw, sh);
        return IPX_ERR_UNSUPPORTED;
    }
    o->adr = adr.shifted(-dr.x0, -dr.y0);
    return IPX_OK;
}

// One axis of the kernel scaler (newDistrib for dw destination and sw source indices) resident in HBM, by (dw, sw): the per-operation
// seam sees the same few geometries over and over.  Entries live until the context does; past kMaxKsAxes the cache is flushed after a
// device-wide wait (launches in flight hold raw pointers into it).
constexpr size_t kMaxKsAxes = 512;
int ks_axis_get(ipx_ctx *ctx, int dw, int sw, KsAxisDev *out)
{
    std::lock_guard<std::mutex> lk(ctx->ks_mu);
    auto it = ctx->ks_axes.find({dw, sw});
    if (it != ctx->ks_axes.end()) { *out = it->second.second; return IPX_OK; }
    KsAxis ax;
    if (!ks_build_axis(dw, sw, &ax)) { set_error("scale: cannot tabulate an axis of %d <- %d", dw, sw); return IPX_ERR_INVALID; }
    if (ctx->ks_axes.size() >= kMaxKsAxes) {
        IPX_HIP(hipDeviceSynchronize());
        for (auto &e : ctx->ks_axes) (void)hipFree(e.second.first);
        ctx->ks_axes.clear();
    }
    const size_t bytes = ks_axis_bytes(ax);
    std::vector<uint8_t> h(bytes);
    uint8_t *d = nullptr;
    IPX_HIP(hipMalloc((void **)&d, bytes));
    KsAxisDev dev;
    ks_axis_pack(ax, h.data(), d, &dev);
    hipError_t e = hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); set_error("axis table upload failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
    ctx->ks_axes[{dw, sw}] = {d, dev};
    *out = dev;
    return IPX_OK;
}

DevSrc rgba_src(const uint8_t *p, int w, int h, int stride, int kind = IPX_SRC_RGBA)
{
    DevSrc d;
    d.kind = kind; d.pix = p; d.stride = stride; d.w = w; d.h = h;
    return d;
}

}  // namespace

int dev_draw_src(hipStream_t s, uint8_t *dst, int dw, int dh, int dstride, Rect r, const DevSrc &src, int spx,
                 int spy, int op, size_t dst_fs)
{
    if (op != IPX_OP_OVER && op != IPX_OP_SRC) { set_error("draw: unknown op %d", op); return IPX_ERR_INVALID; }
    int mx = 0, my = 0;
    if (!draw_clip(r, dw, dh, true, src.w, src.h, spx, spy, false, 0, 0, mx, my)) return IPX_OK;
    uint8_t *d = dst + (size_t)r.y0 * dstride + (size_t)r.x0 * 4;
    if (src.kind == IPX_SRC_YCBCR)   // opaque source: Over == Src (image/draw.DrawMask's YCbCr arm)
        IPX_HIP(launch_draw_ycbcr(d, dstride, src.pix, src.stride, src.cb, src.cr, src.cstride, src.ratio, spx, spy,
                                  r.dx(), r.dy(), s, src.nframes, dst_fs, src.frame_stride, src.c_frame_stride));
    else if (src.kind == IPX_SRC_NRGBA)
        IPX_HIP(launch_draw_nrgba(d, dstride, src.pix + (size_t)spy * src.stride + (size_t)spx * 4, src.stride, r.dx(),
                                  r.dy(), op, s, src.nframes, dst_fs, src.frame_stride));
    else if (src.kind == IPX_SRC_TAP64)
        IPX_HIP(launch_draw_tap64(d, dstride, src.pix + (size_t)spy * src.stride + (size_t)spx * 8, src.stride, r.dx(), r.dy(), op, s,
                                  src.nframes, dst_fs, src.frame_stride));
    else
        for (int i = 0; i < std::max(1, src.nframes); i++)
            IPX_HIP(launch_draw(d + (size_t)i * dst_fs, dstride, src.pix + (size_t)i * src.frame_stride + (size_t)spy * src.stride + (size_t)spx * 4,
                                src.stride, r.dx(), r.dy(), op, s));
    return IPX_OK;
}

int dev_scale_src(ipx_ctx *ctx, hipStream_t s, int *flag, uint8_t *dst, int dw, int dh, int dstride, const Rect &dr,
                  const DevSrc &src, const Rect &sr, int op, size_t dst_fs, int kind_override, const KsAxisDev *axes)
{
    ScalePrep pr;
    int rc = scale_prepare(dw, dh, dr, src.w, src.h, sr, op, &pr);
    if (rc) return rc;
    if (pr.empty) return IPX_OK;
    if (src.kind == IPX_SRC_YCBCR) op = IPX_OP_SRC;   // (*image.YCbCr).Opaque() is always true
    if (op == IPX_OP_OVER && src.kind == IPX_SRC_TAP64) IPX_HIP(launch_opaque_scan_tap64(src.pix, src.w, src.h, src.stride, flag, s));
    else if (op == IPX_OP_OVER) IPX_HIP(launch_opaque_scan(src.pix, src.w, src.h, src.stride, flag, s));  // RGBA and NRGBA: alpha scan
    KsGenArgs a{};
    if (axes) { a.ax = axes[0]; a.ay = axes[1]; }
    else {
        if ((rc = ks_axis_get(ctx, dr.dx(), sr.dx(), &a.ax))) return rc;
        if ((rc = ks_axis_get(ctx, dr.dy(), sr.dy(), &a.ay))) return rc;
    }
    a.dst = dst; a.dstride = dstride; a.src = src.pix; a.sstride = src.stride;
    a.dr_x0 = dr.x0; a.dr_y0 = dr.y0;
    a.adr_x0 = pr.adr.x0; a.adr_y0 = pr.adr.y0; a.adr_x1 = pr.adr.x1; a.adr_y1 = pr.adr.y1;
    a.sr_x0 = sr.x0; a.sr_y0 = sr.y0;
    a.op = op; a.opaque_flag = op == IPX_OP_OVER ? flag : nullptr;
    a.kind = kind_override >= 0 ? kind_override : src.kind;
    a.cb = src.cb; a.cr = src.cr; a.cstride = src.cstride; a.ratio = src.ratio;
    a.nframes = src.nframes; a.src_fs = src.frame_stride; a.c_fs = src.c_frame_stride; a.dst_fs = dst_fs;
    IPX_HIP(launch_ks_generic(a, s));
    return IPX_OK;
}

// ---- host pointers: one frame of each source type, staged through a lane (stage_and_run) -----------------------------------------------
// A source type is a host frame that knows its argument checks, the scratch it needs and how it goes up: check() is what both entries
// of the type ask first, upload() queues the copies (and the expansion) and describes the frame in HBM.
namespace {

struct HostPacked {      // RGBA / NRGBA pixels: one 2-D copy
    const uint8_t *pix; int w, h, stride, kind;
    int check(const char *who, const void *dst, int dw, int dh, int dstride) const
    {
        IPX_FRAME(who, "destination", dst, dw, dh, dstride);
        IPX_FRAME(who, "source", pix, w, h, stride);
        return IPX_OK;
    }
    size_t bytes() const { return align256((size_t)w * h * 4); }
    int upload(hipStream_t s, uint8_t *dsrc, DevSrc *out) const
    {
        IPX_HIP(hipMemcpy2DAsync(dsrc, (size_t)w * 4, pix, stride, (size_t)w * 4, h, hipMemcpyHostToDevice, s));
        *out = rgba_src(dsrc, w, h, w * 4, kind);
        return IPX_OK;
    }
};

struct HostDeep {        // a deep frame -> a frame of taps in the lane's scratch (the Pix copy sits behind it)
    const uint8_t *pix; int w, h, stride, kind;
    int check(const char *who, const void *dst, int dw, int dh, int dstride) const
    {
        if (src_of_deep(kind) < 0) { set_error("%s: unknown source type %d", who, kind); return IPX_ERR_INVALID; }   // deliberate ABI behaviour: the kind before the frames
        int rc = frame_status(who, "destination", dst, dw, dh, dstride);
        if (!rc) rc = frame_status(who, "source", pix, w, h, stride, src_bpp(src_of_deep(kind)));
        if (!rc) rc = frame_status(who, "source", pix, w, h, (long long)w * 8, 8);       // the frame of taps
        return rc;
    }
    size_t bytes() const { return align256((size_t)w * h * 8) * 2; }
    int upload(hipStream_t s, uint8_t *dsrc, DevSrc *out) const
    {
        const int bpp = src_bpp(src_of_deep(kind));
        uint8_t *raw = dsrc + align256((size_t)w * h * 8);
        IPX_HIP(hipMemcpy2DAsync(raw, (size_t)w * bpp, pix, stride, (size_t)w * bpp, h, hipMemcpyHostToDevice, s));
        IPX_HIP(launch_deep_expand(dsrc, 0, raw, w * bpp, 0, kind, w, h, 1, s));
        out->kind = IPX_SRC_TAP64; out->pix = dsrc; out->stride = w * 8; out->w = w; out->h = h;
        return IPX_OK;
    }
};

struct HostYCbCr {       // three planes
    const ipx_ycbcr *y; int cw = 0, ch = 0;
    int check(const char *who, const void *dst, int dw, int dh, int dstride)
    {
        IPX_FRAME(who, "destination", dst, dw, dh, dstride);
        const bool ok = y && y->y && y->cb && y->cr && y->w > 0 && y->h > 0 && ycbcr_ratio_ok(y->ratio);
        if (ok) chroma_size(y->ratio, y->w, y->h, &cw, &ch);
        if (!ok || y->ystride < y->w || y->cstride < cw) { set_error("%s: bad arguments", who); return IPX_ERR_INVALID; }
        if (!frame_span_ok(y->w, y->h, y->ystride, 1)) { set_error("%s: source planes beyond the addressable span", who); return IPX_ERR_UNSUPPORTED; }
        return IPX_OK;
    }
    size_t bytes() const { return align256((size_t)y->w * y->h) + 2 * align256((size_t)cw * ch); }
    int upload(hipStream_t s, uint8_t *dsrc, DevSrc *out) const
    {
        const size_t yb = align256((size_t)y->w * y->h), cbytes = align256((size_t)cw * ch);
        IPX_HIP(hipMemcpy2DAsync(dsrc, y->w, y->y, y->ystride, y->w, y->h, hipMemcpyHostToDevice, s));
        IPX_HIP(hipMemcpy2DAsync(dsrc + yb, cw, y->cb, y->cstride, cw, ch, hipMemcpyHostToDevice, s));
        IPX_HIP(hipMemcpy2DAsync(dsrc + yb + cbytes, cw, y->cr, y->cstride, cw, ch, hipMemcpyHostToDevice, s));
        out->kind = IPX_SRC_YCBCR; out->pix = dsrc; out->stride = y->w;
        out->cb = dsrc + yb; out->cr = dsrc + yb + cbytes; out->cstride = cw; out->ratio = y->ratio;
        out->w = y->w; out->h = y->h;
        return IPX_OK;
    }
};

// Scale and Draw of a host frame of any type: dst and the source go up, the operator runs on them in HBM, dst comes down.  Over
// reads the destination; Src leaves pixels outside the rectangle untouched.
template <typename Src>
int host_scale(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr, const Src &src, ipx_rect sr, int op)
{
    return stage_and_run(ctx, dst, dw, dh, dstride, src.bytes(), [&](hipStream_t s, int *flag, uint8_t *ddst, uint8_t *dsrc) -> int {
        DevSrc d;
        const int rc = src.upload(s, dsrc, &d);
        return rc ? rc : dev_scale_src(ctx, s, flag, ddst, dw, dh, dw * 4, to_rect(dr), d, to_rect(sr), op);
    });
}
template <typename Src>
int host_draw(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r, const Src &src, int spx, int spy, int op)
{
    return stage_and_run(ctx, dst, dw, dh, dstride, src.bytes(), [&](hipStream_t s, int *, uint8_t *ddst, uint8_t *dsrc) -> int {
        DevSrc d;
        const int rc = src.upload(s, dsrc, &d);
        return rc ? rc : dev_draw_src(s, ddst, dw, dh, dw * 4, to_rect(r), d, spx, spy, op);
    });
}

}  // namespace

// The order of the checks differs between the entries below, and callers see it (tests/test_single_ops_args_gpu.py pins it): every
// such place carries a comment; none of them is to be "tidied" into its neighbour's order.
extern "C" {

// ---- device-pointer operations ---------------------------------------------------------------------
int ipx_dev_scale_bilinear_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int dw, int dh,
                                 int dstride, ipx_rect dr, const uint8_t *src, int sw, int sh,
                                 int sstride, ipx_rect sr, int op) try
{
    IPX_ENTER(ctx);
    IPX_FRAME("ipx_dev_scale_bilinear_rgba8", "destination", dst, dw, dh, dstride);
    IPX_DEV_OUT("ipx_dev_scale_bilinear_rgba8", "destination", dst, (unsigned)dstride);
    IPX_FRAME("ipx_dev_scale_bilinear_rgba8", "source", src, sw, sh, sstride);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    AsyncFree mem{s, {}};
    int *flag = nullptr;
    if (op == IPX_OP_OVER) IPX_HIP(mem.get(&flag, sizeof(int)));   // the opaque() flag must outlive the launch: one device int per call
    return dev_scale_src(ctx, s, flag, dst, dw, dh, dstride, to_rect(dr), rgba_src(src, sw, sh, sstride), to_rect(sr), op);
}
IPX_CATCH_STATUS

int ipx_dev_draw_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int dw, int dh, int dstride,
                       ipx_rect r, const uint8_t *src, int sw, int sh, int sstride, int spx, int spy,
                       int op) try
{
    IPX_ENTER(ctx);
    IPX_FRAME("ipx_dev_draw_rgba8", "destination", dst, dw, dh, dstride);
    IPX_DEV_OUT("ipx_dev_draw_rgba8", "destination", dst, (unsigned)dstride);
    IPX_FRAME("ipx_dev_draw_rgba8", "source", src, sw, sh, sstride);
    return dev_draw_src(stream ? (hipStream_t)stream : ctx->stream, dst, dw, dh, dstride, to_rect(r), rgba_src(src, sw, sh, sstride), spx, spy, op);
}
IPX_CATCH_STATUS

// ---- host-pointer operations: the two entries of a source type differ in their last call alone -------------------------------------
int ipx_scale_bilinear_rgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr,
                             const uint8_t *src, int sw, int sh, int sstride, ipx_rect sr, int op) try
{
    IPX_ENTER(ctx);
    const HostPacked h{src, sw, sh, sstride, IPX_SRC_RGBA};
    int rc = h.check("ipx_scale_bilinear_rgba8", dst, dw, dh, dstride);
    if (rc) return rc;
    ScalePrep pr;       // deliberate ABI behaviour: op and sr are judged BEFORE a zero-size frame returns IPX_OK (every other Scale entry: after)
    if ((rc = scale_prepare(dw, dh, to_rect(dr), sw, sh, to_rect(sr), op, &pr))) return rc;
    if (pr.empty || dw == 0 || dh == 0) return IPX_OK;
    return host_scale(ctx, dst, dw, dh, dstride, dr, h, sr, op);
}
IPX_CATCH_STATUS

int ipx_draw_rgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r,
                   const uint8_t *src, int sw, int sh, int sstride, int spx, int spy, int op) try
{
    IPX_ENTER(ctx);
    const HostPacked h{src, sw, sh, sstride, IPX_SRC_RGBA};
    if (const int rc = h.check("ipx_draw_rgba8", dst, dw, dh, dstride)) return rc;
    // deliberate ABI behaviour: op is judged BEFORE a zero-size frame returns IPX_OK (every other Draw entry: after)
    if (op != IPX_OP_OVER && op != IPX_OP_SRC) { set_error("draw: unknown op %d", op); return IPX_ERR_INVALID; }
    if (!dw || !dh || !sw || !sh) return IPX_OK;
    return host_draw(ctx, dst, dw, dh, dstride, r, h, spx, spy, op);
}
IPX_CATCH_STATUS

int ipx_scale_bilinear_nrgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr,
                              const uint8_t *src, int sw, int sh, int sstride, ipx_rect sr, int op) try
{
    IPX_ENTER(ctx);
    const HostPacked h{src, sw, sh, sstride, IPX_SRC_NRGBA};
    if (const int rc = h.check("ipx_scale_bilinear_nrgba8", dst, dw, dh, dstride)) return rc;
    if (!dw || !dh || !sw || !sh) return IPX_OK;       // deliberate ABI behaviour: before op and sr are looked at
    return host_scale(ctx, dst, dw, dh, dstride, dr, h, sr, op);
}
IPX_CATCH_STATUS

int ipx_draw_nrgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r, const uint8_t *src,
                    int sw, int sh, int sstride, int spx, int spy, int op) try
{
    IPX_ENTER(ctx);
    const HostPacked h{src, sw, sh, sstride, IPX_SRC_NRGBA};
    if (const int rc = h.check("ipx_draw_nrgba8", dst, dw, dh, dstride)) return rc;
    if (!dw || !dh || !sw || !sh) return IPX_OK;       // deliberate ABI behaviour: before op is looked at
    return host_draw(ctx, dst, dw, dh, dstride, r, h, spx, spy, op);
}
IPX_CATCH_STATUS

int ipx_scale_bilinear_deep(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr, const uint8_t *src, int sw, int sh,
                            int sstride, int kind, ipx_rect sr, int op) try
{
    IPX_ENTER(ctx);
    const HostDeep h{src, sw, sh, sstride, kind};
    if (const int rc = h.check("ipx_scale_bilinear_deep", dst, dw, dh, dstride)) return rc;
    if (!dw || !dh || !sw || !sh) return IPX_OK;       // deliberate ABI behaviour: before op and sr are looked at
    return host_scale(ctx, dst, dw, dh, dstride, dr, h, sr, op);
}
IPX_CATCH_STATUS

int ipx_draw_deep(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r, const uint8_t *src, int sw, int sh, int sstride,
                  int kind, int spx, int spy, int op) try
{
    IPX_ENTER(ctx);
    const HostDeep h{src, sw, sh, sstride, kind};
    if (const int rc = h.check("ipx_draw_deep", dst, dw, dh, dstride)) return rc;
    if (!dw || !dh || !sw || !sh) return IPX_OK;       // deliberate ABI behaviour: before op is looked at
    return host_draw(ctx, dst, dw, dh, dstride, r, h, spx, spy, op);
}
IPX_CATCH_STATUS

int ipx_scale_bilinear_ycbcr(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr,
                             const ipx_ycbcr *src, ipx_rect sr) try
{
    IPX_ENTER(ctx);
    HostYCbCr h{src};
    if (const int rc = h.check("ipx_scale_bilinear_ycbcr", dst, dw, dh, dstride)) return rc;
    if (!dw || !dh) return IPX_OK;       // deliberate ABI behaviour: an empty SOURCE was refused above (the packed types: IPX_OK), sr is not looked at
    return host_scale(ctx, dst, dw, dh, dstride, dr, h, sr, IPX_OP_SRC);
}
IPX_CATCH_STATUS

int ipx_draw_ycbcr(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r, const ipx_ycbcr *src,
                   int spx, int spy) try
{
    IPX_ENTER(ctx);
    HostYCbCr h{src};
    if (const int rc = h.check("ipx_draw_ycbcr", dst, dw, dh, dstride)) return rc;
    if (!dw || !dh) return IPX_OK;       // deliberate ABI behaviour: an empty SOURCE was refused above (the packed types: IPX_OK)
    return host_draw(ctx, dst, dw, dh, dstride, r, h, spx, spy, IPX_OP_SRC);
}
IPX_CATCH_STATUS

}  // extern "C"
