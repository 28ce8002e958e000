// ipx_runtime_internal.h -- the runtime's own types (context, lanes, glyph sets, plans) and the small helpers every
// translation unit that implements ABI entries needs (ipx_context.hip, ipx_image_ops.hip, ipx_text.hip, ipx_plan.hip, ipx_runtime.hip,
// ipx_out_stage.hip, ipx_jpeg_runtime.hip, ipx_jpeg_dec_runtime.hip, the legs, the GIF and PNG halves).  What only the decode drivers
// share sits on top of it in ipx_decode_common.h.  Not part of the ABI.
#pragma once

#include <atomic>
#include <sched.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ipx_align.h"
#include "ipx_gif_mixed_plan.h"
#include "ipx_internal.h"
#include "ipx_ks.h"

using namespace ipx;

// ---------------------------------------------------------------------------------------------
struct Lane {
    hipStream_t stream = nullptr;
    uint8_t *dev = nullptr;   // device scratch
    size_t dev_bytes = 0;
    int *flag = nullptr;      // device int for the opaque() scan
    uint8_t *dec = nullptr;   // second grow-only buffer: planes and scratch of a decode running on this lane (ipx_plan_run_jpeg_jpeg)
    size_t dec_bytes = 0;
    uint8_t *pin = nullptr;   // pinned bounce buffer for small single-frame calls on pageable memory (run_host_packed)
    size_t pin_bytes = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // of the chunk in this lane's scratch: uploaded, computed, downloaded (run_host_packed)
    bool busy = false;
};

struct ipx_ctx {
    int device = 0;
    int cus = 256;                 // compute units of the device
    hipStream_t stream = nullptr;  // default stream for device-pointer calls
    std::vector<Lane> lanes;
    size_t lane_bytes = 0;
    std::mutex mu;
    std::condition_variable cv;
    // pinned host blocks: hipHostMalloc / hipHostFree cost milliseconds each, and the encoder hands out one block per
    // batch and output, so freed blocks are kept (up to host_cache_limit bytes) and reused for requests they fit
    std::mutex host_mu;
    std::map<void *, size_t> host_size;            // every live block handed out by ipx_host_alloc
    std::multimap<size_t, void *> host_free_blocks;
    std::deque<void *> host_lru;                   // cached blocks, least recently freed first
    size_t host_cached = 0, host_cache_limit = (size_t)8 << 30;   // IPX_HOST_CACHE_MB
    // one row of 128s: the Cb / Cr "planes" (stride 0) that make a Gray frame a YCbCr frame with neutral chroma (ipx_plan_run_dev_gray)
    // compressed-in / compressed-out parts in flight (ipx_plan_run_jpeg_jpeg): capped at three per context.  Measured: two or three parts
    // side by side overlap nicely (one decodes while another is in its host-paced encode read-backs), four take 0.9 s EACH in their
    // decode step instead of 0.03 s -- whatever serialises there (allocation, synchronisation), a fourth part gains nothing
    int jj_active = 0;
    uint8_t *flat_chroma = nullptr;
    // plans (tap tables in HBM) and uploaded glyph sets by content, for callers that describe their operators per call
    // (ipx_plan_acquire: the per-operator seam, the pool): no hipMalloc / hipFree in the steady state
    std::mutex plan_mu;
    std::map<std::string, std::pair<ipx_glyphset *, ipx_plan *>> plan_cache;
    uint64_t plan_clock = 0;
    // axes of the kernel scaler in HBM by (destination extent, source extent), for the per-operation seam (ks_axis_get)
    std::mutex ks_mu;
    std::map<std::pair<int, int>, std::pair<uint8_t *, KsAxisDev>> ks_axes;
    // ipx_jpeg_decode_counts: files decoded by route (IPX_JPEG_ROUTE_*) since ipx_create; [3]: files the GPU scan walk ended with a status
    std::atomic<long long> jpeg_counts[4] = {{0}, {0}, {0}, {0}};
    // ipx_png_decode_counts: files and tokens of the parallel inflate (IPX_PNG_PAR=1) since ipx_create
    std::atomic<long long> png_counts[5] = {{0}, {0}, {0}, {0}, {0}};
    // ipx_gif_decode_counts: files and records of the parallel code walk (IPX_GIF_PAR=1) since ipx_create
    std::atomic<long long> gif_counts[4] = {{0}, {0}, {0}, {0}};
    std::atomic<long long> jpeg_cmyk_files{0};     // ipx_jpeg_cmyk_files: files that reached the four-component decoder (ipx_jpeg_dec_cmyk.hip)
    static constexpr size_t kFlatChromaBytes = (size_t)64 << 10;
};

struct GlyphHost {
    size_t mask_off;  // offset of this glyph's mask in the packed blob
    int mw, mh;
    Rect dr;
    int mpx, mpy;
};

struct ClippedGlyphs {
    DevGlyph *dev = nullptr;
    int n = 0;
    Rect bbox{0, 0, 0, 0};
};

struct ipx_glyphset {
    int device = 0;
    std::vector<GlyphHost> g;
    uint8_t *masks_dev = nullptr;
    size_t masks_bytes = 0;
    uint8_t col[4] = {0, 0, 0, 0};
    mutable std::mutex mu;
    mutable std::map<std::pair<int, int>, ClippedGlyphs> clipped;  // per frame size
};

struct PlanScale {
    bool on = false;
    int dw = 0, dh = 0;
    Rect sr{0, 0, 0, 0};
    KsAxis hx, hy;          // newDistrib of the two axes, as built on the host (the fused kernel's tables are cut from these)
    KsAxisDev ax[2]{};      // the same in the plan's blob: [0] horizontal, [1] vertical
};

struct ipx_plan {
    ipx_plan_params p{};
    ipx_plan_info info{};
    PlanScale sc[2];      // 0 = resize, 1 = thumbnail
    // tilings and tables of the one-pass kernel (ipx_ks_fused.hip) per LDS tile format -- [0] packed RGBA8 pixels (4 bytes), [1] four 16-bit
    // taps per pixel (8: NRGBA, YCbCr, deep sources), [2] one 16-bit tap (2: Gray); .ok = false: per-output kernels for that format
    KsFusedPlan fused[3];
    uint8_t *blob = nullptr;
    ClippedGlyphs glyphs;
    mutable std::mutex mu;
    ipx_glyphset *owned_gs = nullptr;         // a glyph set that lives and dies with this plan (ipx_plan_acquire)
    // a plan of the context's cache (guarded by ipx_ctx::plan_mu): calls holding it, and when it was last handed out
    int cache_refs = 0;
    uint64_t cache_stamp = 0;
};

inline int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

struct DeviceGuard {  // hipSetDevice is per-thread; callers may arrive on any OS thread
    explicit DeviceGuard(int dev) { ok = hipSetDevice(dev) == hipSuccess; }
    bool ok;
};

#define IPX_ENTER(ctx)                                                         \
    clear_error();                                                             \
    if (!(ctx)) { set_error("%s: null context", __func__); return IPX_ERR_INVALID; } \
    DeviceGuard guard_((ctx)->device);                                         \
    if (!guard_.ok) { set_error("hipSetDevice(%d) failed", (ctx)->device); return IPX_ERR_HIP; }

class LaneLease {
public:
    explicit LaneLease(ipx_ctx *c) : c_(c)
    {
        std::unique_lock<std::mutex> lk(c->mu);
        c->cv.wait(lk, [&] {
            for (auto &l : c->lanes) if (!l.busy) return true;
            return false;
        });
        for (auto &l : c->lanes) if (!l.busy) { l.busy = true; lane_ = &l; break; }
    }
    ~LaneLease()
    {
        {
            std::lock_guard<std::mutex> lk(c_->mu);
            lane_->busy = false;
        }
        c_->cv.notify_all();     // waiters differ (one lane / every lane): wake them all, the predicates sort it out
    }
    Lane *operator->() { return lane_; }
    Lane &get() { return *lane_; }
private:
    ipx_ctx *c_;
    Lane *lane_ = nullptr;
};

inline int lane_reserve_dec(Lane &l, size_t bytes)
{
    if (bytes <= l.dec_bytes) return IPX_OK;
    if (l.dec) { IPX_HIP(hipStreamSynchronize(l.stream)); IPX_HIP(hipFree(l.dec)); l.dec = nullptr; l.dec_bytes = 0; }
    const size_t want = bytes + bytes / 8;        // a little headroom: batches of one size differ by a few files' worth of scan bytes
    hipError_t e = hipMalloc((void **)&l.dec, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("device allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
        return IPX_ERR_NOMEM;
    }
    l.dec_bytes = want;
    return IPX_OK;
}

inline int lane_reserve(Lane &l, size_t bytes)
{
    if (bytes <= l.dev_bytes) return IPX_OK;
    if (l.dev) { IPX_HIP(hipStreamSynchronize(l.stream)); IPX_HIP(hipFree(l.dev)); l.dev = nullptr; l.dev_bytes = 0; }
    const size_t want = std::max(bytes, l.dev_bytes * 2);
    hipError_t e = hipMalloc((void **)&l.dev, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("device allocation of %zu bytes failed: %s", want, hipGetErrorString(e));
        return IPX_ERR_NOMEM;
    }
    l.dev_bytes = want;
    return IPX_OK;
}

// status of a frame argument: IPX_ERR_INVALID for a malformed one, IPX_ERR_UNSUPPORTED for one beyond the addressable span
inline int frame_status(const char *who, const char *what, const void *p, int w, int h, long long stride, int bpp = 4)
{
    if (!p || w < 0 || h < 0 || stride < (long long)w * bpp) { set_error("%s: bad %s frame arguments", who, what); return IPX_ERR_INVALID; }
    if (!frame_span_ok(w, h, stride, bpp)) {
        set_error("%s: %s frame %dx%d (stride %lld) is beyond the 2 GiB / 65535-pixel span the kernels address", who, what, w, h, stride);
        return IPX_ERR_UNSUPPORTED;
    }
    return IPX_OK;
}
#define IPX_FRAME(who, what, p, w, h, stride) do { const int rc_ = frame_status(who, what, p, w, h, stride); if (rc_) return rc_; } while (0)

// A frame the kernels WRITE in HBM: every store is a whole pixel (a dword; the one-pass kernel's watermark copy: four) at its natural
// alignment, so the frame's address, row stride and frame stride are multiples of 4.  Anything else is refused before a launch.
inline int dev_out_status(const char *who, const char *what, const void *p, unsigned long long stride, unsigned long long frame_stride = 0)
{
    if (p && (((uintptr_t)p | stride | frame_stride) & 3)) {
        set_error("%s: the %s frames' address and strides must be multiples of 4", who, what);
        return IPX_ERR_INVALID;
    }
    return IPX_OK;
}
#define IPX_DEV_OUT(who, what, p, ...) do { const int rc_ = dev_out_status(who, what, p, __VA_ARGS__); if (rc_) return rc_; } while (0)

// The body of a worker thread: an exception must not leave the thread (std::terminate would take the Go / Python worker down);
// it becomes the status and text the spawning call reports.
template <class F> inline int guarded_status(F &&fn, std::string *text) noexcept
{
    try { fn(); return IPX_OK; }
    catch (...) {
        const int rc = status_of_exception();
        if (text) { try { *text = ipx_last_error(); } catch (...) { } }
        return rc;
    }
}

// CPUs local to a device's PCIe root, intersected with what the process may use.  Best effort: nothing happens if sysfs says nothing.
inline void bind_near_device(int device)
{
    if (env_int("IPX_POOL_NUMA", 1) == 0) return;
    char bus[32] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return; }
    for (char *c = bus; *c; c++) *c = (char)tolower((unsigned char)*c);
    char path[128];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
    FILE *f = fopen(path, "r");
    if (!f) return;
    char line[4096] = {0};
    const bool ok = fgets(line, sizeof line, f) != nullptr;
    fclose(f);
    if (!ok) return;
    cpu_set_t allowed, want;
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
    CPU_ZERO(&want);
    for (char *p = line; *p;) {            // "0-31,64-95"
        char *e = nullptr;
        long a = strtol(p, &e, 10);
        if (e == p) break;
        long b = a;
        if (*e == '-') { p = e + 1; b = strtol(p, &e, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (CPU_ISSET((int)c, &allowed)) CPU_SET((int)c, &want);
        p = *e == ',' ? e + 1 : e;
        if (*e != ',') break;
    }
    if (CPU_COUNT(&want) > 0) (void)sched_setaffinity(0, sizeof want, &want);
}


// The device's view of `span` bytes of host memory a kernel may write: non-null when the range is pinned and mapped (hipHostMalloc,
// hipHostRegister), null for pageable memory.  Kernels then write outputs over the link themselves: dst_direct, below, is its one caller.
inline uint8_t *pinned_device_view(uint8_t *host, size_t span)
{
    if (!host || !span) return nullptr;
    hipPointerAttribute_t at, last;
    if (hipPointerGetAttributes(&at, host) != hipSuccess || at.type != hipMemoryTypeHost || !at.devicePointer) { (void)hipGetLastError(); return nullptr; }
    if (hipPointerGetAttributes(&last, host + span - 1) != hipSuccess || last.type != hipMemoryTypeHost) { (void)hipGetLastError(); return nullptr; }   // a registered range may end before the batch does
    return (uint8_t *)at.devicePointer;
}

// stream-ordered scratch of one call: freed (in stream order) when the call returns
struct AsyncFree {
    hipStream_t s;
    std::vector<void *> p;
    // optional arena (a lane's grow-only buffer): requests are bumped out of it while they fit, so a call that holds a lane allocates
    // nothing in the steady state.  Stream-ordered allocations of gigabytes per call turned out to stall for 0.5 - 5 s every few calls
    // on some boxes (the time sat in hipMallocAsync or behind it).
    uint8_t *arena = nullptr;
    size_t cap = 0, off = 0;
    ~AsyncFree() { for (void *q : p) (void)hipFreeAsync(q, s); }
    template <class T> hipError_t get(T **out, size_t bytes)
    {
        const size_t need = ((bytes ? bytes : 1) + 255) & ~(size_t)255;
        if (arena && off + need <= cap) { *out = (T *)(arena + off); off += need; return hipSuccess; }
        void *q = nullptr;
        hipError_t e = hipMallocAsync(&q, bytes ? bytes : 1, s);
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
};

// n texts clipped against one frame size (ipx_textset_create; the compressed-in / compressed-out legs build one per call on their own
// stream): every text's clipped glyphs in ONE table, every mask in one blob, one descriptor per text.  The device memory is
// stream-ordered and goes, in stream order, with the object.
struct ipx_textset {
    int device = 0, w = 0, h = 0, n = 0;
    std::vector<Rect> bbox;             // per text, as in its descriptor: the host sizes the grid by the largest of a launch
    DevText *texts_dev = nullptr;
    DevGlyph *glyphs_dev = nullptr;
    AsyncFree mem{nullptr, {}};
};
// host only: IPX_ERR_INVALID for a bad list or mask, IPX_ERR_UNSUPPORTED for a text of more than kMaxGlyphs glyphs
int texts_check(const char *who, const ipx_text *texts, int n);
// texts_check, then clip, pack and upload on `s`; returns with the uploads finished (the host staging is the call's own)
int textset_build(hipStream_t s, const char *who, const ipx_text *texts, int n, int w, int h, ipx_textset *ts);
// ONE launch (per 65535 frames) of composite_texts_kernel: frame z takes text map[z], or first + z.  `map` is host memory, uploaded into
// *mem and read by that copy until `s` has been waited for; indices are checked here, before the launch.
int dev_composite_texts(hipStream_t s, AsyncFree *mem, uint8_t *dst, int dstride, size_t frame_stride, int n_frames, const ipx_textset &ts,
                        int first, const int *map);
// what the six compressed-in / compressed-out entries check before they do anything: the arguments and, in a _texts entry, that the plan
// is copy-only (no glyph set of its own) and the texts are well-formed; *result is null from here on
int leg_entry_check(const char *who, const ipx_plan *pl, int n, const ipx_bytes *files, const int *status, ipx_jpeg_result **result,
                    bool texts_entry, const ipx_text *texts);

// Waits for its stream on every way out of the scope.  Declare it AFTER every host buffer that copies queued on the stream read or write:
// locals go in reverse order, so the wait then comes before those buffers are destroyed.
struct StreamSync {
    hipStream_t s;
    ~StreamSync() { (void)hipStreamSynchronize(s); }
};

// ---- what the six encode cores (jpeg_encode_sets, jpeg_encode_mixed_core, png_encode_core, png_encode_mixed_core, gif_encode_core,
// ---- gif_encode_mixed_core)
// ---- and the single-frame entries built on them share -----------------------------------------------------------------------------

// The tail of every core: the `total` bytes of finished streams at `dev` come down into one pinned block (one byte for an empty total),
// *blob.  Allocate, queue, wait, keep the first error; a failed download gives the block back and reports "<prefix>stream download
// failed".  The wait is also what the core's host tables, read by copies queued before, are kept until.  queued: when the copy was queued.
inline int download_streams(ipx_ctx *ctx, hipStream_t s, const uint8_t *dev, size_t total, const char *prefix, uint8_t **blob,
                            std::chrono::steady_clock::time_point *queued = nullptr)
{
    uint8_t *host = (uint8_t *)ipx_host_alloc(ctx, total ? total : 1);   // pinned: the download runs at link speed
    if (!host) return IPX_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(host, dev, total, hipMemcpyDeviceToHost, s);
    if (queued) *queued = std::chrono::steady_clock::now();
    { const hipError_t e2 = hipStreamSynchronize(s); if (e == hipSuccess) e = e2; }
    if (e != hipSuccess) { (void)ipx_host_free(ctx, host); set_error("%sstream download failed: %s", prefix, hipGetErrorString(e)); return IPX_ERR_HIP; }
    *blob = host;
    return IPX_OK;
}

// ipx_png_encode_rgba8 and ipx_gif_encode_rgba8: one frame in host memory is checked by the codec's rule, staged in stream-ordered
// scratch of a leased lane, encoded by the codec's core and copied out of the pinned block into a malloc'ed buffer (ipx_buffer_free).
using EncodeCheck = int (*)(const char *who, const void *src, int w, int h, long long stride, int n);
using EncodeCore = int (*)(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                           size_t *offs, size_t *lens);
inline int encode_one_rgba8(const char *who, ipx_ctx *ctx, EncodeCheck check, EncodeCore core, const uint8_t *pix, int w, int h, int stride,
                            uint8_t **out, size_t *len)
{
    if (!out || !len) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *out = nullptr;
    *len = 0;
    int rc = check(who, pix, w, h, stride, 1);
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
        rc = core(ctx, s, dsrc, w, h, w * 4, fbytes, 1, &blob, &off, &n);
        if (rc) return rc;
    }
    uint8_t *m = (uint8_t *)malloc(n);
    if (!m) { (void)ipx_host_free(ctx, blob); set_error("%s: out of memory", who); return IPX_ERR_NOMEM; }
    memcpy(m, blob + off, n);
    (void)ipx_host_free(ctx, blob);
    *out = m;
    *len = n;
    return IPX_OK;
}

// The opening of ipx_png_encode_mixed_dev, ipx_jpeg_encode_mixed_dev and ipx_gif_encode_mixed_dev: the arguments, then *blob = NULL (n == 0 is then done: the
// caller returns), at most 65535 frames, and every frame before any launch -- a malformed one first (IPX_ERR_INVALID; `extra` is the
// codec's own refusal of a well-formed frame, with its text set, or IPX_OK), then one beyond the span the kernels address
// (IPX_ERR_UNSUPPORTED; span_of_stride: of rows `stride` apart as the caller has them, else of tight rows).
using RgbaFrameCheck = int (*)(const char *who, int f, const ipx_rgba_frame &fr);
inline int rgba_frames_check(const char *who, const ipx_rgba_frame *frames, int n, uint8_t **blob, const size_t *offs, const size_t *lens,
                             RgbaFrameCheck extra, bool span_of_stride)
{
    if (!blob || !offs || !lens || n < 0 || (n && !frames)) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("%s: at most 65535 frames per call", who); return IPX_ERR_UNSUPPORTED; }
    for (int f = 0; f < n; f++) {
        const ipx_rgba_frame &fr = frames[f];
        if (!fr.pix || fr.w <= 0 || fr.h <= 0 || (long long)fr.stride < (long long)fr.w * 4) {
            set_error("%s: frame %d: bad argument", who, f);
            return IPX_ERR_INVALID;
        }
        if (const int rc = extra(who, f, fr)) return rc;
    }
    for (int f = 0; f < n; f++)
        if (!frame_span_ok(frames[f].w, frames[f].h, span_of_stride ? (long long)frames[f].stride : (long long)frames[f].w * 4, 4)) {
            set_error("%s: frame %d: %dx%d is beyond the frames the encoder addresses", who, f, frames[f].w, frames[f].h);
            return IPX_ERR_UNSUPPORTED;
        }
    return IPX_OK;
}

// ---- Scale and Draw on frames in HBM (ipx_image_ops.hip) -----------------------------------------------------------------------------

// a source image resident in HBM: RGBA / NRGBA pixels, or the three planes of a YCbCr image
struct DevSrc {
    int kind = IPX_SRC_RGBA;
    const uint8_t *pix = nullptr;   // pixels, or the Y plane
    int stride = 0;                 // bytes per row of pix
    const uint8_t *cb = nullptr, *cr = nullptr;
    int cstride = 0, ratio = 0;
    int w = 0, h = 0;
    int nframes = 1;                // a batch: frames frame_stride / c_frame_stride bytes apart
    size_t frame_stride = 0, c_frame_stride = 0;
    bool le_alpha = false;          // IPX_SRC_TAP64: no colour tap exceeds its alpha tap (NRGBA64, Gray16, CMYK after the expansion; not RGBA64)
};

// dst / src are device pointers at pixel (0,0)
int dev_draw_src(hipStream_t s, uint8_t *dst, int dw, int dh, int dstride, Rect r, const DevSrc &src, int spx, int spy, int op, size_t dst_fs = 0);
// xdraw.BiLinear.Scale(dst, dr, src, sr, op, nil) on device frames.  kind_override >= 0: the tap kind to read the source with (the
// crop thumbnail's second scale, ipx_ks.h); axes: the plan's own tables, or NULL to take them from the context's cache
int dev_scale_src(ipx_ctx *ctx, hipStream_t s, int *flag, uint8_t *dst, int dw, int dh, int dstride, const Rect &dr, const DevSrc &src,
                  const Rect &sr, int op, size_t dst_fs = 0, int kind_override = -1, const KsAxisDev *axes = nullptr);

// The one staging path of the single-image host entries (the eight of ipx_image_ops.hip, ipx_composite_glyphs_rgba8 of ipx_text.hip):
// a leased lane's scratch as [dst][src_bytes of source][1024 bytes of slack]; dst goes up, `upload_and_run` uploads what source it has
// and launches on the lane's stream, dst comes down and the stream is waited for.  A failing run drains the stream before its status
// is returned: copies queued on it read the caller's memory.
template <typename F>
int stage_and_run(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, size_t src_bytes, F &&upload_and_run)
{
    LaneLease lane(ctx);
    const size_t dbytes = align256((size_t)dw * dh * 4);
    int rc = lane_reserve(lane.get(), dbytes + src_bytes + 1024);
    if (rc) return rc;
    uint8_t *ddst = lane->dev, *dsrc = lane->dev + dbytes;
    hipStream_t s = lane->stream;
    IPX_HIP(hipMemcpy2DAsync(ddst, (size_t)dw * 4, dst, dstride, (size_t)dw * 4, dh, hipMemcpyHostToDevice, s));
    rc = upload_and_run(s, lane->flag, ddst, dsrc);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    IPX_HIP(hipMemcpy2DAsync(dst, dstride, ddst, (size_t)dw * 4, (size_t)dw * 4, dh, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    return IPX_OK;
}

// ---- glyph sets (ipx_text.hip) -------------------------------------------------------------------------------------------------------

// clip every glyph against a dw x dh frame (image/draw.clip) and cache the device table
int glyphs_for_frame(const ipx_glyphset *gs, int dw, int dh, ClippedGlyphs *out);

// ---- the input side of the plan entries (ipx_runtime.hip) ---------------------------------------------------------------------------

// n equally sized frames of one Go image type, in host memory or in HBM: the size is the plan's, frame i of plane p starts at
// plane[p] + i * frame_stride[p ? 1 : 0]
struct BatchSrc {
    int type = kSrcRGBA;                                   // SrcType
    int ratio = 0;                                         // kSrcYCbCr: IPX_YCBCR_*
    const uint8_t *plane[3] = {nullptr, nullptr, nullptr}; // pixels / index / Y, then Cb and Cr
    int stride[2] = {0, 0};                                // bytes per row of plane 0, of the chroma planes
    size_t frame_stride[2] = {0, 0};
    const uint8_t *palettes = nullptr;                     // kSrcPaletted: 256 x RGBA per frame, 1024 bytes apart
    BatchSrc from(int i0) const                            // the same from frame i0 on
    {
        BatchSrc b = *this;
        for (int p = 0; p < 3; p++) if (b.plane[p]) b.plane[p] += (size_t)i0 * frame_stride[p ? 1 : 0];
        if (b.palettes) b.palettes += (size_t)i0 * 1024;
        return b;
    }
};
inline BatchSrc packed_src(int type, const uint8_t *pix, int stride, size_t frame_stride, const uint8_t *palettes = nullptr)
{
    BatchSrc b;
    b.type = type; b.plane[0] = pix; b.stride[0] = stride; b.frame_stride[0] = frame_stride; b.palettes = palettes;
    return b;
}
inline BatchSrc ycbcr_src(const ipx_ycbcr_batch *y)        // (a null y: a batch src_check refuses)
{
    BatchSrc b;
    b.type = kSrcYCbCr;
    if (!y) return b;
    b.ratio = y->ratio; b.plane[0] = y->y; b.plane[1] = y->cb; b.plane[2] = y->cr;
    b.stride[0] = y->ystride; b.stride[1] = y->cstride; b.frame_stride[0] = y->y_frame_stride; b.frame_stride[1] = y->c_frame_stride;
    return b;
}

// The one rule for the arguments of a batch entry `who`.  IPX_ERR_INVALID: no plan, n < 0, an unknown type or ratio, a null plane or
// palette, a row stride below the row (for YCbCr: of the chroma planes too).  IPX_ERR_UNSUPPORTED: rows beyond the span the kernels
// address (for the deep types: of their frames of taps too).  in_hbm -- the kernels read this memory themselves, not a re-packed copy in
// scratch -- adds what they need of it: pixels, row and frame stride of a deep type on 2 bytes (CMYK: 4), palettes on 4
// (IPX_ERR_INVALID), and at most 65535 frames per call (IPX_ERR_UNSUPPORTED).
int src_check(const char *who, const ipx_plan *pl, const BatchSrc &b, int n, bool in_hbm);

// How `slots` frames of a source lie in device scratch: [slots x plane 0][slots x Cb][slots x Cr][slots x palette], rows tight,
// frames fs[] apart.  frame_rule: a plane's bytes -> its frame stride (align256, or run_host_packed's own).
struct SrcLayout {
    int planes;            // 1, or 3 (kSrcYCbCr)
    size_t row[2];         // bytes per row: plane 0, chroma
    int h[2];
    size_t fs[2];
    size_t pal;            // 1024 (kSrcPaletted) or 0
    size_t frame_bytes() const { return fs[0] + (planes == 3 ? 2 * fs[1] : 0) + pal; }
};
SrcLayout src_layout(const ipx_plan *pl, const BatchSrc &b, size_t (*frame_rule)(size_t) = align256);

// How a leg moves frames up: frames that lie in host memory as they will in scratch as one run of bytes
// (join_frames; in pieces of `piece` bytes when that is not 0), else frame by frame -- a frame of tight rows as one run when
// join_rows, else hipMemcpy2DAsync.
struct CopyPolicy { bool join_frames, join_rows; size_t piece; };
constexpr CopyPolicy kCopyWholePlanes{true, false, 0}, kCopyFrames{false, true, 0}, kCopyFrameRows{false, false, 0};

// Queues the copies of frames i0 .. i0 + m of `host` into a block laid out for `slots` frames and describes them there in *in_hbm.
hipError_t src_upload(const BatchSrc &host, const SrcLayout &L, int i0, int m, uint8_t *scratch, int slots, hipStream_t s, const CopyPolicy &cp,
                      BatchSrc *in_hbm);

// ---- the output side of the plan entries (ipx_runtime.hip) --------------------------------------------------------------------------

// The plan's three outputs for a batch, in host memory or device-addressable: rows tight, frame i of output k at out[k] + i * frame_stride[k]
enum { kOutResize, kOutThumb, kOutWm, kOuts };
struct BatchDst {
    uint8_t *out[kOuts] = {nullptr, nullptr, nullptr};     // null: not wanted
    size_t frame_stride[kOuts] = {0, 0, 0};
    BatchDst from(int i0) const                            // the same from frame i0 on
    {
        BatchDst d = *this;
        for (int k = 0; k < kOuts; k++) if (d.out[k]) d.out[k] += (size_t)i0 * frame_stride[k];
        return d;
    }
};
inline BatchDst abi_dst(uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                        size_t wm_frame_stride)
{
    return BatchDst{{resize_out, thumb_out, wm_out}, {resize_frame_stride, thumb_frame_stride, wm_frame_stride}};
}
inline BatchDst job_dst(const ipx_job &q) { return abi_dst(q.resize_out, q.resize_frame_stride, q.thumb_out, q.thumb_frame_stride, q.wm_out, q.wm_frame_stride); }

// what the plan makes of output k: the size, the tightly packed bytes per frame (0: no such operator) and the name error texts use
struct OutShape { int w, h; size_t bytes; const char *name; };
inline OutShape out_shape(const ipx_plan_info &in, int k)
{
    if (k == kOutResize) return {in.resize_w, in.resize_h, in.resize_bytes, "resize"};
    if (k == kOutThumb) return {in.thumb_w, in.thumb_h, in.thumb_bytes, "thumbnail"};
    return {in.wm_w, in.wm_h, in.wm_bytes, "watermark"};
}

// How `slots` frames of every output lie in device scratch: [slots x resize][slots x thumbnail][slots x watermark], frames fs[] apart;
// bytes and fs are 0 for an output the caller does not want or the plan does not make.  frame_rule as for src_layout.
struct DstLayout {
    size_t bytes[kOuts] = {0, 0, 0}, fs[kOuts] = {0, 0, 0};
    DstLayout(const ipx_plan *pl, const BatchDst &host, size_t (*frame_rule)(size_t) = align256)
    {
        for (int k = 0; k < kOuts; k++)
            if (host.out[k] && (bytes[k] = out_shape(pl->info, k).bytes) != 0) fs[k] = frame_rule(bytes[k]);
    }
    size_t frame_bytes() const { return fs[0] + fs[1] + fs[2]; }
    BatchDst place(uint8_t *scratch, int slots) const
    {
        BatchDst d;
        for (int k = 0; k < kOuts; scratch += fs[k++] * slots)
            if (fs[k]) { d.out[k] = scratch; d.frame_stride[k] = fs[k]; }
        return d;
    }
};

// Outputs in pinned memory (hipHostMalloc / hipHostRegister: mapped into the device's address space) are written by the kernels
// themselves, over the link, instead of into scratch and from there by a copy engine.  true: *view is the device's view of m frames of
// every wanted output of `host`.  false -- they go through scratch, which pads: a wanted pointer or frame stride is no multiple of 16
// (the kernels store 16 bytes per lane), a range is not pinned, or IPX_HOST_DIRECT=0.
bool dst_direct(const DstLayout &L, const BatchDst &host, int m, BatchDst *view);

// Queues the copies of m frames of every wanted output from `dev` into `host` from frame i0 on.  join_frames: output by output, one that
// is tight on both sides (or a single frame) as one run of bytes, in pieces of `piece`; else one copy per frame and output, frame by frame.
hipError_t dst_download(const BatchDst &host, const BatchDst &dev, const DstLayout &L, int i0, int m, hipStream_t s, const CopyPolicy &cp);

// The plan's operators on m frames in HBM, outputs to device-addressable frames.  The one place that knows what a source type needs
// first: a palette or deep pixels are expanded (stream-ordered scratch), Gray gets the flat chroma row.
int run_dev_src(ipx_ctx *ctx, hipStream_t s, const ipx_plan *pl, int m, const BatchSrc &in_hbm, const BatchDst &dst);

// jpeg.Encode of up to three sets of n frames in HBM into one pinned block *blob (ipx_jpeg_runtime.hip); dcoefs: n * ipx_jpeg_coef_count
// int16 of scratch per set.
struct JpegEncSet { int16_t *dcoefs; const uint8_t *src; int w, h, stride; size_t frame_stride; size_t *offs, *lens; };   // offs / lens: [n], into *blob
int jpeg_encode_sets(ipx_ctx *ctx, hipStream_t s, const JpegEncSet *sets, int K, int n, int quality, uint8_t **blob);
// jpeg.Encode of n frames of any sizes in HBM into one pinned block *blob, three waits for the device for the whole list
// (ipx_jpeg_runtime.hip; the records: ipx_jpeg_enc_mixed_plan.h).  offs / lens: [n], into *blob.  Always the fused length pass:
// IPX_JPEG_FUSED_LEN and IPX_JPEG_HOST_ENTROPY do not apply.
int jpeg_encode_mixed_core(ipx_ctx *ctx, hipStream_t s, const ipx::JpegEncSrc *frames, int n, int quality, uint8_t **blob, size_t *offs, size_t *lens);

// gif.Encode of n frames in HBM into one pinned block *blob (ipx_gif.hip)
int gif_encode_core(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                    uint8_t **blob, size_t *offs, size_t *lens);
// gif.Encode of n frames of any sizes in HBM into one pinned block *blob, two waits for the device for the whole list (ipx_gif_mixed.hip;
// the records: ipx_gif_mixed_plan.h).  offs / lens: [n], into *blob.
int gif_encode_mixed_core(ipx_ctx *ctx, hipStream_t s, const ipx::GifMixSrc *frames, int n, uint8_t **blob, size_t *offs, size_t *lens);

// image.Decode of n JPEG files into planes in HBM (ipx_jpeg_dec_runtime.hip); *w x *h: the size asked for, or 0 for the first parsed file's
int jpeg_decode_files(ipx_ctx *ctx, hipStream_t s, Lane *lane, bool planes_in_lane, const ipx_bytes *jpegs, int n, int *w, int *h,
                      ipx_ycbcr_batch *planes, int *status, ipx_jpeg_planes **owner);
// IPX_JPEG_411=1, read on every call that parses files: 4:1:1 and 4:1:0 files are decoded instead of refused (handed to jpeg_parse)
bool jpeg_411_enabled();
// four-component files (ipx_jpeg_dec_cmyk.hip): the switch, the legs' test of a file's frame header (its vector, 1 or 2; 0: not one
// of these files), and the driver -- *w, *h as for jpeg_decode_files, want_h0 > 0: only files whose component 0 has that sampling
// factor (the legs' sub-batches are of one vector)
bool jpeg_cmyk_enabled();
int jpeg_cmyk_peek(const uint8_t *d, size_t len);
int jpeg_decode_cmyk_files(ipx_ctx *ctx, hipStream_t s, const ipx_bytes *jpegs, int n, int *w, int *h, int want_h0, ipx_cmyk_batch *frames,
                           int *status, ipx_jpeg_planes **owner);

// the pinned blocks the streams of the compressed-out batch entries live in (ipx_jpeg_result_free)
struct ipx_jpeg_result { std::vector<uint8_t *> blobs; };

// ---- the output stage of the compressed-out batch entries (ipx_out_stage.hip) --------------------------------------------------------

// An entry's result while it runs: freed on every way out but release(), which hands it to the caller.
class ResultOwner {
public:
    explicit ResultOwner(ipx_ctx *ctx) : ctx_(ctx), r_(new ipx_jpeg_result) {}
    ~ResultOwner() { ipx_jpeg_result_free(ctx_, r_); }
    ResultOwner(const ResultOwner &) = delete;
    ResultOwner &operator=(const ResultOwner &) = delete;
    void add(uint8_t *blob) { if (blob) r_->blobs.push_back(blob); }
    void adopt(ipx_jpeg_result *o);                    // moves o's blocks in and deletes o (null: nothing)
    ipx_jpeg_result *release() { ipx_jpeg_result *r = r_; r_ = nullptr; return r; }
private:
    ipx_ctx *ctx_;
    ipx_jpeg_result *r_;
};

enum class Codec { Jpeg, Png, Gif };

// The plan's three outputs (resize, thumbnail, watermark) as one compressed-out entry hands them out: the caller's array, the size, the
// frame bytes in HBM (0: not wanted, or not made by the plan) and, for JPEG, the coefficient scratch of jpeg_encode_sets.
struct PlanOutputs {
    struct Output { ipx_bytes *dst; int w, h; size_t fs, coef; Codec codec; };
    struct Frames { uint8_t *dev[3]; int16_t *coef[3]; };     // one chunk's outputs in a device block (place)
    Output o[3];
    PlanOutputs(const ipx_plan *pl, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, Codec res, Codec thumb, Codec wm);
    BatchDst dst(const Frames &f) const { return BatchDst{{f.dev[0], f.dev[1], f.dev[2]}, {o[0].fs, o[1].fs, o[2].fs}}; }   // for run_dev_src
    size_t frame_bytes() const { return o[0].fs + o[1].fs + o[2].fs + o[0].coef + o[1].coef + o[2].coef; }   // per frame of a block
    // a block of `chunk` frames: [chunk x resize][chunk x thumbnail][chunk x watermark][chunk x coefficients of each JPEG output]
    Frames place(uint8_t *block, int chunk) const;
    void clear(int n) const;      // nulls the first n slots of every array the caller passed
    int check_gif() const;        // every GIF output within gif.Encode's limits: IPX_OK, or IPX_ERR_INVALID with the error text set
};

// Which files of a call a leg, or a part, sub-batch or chunk of one, works on: slot g is the caller's file at(g).  What a leg makes for
// itself (gathered files, decoded frames, a text set of its own texts) is indexed by the slot; the caller's arrays (files, texts, status,
// the three ipx_bytes arrays) are reached through at(g) and nothing else.
struct FileSel {
    const int *idx;    // null: the n files from `first` on
    int first, n;
    int at(int g) const { return idx ? idx[g] : first + g; }
    FileSel slice(int g0, int m) const { return FileSel{idx ? idx + g0 : nullptr, first + g0, m}; }
};
inline FileSel all_files(int n) { return FileSel{nullptr, 0, n}; }

// A leg's per-file texts: whether they are drawn at all, the set, and what indexes it -- the slot in the selection it was built from
// (the JPEG parts and sub-batches, the GIF leg) or the caller's index (the PNG leg: one set per call, its groups select through idx).
struct LegTexts {
    bool draw = false, by_slot = true;
    ipx_textset ts;
    // draw: texts are given and the plan makes the watermark output the caller wants; then texts[sel.at(g)] become one set, on `s`
    int build(hipStream_t s, const char *who, const ipx_plan *pl, const PlanOutputs &outs, const ipx_text *texts, const FileSel &sel, bool slots);
};

// The step every compressed-out leg takes for a chunk of m frames that lie in HBM (`d`), slots c0 .. c0 + m of `sel`: the outputs are
// placed in `block` (laid out for `slots` frames), the operators run, the chunk's texts are drawn in one launch (texts: null, or the
// leg's) and the streams of every present output are published in the caller's arrays at sel.at(c0 + i) -- every slot when status is
// null, else only those whose status there is IPX_OK -- with the blocks going to *res.  Both the text index and the output index come
// from (sel, c0) here.  mem: where the copy of a frame-to-text map goes (texts by the caller's index through an index list); it is read
// until `s` has been waited for.
int run_chunk(ipx_ctx *ctx, hipStream_t s, const ipx_plan *pl, const PlanOutputs &outs, uint8_t *block, int slots, const BatchSrc &d,
              const FileSel &sel, int c0, int m, const LegTexts *texts, AsyncFree *mem, int quality, const int *status, ResultOwner &res);

// The leg of ipx_plan_run_host_png and ipx_plan_run_host_paletted_gif: n frames in host memory go up in chunks on one lane, each chunk
// through run_chunk; only the streams come back, into pinned blocks owned by *result.  chunk_env / chunk_default: the knob that caps a
// chunk's frames (a chunk also stays within 1 GiB of scratch).  Refusals in this order: a null result, src_check, a GIF output beyond
// gif.Encode's limits; then n == 0 is done.  (The host-frame JPEG leg drives every lane from a thread of its own: ipx_jpeg_legs.hip.)
int run_host_streams(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const BatchSrc &host, Codec res, Codec thumb, Codec wm,
                     const char *chunk_env, int chunk_default, int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out,
                     ipx_jpeg_result **result);
