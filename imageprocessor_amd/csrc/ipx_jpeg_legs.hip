// ipx_jpeg_legs.hip -- the three JPEG-out legs.  What JPEG supplies to the mixed-size JPEG-in, JPEG-out leg (ipx_run_jpeg_jpeg_mixed; the
// walk is mixed_leg in ipx_mixed_leg.h): the sampling class as the cut's kind, one decode pass per group (jpeg_mixed_decode in
// ipx_jpeg_dec_runtime.hip), a chunk's block out of the lane's scratch, one jpeg.Encode per chunk: jpeg_encode_sets where every output
// has one size, else jpeg_encode_mixed_core over every frame of the chunk.  Behind it the two uniform legs (one plan, every frame of
// the plan's size): frames in host memory to JPEG streams, every lane driven by a thread of its own (ipx_plan_run_host_jpeg,
// ipx_plan_run_host_ycbcr_jpeg), and JPEG files to JPEG streams (ipx_plan_run_jpeg_jpeg and its _texts twin).  All decode through
// ipx_jpeg_dec_runtime.hip, take the chunk step of ipx_out_stage.hip and encode through ipx_jpeg_runtime.hip.
// DESIGN.md sections 4.6, 4.11 and 7.
#include <atomic>
#include <chrono>
#include <optional>
#include <string>
#include <vector>

#include "ipx_mixed_leg.h"

// ---- the mixed-size JPEG-in, JPEG-out leg ------------------------------------------------------------------------------------------

namespace {
struct JpegMixed {
    static constexpr const char *kWho = "ipx_run_jpeg_jpeg_mixed";
    static constexpr const char *kGroupEnv = "IPX_JPEG_MIXED_GROUP", *kChunkEnv = "IPX_JPEG_MIXED_CHUNK_MB";
    static constexpr int kGroupFiles = 256, kChunkMB = 8192;
    static constexpr bool kRunsWithoutOutputs = false;      // a run no output is made for is left out
    // a file the decode left without planes is left out of its run
    bool decoded(int i) const { return frames[i].y != nullptr; }

    int quality;
    JpegBatchPlan parsed;
    std::vector<ipx_jpeg_frame> frames;     // by the caller's index, filled group by group
    // a group's planes: they go back, in stream order, with the group
    struct Group {
        OwnedBlocks<ipx_jpeg_planes> planes;
        Group(ipx_ctx *ctx, hipStream_t s) : planes(ctx, s) {}
    };
    // a chunk's block in the lane's scratch: per output the frames of every file, then the coefficient scratch of every file
    struct Chunk : ChunkFrames {
        std::vector<size_t> coef_off[kOuts];                // file p's coefficients of output k at base[k] + coef_off[k][p]
        bool same_size[kOuts] = {false, false, false};      // every file of the chunk has this output, of one size: one encode per chunk
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
    int parse(const ipx_bytes *files, int n, int *status)
    {
        frames.assign(n, ipx_jpeg_frame{});
        return jpeg_mixed_parse(files, n, status, &parsed);
    }
    std::pair<int, int> size(int i) const { return {parsed.info[i].w, parsed.info[i].h}; }
    // the sampling class of a parsed file as one number
    int kind(int i) const { const JpegDecInfo &I = parsed.info[i]; return I.ncomp == 1 ? 0 : I.h0 * 4 + I.v0; }
    int admit(const MixedCall &, int) const { return IPX_OK; }      // a file that has a plan is taken
    // bytes a file costs its decode group: the MCU-padded planes and the coefficient scratch (128 bytes per block and its DC value)
    size_t decode_cost(int i) const
    {
        const JpegDecInfo &I = parsed.info[i];
        const size_t mxx = (size_t)(I.w + 8 * I.h0 - 1) / (8 * I.h0), myy = (size_t)(I.h + 8 * I.v0 - 1) / (8 * I.v0);
        const size_t y = align256(64 * I.h0 * I.v0 * mxx * myy), c = I.ncomp == 1 ? 0 : align256(64 * mxx * myy);
        return y + 2 * c + mxx * myy * (I.ncomp == 1 ? 1 : I.h0 * I.v0 + 2) * 130 + 8192;
    }
    static size_t coef_bytes(const OutShape &sh) { return align256(ipx_jpeg_coef_count(sh.w, sh.h) * sizeof(int16_t)); }
    // what an output costs a chunk: the frame, its coefficients, and the encoder's streams (about the coefficients again)
    size_t out_cost(const OutShape &sh, int) const { return align256(sh.bytes) + 2 * coef_bytes(sh); }
    void trace(int n, const MixCut &cut) const
    {
        if (env_int("IPX_DEBUG_J2J", 0) != 0)
            fprintf(stderr, "[ipx] %s: %d files, %zu groups, %zu chunks, %zu runs\n", kWho, n, cut.groups.size(), cut.chunks.size(), cut.runs.size());
    }

    // ONE jpeg_mixed_decode call, which is one decode pass per sampling class whatever sizes it holds
    int decode(const MixedCall &c, Lane &lane, hipStream_t s, const ipx_bytes *files, const int *idx, int m, Group &g)
    {
        return jpeg_mixed_decode(c.ctx, s, env_int("IPX_JPEG_LANE_ARENA", 1) ? &lane : nullptr, files, parsed, idx, m, g.planes, frames.data(), c.status);
    }
    // the planes from file i on: the files of one size and class that follow it in the group lie one frame stride apart
    BatchSrc src(const Group &, int i, int) const
    {
        const JpegDecInfo &I = parsed.info[i];
        const ipx_jpeg_frame &f = frames[i];
        BatchSrc d;
        d.type = f.ratio == IPX_GRAY ? kSrcGray : kSrcYCbCr;
        d.ratio = f.ratio;
        d.plane[0] = f.y; d.plane[1] = f.cb; d.plane[2] = f.cr;
        d.stride[0] = f.ystride; d.stride[1] = f.cstride;
        const size_t myy = (size_t)(I.h + 8 * I.v0 - 1) / (8 * I.v0);
        d.frame_stride[0] = align256((size_t)f.ystride * 8 * I.v0 * myy); d.frame_stride[1] = align256((size_t)f.cstride * 8 * myy);
        return d;
    }
    int chunk_memory(const MixedCall &c, Lane &lane, AsyncFree &, const int *file, int n, Chunk &b) const
    {
        size_t bytes = 0;
        for (int k = 0; k < kOuts; k++) bytes = b.lay(c, file, n, k, bytes);
        for (int k = 0; k < kOuts; k++) {
            b.coef_off[k].resize(n);
            for (int p = 0; p < n; p++) { b.coef_off[k][p] = bytes; if (c.has(file[p], k)) bytes += coef_bytes(c.shape(file[p], k)); }
            b.same_size[k] = c.has(file[0], k);
            for (int p = 1; p < n && b.same_size[k]; p++)
                b.same_size[k] = c.has(file[p], k) && c.shape(file[p], k).w == c.shape(file[0], k).w && c.shape(file[p], k).h == c.shape(file[0], k).h;
        }
        if ((b.empty = !bytes)) return IPX_OK;
        if (const int rc = lane_reserve(lane, bytes + 256)) return rc;
        b.base[0] = b.base[1] = b.base[2] = (uint8_t *)(((uintptr_t)lane.dev + 255) & ~(uintptr_t)255);
        return IPX_OK;
    }
    // jpeg.Encode of the outputs `ks` of files [p0, p0 + n) of the chunk -- every one of them has each of these outputs, of one size, so
    // an output's frames are one frame stride apart -- in one jpeg_encode_sets call (three waits for the device)
    int encode(const MixedCall &c, hipStream_t s, const int *file, int p0, int n, const Chunk &b, const std::vector<int> &ks, ResultOwner &res) const
    {
        if (ks.empty()) return IPX_OK;
        std::vector<size_t> offs(ks.size() * (size_t)n), lens(ks.size() * (size_t)n);
        JpegEncSet sets[kOuts];
        for (size_t j = 0; j < ks.size(); j++) {
            const int k = ks[j];
            const OutShape sh = c.shape(file[p0], k);
            sets[j] = JpegEncSet{(int16_t *)(b.base[k] + b.coef_off[k][p0]), b.at(k, p0), sh.w, sh.h, sh.w * 4, c.out_fs(file[p0], k),
                                 offs.data() + j * (size_t)n, lens.data() + j * (size_t)n};
        }
        uint8_t *blob = nullptr;
        const int rc = jpeg_encode_sets(c.ctx, s, sets, (int)ks.size(), n, quality, &blob);
        if (rc) return rc;
        res.add(blob);
        for (size_t j = 0; j < ks.size(); j++)
            for (int q = 0; q < n; q++) c.publish(file[p0 + q], ks[j], blob + sets[j].offs[q], sets[j].lens[q]);
        return IPX_OK;
    }
    // nothing per run: the chunk's frames are encoded together once its runs have all been through the operators
    int encode_run(const MixedCall &, hipStream_t, const int *, int, int, const Chunk &, ResultOwner &) const { return IPX_OK; }
    // A chunk whose every present output has one size for every file: one jpeg_encode_sets call, the one-size cost.  Any other chunk:
    // every present output of its files that are still IPX_OK in ONE jpeg_encode_mixed_core call, the records pointing at the frames
    // and coefficient scratch where the block already holds them.  Three waits for the device per chunk either way.
    int encode_chunk(const MixedCall &c, hipStream_t s, const int *file, int n, const Chunk &b, ResultOwner &res) const
    {
        bool uniform = true;
        for (int k = 0; k < kOuts && uniform; k++)
            if (!b.same_size[k])
                for (int p = 0; p < n && uniform; p++) uniform = !c.has(file[p], k);
        int rc = IPX_OK;
        if (uniform) {
            std::vector<int> ks;
            for (int k = 0; k < kOuts; k++) if (b.same_size[k]) ks.push_back(k);
            rc = encode(c, s, file, 0, n, b, ks, res);
        } else {
            std::vector<JpegEncSrc> fr;
            std::vector<std::pair<int, int>> owner_of;      // (file, output) of a frame
            for (int k = 0; k < kOuts; k++)
                for (int p = 0; p < n; p++) {
                    if (c.status[file[p]] != IPX_OK || !decoded(file[p]) || !c.has(file[p], k)) continue;
                    const OutShape sh = c.shape(file[p], k);
                    fr.push_back(JpegEncSrc{b.at(k, p), (int16_t *)(b.base[k] + b.coef_off[k][p]), sh.w, sh.h, sh.w * 4});
                    owner_of.emplace_back(file[p], k);
                }
            if (!fr.empty()) {
                std::vector<size_t> offs(fr.size()), lens(fr.size());
                uint8_t *blob = nullptr;
                rc = jpeg_encode_mixed_core(c.ctx, s, fr.data(), (int)fr.size(), quality, &blob, offs.data(), lens.data());
                if (!rc) {
                    res.add(blob);
                    for (size_t j = 0; j < fr.size(); j++) c.publish(owner_of[j].first, owner_of[j].second, blob + offs[j], lens[j]);
                }
            }
        }
        if (rc) return rc;
        (void)hipStreamSynchronize(s);                      // the next chunk takes the block over
        return IPX_OK;
    }
};
}  // namespace

extern "C" int ipx_run_jpeg_jpeg_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                                       ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    JpegMixed cx{quality, {}, {}};
    return mixed_leg(cx, ctx, ops, n, files, texts, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

// ---- host frames in, JPEG streams out: the worker's whole GPU leg ----------------------------------------------------------------

// frames of any source type in host memory through the plan, every output JPEG-encoded
static int run_host_jpeg_impl(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const BatchSrc &host, int quality, ipx_bytes *resize_out,
                              ipx_bytes *thumb_out, ipx_bytes *wm_out, ipx_jpeg_result **result)
{
    if (!result) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *result = nullptr;
    const int rc0 = src_check(who, pl, host, n, false);
    if (rc0 || n == 0) return rc0;
    const SrcLayout L = src_layout(pl, host);
    const size_t fsrc = L.frame_bytes();
    const PlanOutputs outs(pl, resize_out, thumb_out, wm_out, Codec::Jpeg, Codec::Jpeg, Codec::Jpeg);
    const size_t per_frame = fsrc + outs.frame_bytes();
    // every lane runs its own host thread: upload, operators, the three encodes together (two small read-backs) --
    // the threads block independently, so copies and kernels of different chunks overlap
    std::vector<Lane *> lanes;
    {
        std::unique_lock<std::mutex> lk(ctx->mu);
        ctx->cv.wait(lk, [&] { for (auto &l : ctx->lanes) if (l.busy) return false; return true; });
        for (auto &l : ctx->lanes) { l.busy = true; lanes.push_back(&l); }
    }
    const int nl = (int)lanes.size();
    int chunk = std::max(1, (n + 2 * nl - 1) / (2 * nl));
    chunk = (int)std::min<size_t>((size_t)chunk, std::max<size_t>(1, ctx->lane_bytes / per_frame));
    chunk = std::max(1, std::min(chunk, env_int("IPX_HOST_CHUNK_JPEG", 32)));
    ResultOwner res(ctx);
    std::mutex res_mu;
    std::atomic<int> next{0};
    std::atomic<int> status{IPX_OK};
    std::string err_text;
    const int nchunks = (n + chunk - 1) / chunk;
    auto worker = [&](Lane *l) {
        if (hipSetDevice(ctx->device) != hipSuccess) { status = IPX_ERR_HIP; return; }
        ResultOwner mine(ctx);                    // this lane's blocks, handed to `res` once its chunks are done
        int rc = lane_reserve(*l, per_frame * chunk + 256);
        for (int c = next.fetch_add(1); !rc && c < nchunks && status == IPX_OK; c = next.fetch_add(1)) {
            const int i0 = c * chunk, m = std::min(chunk, n - i0);
            uint8_t *dsrc = (uint8_t *)(((uintptr_t)l->dev + 255) & ~(uintptr_t)255);
            BatchSrc d;
            const hipError_t e = src_upload(host, L, i0, m, dsrc, chunk, l->stream, kCopyWholePlanes, &d);
            if (e != hipSuccess) { set_error("upload failed: %s", hipGetErrorString(e)); rc = IPX_ERR_HIP; break; }
            rc = run_chunk(ctx, l->stream, pl, outs, dsrc + fsrc * chunk, chunk, d, all_files(n), i0, m, nullptr, nullptr, quality, nullptr, mine);
        }
        {
            std::lock_guard<std::mutex> lk(res_mu);
            res.adopt(mine.release());
            if (rc && status == IPX_OK) { status = rc; err_text = ipx_last_error(); }
        }
        (void)hipStreamSynchronize(l->stream);
    };
    auto guarded = [&](Lane *l) {
        std::string text;
        const int rc = guarded_status([&] { worker(l); }, &text);
        if (!rc) return;
        (void)hipStreamSynchronize(l->stream);   // whatever the worker queued may still be reading the lane's scratch
        std::lock_guard<std::mutex> lk(res_mu);
        if (status == IPX_OK) { status = rc; err_text = text; }
    };
    HostPool::instance().parallel_for(nl, nl, [&](int i) { guarded(lanes[i]); });   // one host thread per lane (they block on their streams)
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (auto *l : lanes) l->busy = false;
    }
    ctx->cv.notify_all();
    if (status != IPX_OK) {
        ipx_jpeg_result_free(ctx, res.release());   // the chunks that did finish: freed BEFORE the text is set (ipx_host_free clears it)
        set_error("%s", err_text.c_str());
        return status;
    }
    *result = res.release();
    return IPX_OK;
}

extern "C" {

int ipx_plan_run_host_jpeg(ipx_ctx *ctx, const ipx_plan *pl, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                           int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    return run_host_jpeg_impl("ipx_plan_run_host_jpeg", ctx, pl, n, packed_src(kSrcRGBA, src, sstride, src_frame_stride), quality, resize_out, thumb_out,
                              wm_out, result);
}
IPX_CATCH_STATUS

int ipx_plan_run_host_ycbcr_jpeg(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_ycbcr_batch *src, int quality,
                                 ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    return run_host_jpeg_impl("ipx_plan_run_host_ycbcr_jpeg", ctx, pl, n, ycbcr_src(src), quality, resize_out, thumb_out, wm_out, result);
}
IPX_CATCH_STATUS

}  // extern "C"

// ---- compressed in, compressed out: image.Decode, the operators and jpeg.Encode without leaving the GPU ------
extern "C" {

// One part of a JPEG call on a lane of its own: the files of `sel`, all of one kind, are decoded and go chunk by chunk through
// run_chunk.  h0 == 0: three-component and Gray files, decoded to planes (jpeg_decode_files); h0 > 0: four-component files of that
// sampling vector (IPX_JPEG_CMYK=1; ipx_jpeg_dec_cmyk.hip), decoded to *image.CMYK frames that go through the plan as the deep CMYK
// source.  The decoders take files and statuses side by side: a selection through an index list is gathered for them and its statuses
// go back to at(g), one without is handed on where it lies.  texts: null, or the call's; the part draws texts[sel.at(g)] as a set of
// its own.  The jj_active slot, the lane arena and the timing line are the three-component parts'.
static int run_jpeg_part(const char *who, ipx_ctx *ctx, const ipx_plan *pl, const ipx_bytes *files, const ipx_text *texts, const FileSel &sel,
                         int h0, int quality, const PlanOutputs &outs, int *status, ipx_jpeg_result **result)
{
    IPX_ENTER(ctx);
    *result = nullptr;
    const int n = sel.n;
    if (n == 0) return IPX_OK;
    const bool four = h0 > 0;
    if (four && n > 65535) { for (int g = 0; g < n; g++) status[sel.at(g)] = IPX_ERR_UNSUPPORTED; return IPX_OK; }
    const bool dbg = !four && getenv("IPX_DEBUG") != nullptr;
    struct Slot {
        ipx_ctx *c;
        explicit Slot(ipx_ctx *ctx) : c(ctx)
        {
            const int cap = std::max(1, env_int("IPX_JPEG_JPEG_PARALLEL", 4));
            std::unique_lock<std::mutex> lk(c->mu);
            c->cv.wait(lk, [&] { return c->jj_active < cap; });
            c->jj_active++;
        }
        ~Slot()
        {
            { std::lock_guard<std::mutex> lk(c->mu); c->jj_active--; }
            c->cv.notify_all();
        }
    };
    std::optional<Slot> slot;
    if (!four) slot.emplace(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    LaneLease lane(ctx);
    const double t_lane = ms_since(t0);
    hipStream_t s = lane->stream;
    std::vector<ipx_bytes> gfiles(sel.idx ? n : 0);
    std::vector<int> gstatus(gfiles.size(), IPX_OK);
    for (size_t g = 0; g < gfiles.size(); g++) gfiles[g] = files[sel.idx[g]];
    const ipx_bytes *fl = sel.idx ? gfiles.data() : files + sel.first;
    int *st = sel.idx ? gstatus.data() : status + sel.first;
    int w = pl->p.sw, h = pl->p.sh, rc;
    BatchSrc src;                                             // the part's frames in HBM: no plane 0 when nothing was decodable
    ipx_jpeg_planes *owner = nullptr;
    if (four) {
        ipx_cmyk_batch frames{};
        std::fill(st, st + n, IPX_ERR_UNSUPPORTED);
        rc = jpeg_decode_cmyk_files(ctx, s, fl, n, &w, &h, h0, &frames, st, &owner);
        src = packed_src(kSrcCMYK, frames.pix, frames.stride, frames.frame_stride);
    } else {
        ipx_ycbcr_batch planes{};
        rc = n > 65535 ? IPX_ERR_UNSUPPORTED : jpeg_decode_files(ctx, s, env_int("IPX_JPEG_LANE_ARENA", 1) ? &lane.get() : nullptr, true, fl, n, &w, &h, &planes, st, &owner);
        src = ycbcr_src(&planes);                             // (ratio IPX_GRAY: only y is set)
        if (planes.ratio == IPX_GRAY) src.type = kSrcGray;
    }
    const double t_dec = ms_since(t0);
    for (size_t g = 0; g < gstatus.size(); g++) status[sel.idx[g]] = gstatus[g];
    if (rc || !src.plane[0]) return rc;                       // nothing decodable: every status says why
    struct Guard { ipx_ctx *c; ipx_jpeg_planes *o; ~Guard() { ipx_jpeg_planes_free(c, o); } } guard{ctx, owner};
    // (a coefficient buffer per output: the three encodes run stage by stage together, jpeg_encode_sets)
    const size_t per_frame = outs.frame_bytes();
    if (per_frame == 0) return IPX_OK;
    const int chunk = std::max(1, std::min(n, env_int("IPX_JPEG_JPEG_CHUNK", 256)));
    rc = lane_reserve(lane.get(), per_frame * chunk + 256);
    if (rc) return rc;
    const double t_res = ms_since(t0);
    ResultOwner res(ctx);
    LegTexts lt;                                              // uploaded once per part; chunk c0 draws texts c0 .. c0 + m of the set
    if ((rc = lt.build(s, who, pl, outs, texts, sel, true))) return rc;
    uint8_t *const block = (uint8_t *)(((uintptr_t)lane->dev + 255) & ~(uintptr_t)255);
    for (int c0 = 0; c0 < n && !rc; c0 += chunk)
        rc = run_chunk(ctx, s, pl, outs, block, chunk, src.from(c0), sel, c0, std::min(chunk, n - c0), &lt, nullptr, quality, status, res);
    (void)hipStreamSynchronize(s);
    if (dbg) fprintf(stderr, "[ipx] jpeg->jpeg part of %d files: lane after %.1f ms, decoded at %.1f, scratch at %.1f, done at %.1f\n", n, t_lane, t_dec, t_res, ms_since(t0));
    if (rc) return rc;
    *result = res.release();
    return IPX_OK;
}

// the three-component and Gray files of a call (every file, without IPX_JPEG_CMYK=1)
static int run_jpeg_jpeg_ycbcr(const char *who, ipx_ctx *ctx, const ipx_plan *pl, const ipx_bytes *files, const ipx_text *texts, const FileSel &sel,
                               int quality, const PlanOutputs &outs, int *status, ipx_jpeg_result **result)
{
    *result = nullptr;
    // a large batch is cut into parts that run on lanes of their own, one host thread each: while one part is in its (host-paced)
    // encode read-backs another decodes.  Two callers with 1024 files each measured 15 k images/s against 11.7 k for one.
    // Four parts of 256 measured 9 % above two of 512 or three of 341 (tools/j2j_parts.sh: 55.3 ms against 60.4 per 1024 files); more
    // than four gain nothing.  One lane stays free for a per-operator call that arrives while the batch runs.
    const int n = sel.n, nl = (int)ctx->lanes.size();
    const int parts = std::max(1, std::min({nl >= 3 ? nl - 1 : nl, n / std::max(1, env_int("IPX_JPEG_JPEG_PART", 256)), env_int("IPX_JPEG_JPEG_MAXPARTS", 4)}));
    if (parts == 1) return run_jpeg_part(who, ctx, pl, files, texts, sel, 0, quality, outs, status, result);
    std::vector<ipx_jpeg_result *> res(parts, nullptr);
    std::vector<int> rcs(parts, IPX_OK);
    std::vector<std::string> errs(parts);
    auto work = [&](int k) {
        const int g0 = (int)((long long)n * k / parts), g1 = (int)((long long)n * (k + 1) / parts);
        rcs[k] = run_jpeg_part(who, ctx, pl, files, texts, sel.slice(g0, g1 - g0), 0, quality, outs, status, &res[k]);
        if (rcs[k]) errs[k] = ipx_last_error();
    };
    auto guarded = [&](int k) { const int rc = guarded_status([&] { work(k); }, &errs[k]); if (rc) rcs[k] = rc; };
    HostPool::instance().parallel_for(parts, parts, [&](int k) { guarded(k); });      // one host thread per part (each drives a lane)
    ResultOwner all(ctx);
    int rc = IPX_OK;
    for (int k = 0; k < parts; k++) {
        all.adopt(res[k]);
        if (rcs[k] && !rc) { rc = rcs[k]; set_error("%s", errs[k].c_str()); }
    }
    if (rc) return rc;
    *result = all.release();
    return IPX_OK;
}

// the body of ipx_plan_run_jpeg_jpeg (texts == NULL: no text launch) and ipx_plan_run_jpeg_jpeg_texts.  Under IPX_JPEG_CMYK=1 the
// four-component files are taken out of the call and run as sub-batches of one sampling vector each; the rest runs as it always did.
// All three are selections of the call's files handed to the same part runner, which reaches the caller's arrays through them.
static int run_jpeg_jpeg(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                         ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result)
{
    const PlanOutputs outs(pl, resize_out, thumb_out, wm_out, Codec::Jpeg, Codec::Jpeg, Codec::Jpeg);
    outs.clear(n);
    std::vector<int> four[2], rest;
    if (jpeg_cmyk_enabled())
        for (int i = 0; i < n; i++) {
            const int h0 = jpeg_cmyk_peek(files[i].data, files[i].len);
            if (h0) four[h0 - 1].push_back(i); else rest.push_back(i);
        }
    if (four[0].empty() && four[1].empty()) return run_jpeg_jpeg_ycbcr(who, ctx, pl, files, texts, all_files(n), quality, outs, status, result);
    ResultOwner all(ctx);
    for (int v = 0; v < 3; v++) {                             // the rest, then the two vectors
        const std::vector<int> &of = v ? four[v - 1] : rest;
        const FileSel sel{of.data(), 0, (int)of.size()};
        ipx_jpeg_result *r = nullptr;
        const int rc = v ? run_jpeg_part(who, ctx, pl, files, texts, sel, v, quality, outs, status, &r)
                         : run_jpeg_jpeg_ycbcr(who, ctx, pl, files, texts, sel, quality, outs, status, &r);
        all.adopt(r);
        if (rc) return rc;
    }
    *result = all.release();
    return IPX_OK;
}

int ipx_plan_run_jpeg_jpeg(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, int quality, ipx_bytes *resize_out,
                           ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (const int rc = leg_entry_check("ipx_plan_run_jpeg_jpeg", pl, n, files, status, result, false, nullptr)) return rc;
    return run_jpeg_jpeg("ipx_plan_run_jpeg_jpeg", ctx, pl, n, files, nullptr, quality, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

int ipx_plan_run_jpeg_jpeg_texts(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                                 ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (const int rc = leg_entry_check("ipx_plan_run_jpeg_jpeg_texts", pl, n, files, status, result, true, texts)) return rc;
    return run_jpeg_jpeg("ipx_plan_run_jpeg_jpeg_texts", ctx, pl, n, files, texts, quality, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

}  // extern "C"
