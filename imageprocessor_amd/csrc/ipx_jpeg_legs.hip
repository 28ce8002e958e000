// ipx_jpeg_legs.hip -- the mixed-size JPEG-in, JPEG-out leg (ipx_run_jpeg_jpeg_mixed): a plan per size, the cut of
// ipx_png_mixed_plan.h with the sampling class as the kind, one decode pass per group (jpeg_mixed_decode in ipx_jpeg_dec_runtime.hip),
// the operators per run, jpeg.Encode through jpeg_encode_sets.  The uniform leg is in ipx_jpeg_runtime.hip.  DESIGN.md sections 4.6 and 7.
#include <vector>

#include "ipx_decode_common.h"
#include "ipx_png_mixed_plan.h"
#include "ipx_size_plans.h"

namespace {

const char who[] = "ipx_run_jpeg_jpeg_mixed";

// what the steps of one call share: the caller's arrays, the parse, and every file's plan
struct MixedCall {
    ipx_ctx *ctx;
    const ipx_text *texts;
    ipx_bytes *const *dst;                  // [kOuts]; null: the output is not asked for
    int *status;
    int quality;
    const JpegBatchPlan &parsed;
    std::vector<ipx_plan *> plan_of;        // null: the file is not OK
    OutShape shape(int i, int k) const { return out_shape(plan_of[i]->info, k); }
    // an output that is wanted, made and not empty for file i: its frames lie fs apart in the chunk's arena, its coefficient scratch coef
    bool has(int i, int k) const { const OutShape sh = shape(i, k); return dst[k] && sh.bytes && sh.w > 0 && sh.h > 0; }
    size_t out_fs(int i, int k) const { return has(i, k) ? align256(shape(i, k).bytes) : 0; }
    size_t out_coef(int i, int k) const { return has(i, k) ? align256(ipx_jpeg_coef_count(shape(i, k).w, shape(i, k).h) * sizeof(int16_t)) : 0; }
};

// the sampling class of a parsed file as one number: the cut's kind
int class_of(const JpegDecInfo &I) { return I.ncomp == 1 ? 0 : I.h0 * 4 + I.v0; }

// bytes a file costs its decode group: the MCU-padded planes and the coefficient scratch (128 bytes per block and its DC value)
size_t decode_cost(const JpegDecInfo &I)
{
    const size_t mxx = (size_t)(I.w + 8 * I.h0 - 1) / (8 * I.h0), myy = (size_t)(I.h + 8 * I.v0 - 1) / (8 * I.v0);
    const size_t y = align256(64 * I.h0 * I.v0 * mxx * myy), c = I.ncomp == 1 ? 0 : align256(64 * mxx * myy);
    return y + 2 * c + mxx * myy * (I.ncomp == 1 ? 1 : I.h0 * I.v0 + 2) * 130 + 8192;
}

// a chunk's device block: per output the frames of every file, then the coefficient scratch of every file; file p's at off[k][p]
struct ChunkBlock {
    std::vector<size_t> frame_off[kOuts], coef_off[kOuts];
    size_t bytes = 0;
    uint8_t *base = nullptr;
    bool same_size[kOuts] = {false, false, false};      // every file of the chunk has this output, of one size: one encode per chunk
};
ChunkBlock chunk_block(const MixedCall &c, const int *file, int n)
{
    ChunkBlock b;
    for (int k = 0; k < kOuts; k++) {
        b.frame_off[k].resize(n);
        for (int p = 0; p < n; p++) { b.frame_off[k][p] = b.bytes; b.bytes += c.out_fs(file[p], k); }
    }
    for (int k = 0; k < kOuts; k++) {
        b.coef_off[k].resize(n);
        for (int p = 0; p < n; p++) { b.coef_off[k][p] = b.bytes; b.bytes += c.out_coef(file[p], k); }
        b.same_size[k] = c.has(file[0], k);
        for (int p = 1; p < n && b.same_size[k]; p++)
            b.same_size[k] = c.has(file[p], k) && c.shape(file[p], k).w == c.shape(file[0], k).w && c.shape(file[p], k).h == c.shape(file[0], k).h;
    }
    return b;
}

// jpeg.Encode of the outputs `ks` of files [p0, p0 + n) of the chunk -- every one of them has each of these outputs, of one size, so an
// output's frames are one frame stride apart -- in one jpeg_encode_sets call; the OK files' streams are handed out
int mixed_encode(const MixedCall &c, hipStream_t s, const int *file, int p0, int n, const ChunkBlock &b, const std::vector<int> &ks, ResultOwner &res)
{
    if (ks.empty()) return IPX_OK;
    std::vector<size_t> offs(ks.size() * (size_t)n), lens(ks.size() * (size_t)n);
    JpegEncSet sets[kOuts];
    for (size_t j = 0; j < ks.size(); j++) {
        const int k = ks[j];
        const OutShape sh = c.shape(file[p0], k);
        sets[j] = JpegEncSet{(int16_t *)(b.base + b.coef_off[k][p0]), b.base + b.frame_off[k][p0], sh.w, sh.h, sh.w * 4, c.out_fs(file[p0], k),
                             offs.data() + j * (size_t)n, lens.data() + j * (size_t)n};
    }
    uint8_t *blob = nullptr;
    const int rc = jpeg_encode_sets(c.ctx, s, sets, (int)ks.size(), n, c.quality, &blob);
    if (rc) return rc;
    res.add(blob);
    for (size_t j = 0; j < ks.size(); j++)
        for (int q = 0; q < n; q++)
            if (c.status[file[p0 + q]] == IPX_OK) c.dst[ks[j]][file[p0 + q]] = ipx_bytes{blob + sets[j].offs[q], sets[j].lens[q]};
    return IPX_OK;
}

// one run -- files [p0, p0 + n) of the chunk, of one size and class, their planes one frame stride apart from frames[file[p0]] on: the
// operators into the run's slice of the chunk's block, its texts in one launch, and the encode of the outputs that are not the
// chunk's to encode
int mixed_run(const MixedCall &c, hipStream_t s, const ipx_jpeg_frame *frames, const int *file, int p0, int n, const ChunkBlock &b, AsyncFree *omem,
              ResultOwner &res)
{
    const int i0 = file[p0];
    const ipx_plan *pl = c.plan_of[i0];
    const JpegDecInfo &I = c.parsed.info[i0];
    const ipx_jpeg_frame &f = frames[i0];
    BatchSrc d;
    d.type = f.ratio == IPX_GRAY ? kSrcGray : kSrcYCbCr;
    d.ratio = f.ratio;
    d.plane[0] = f.y; d.plane[1] = f.cb; d.plane[2] = f.cr;
    d.stride[0] = f.ystride; d.stride[1] = f.cstride;
    const size_t myy = (size_t)(I.h + 8 * I.v0 - 1) / (8 * I.v0);
    d.frame_stride[0] = align256((size_t)f.ystride * 8 * I.v0 * myy); d.frame_stride[1] = align256((size_t)f.cstride * 8 * myy);
    BatchDst bd;
    std::vector<int> ks;
    for (int k = 0; k < kOuts; k++)
        if (const size_t fs = c.out_fs(i0, k)) {
            bd.out[k] = b.base + b.frame_off[k][p0]; bd.frame_stride[k] = fs;
            if (!b.same_size[k]) ks.push_back(k);
        }
    if (!bd.out[0] && !bd.out[1] && !bd.out[2]) return IPX_OK;
    int rc = run_dev_src(c.ctx, s, pl, n, d, bd);
    if (rc) return rc;
    if (c.texts && pl->p.do_watermark && bd.out[kOutWm]) {
        const OutShape sh = c.shape(i0, kOutWm);
        std::vector<ipx_text> own(n);
        for (int q = 0; q < n; q++) own[q] = c.texts[file[p0 + q]];
        ipx_textset ts;                             // (its memory goes back in stream order, behind the launch)
        if ((rc = textset_build(s, who, own.data(), n, sh.w, sh.h, &ts))) return rc;
        if ((rc = dev_composite_texts(s, omem, bd.out[kOutWm], sh.w * 4, bd.frame_stride[kOutWm], n, ts, 0, nullptr))) return rc;
    }
    return mixed_encode(c, s, file, p0, n, b, ks, res);
}

}  // namespace

extern "C" {

// The JPEG leg for uploads of any sizes and samplings: one parse; a plan per size from the context's cache; the cut of
// ipx_png_mixed_plan.h with the sampling class as the kind (order by size and class, decode groups, chunks, runs); per group ONE
// jpeg_mixed_decode call, which is one decode pass per sampling class whatever sizes it holds; per chunk the operators once per run into
// the run's slice of the chunk's block; the outputs every file of the chunk has in one size are encoded once per chunk, the others once
// per run (jpeg_encode_sets: three waits for the device per call).
int ipx_run_jpeg_jpeg_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                            ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (!ops || n < 0 || !result || (n && (!files || !status))) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *result = nullptr;
    if (texts && (ops->glyphs || ops->n_glyphs)) {
        set_error("%s: a text per file needs ops->glyphs == NULL: the plan copies the frame and the texts are drawn behind it", who);
        return IPX_ERR_INVALID;
    }
    if (n > 65535) { set_error("%s: at most 65535 files per call", who); return IPX_ERR_UNSUPPORTED; }
    if (texts)
        if (const int rc = texts_check(who, texts, n)) return rc;
    ipx_bytes *const dst[kOuts] = {resize_out, thumb_out, wm_out};
    for (int k = 0; k < kOuts; k++)
        if (dst[k])
            for (int i = 0; i < n; i++) dst[k][i] = ipx_bytes{nullptr, 0};
    if (n == 0) return IPX_OK;
    JpegBatchPlan parsed;
    int rc = jpeg_mixed_parse(files, n, status, &parsed);
    if (rc) return rc;
    // given up in reverse order: the plans go back last, behind everything that ran through them
    SizePlans plans(ctx);
    MixedCall c{ctx, texts, dst, status, quality, parsed, {}};
    {
        std::vector<int> w(n), h(n);
        for (int i = 0; i < n; i++) { w[i] = parsed.info[i].w; h[i] = parsed.info[i].h; }
        if ((rc = size_plans_acquire(ctx, ops, n, w.data(), h.data(), status, plans, &c.plan_of))) return rc;
    }
    std::vector<MixItem> items(n);
    for (int i = 0; i < n; i++) {
        MixItem &it = items[i];
        it = MixItem{status[i] == IPX_OK, parsed.info[i].w, parsed.info[i].h, 0, 0, 0};
        if (!it.ok) continue;
        it.kind = class_of(parsed.info[i]);
        it.frame_bytes = decode_cost(parsed.info[i]);
        for (int k = 0; k < kOuts; k++) it.chunk_bytes += c.out_fs(i, k) + 2 * c.out_coef(i, k);      // (the encoder's streams: about the coefficients again)
    }
    const int group_max = std::min(65535, std::max(1, env_int("IPX_JPEG_MIXED_GROUP", 256)));
    const size_t chunk_bytes = (size_t)std::max(0, env_int("IPX_JPEG_MIXED_CHUNK_MB", 8192)) << 20;
    const MixCut cut = png_mixed_cut(items.data(), n, group_max, (size_t)4 << 30, chunk_bytes);
    const bool trace = env_int("IPX_DEBUG_J2J", 0) != 0;
    if (trace) fprintf(stderr, "[ipx] %s: %d files, %zu groups, %zu chunks, %zu runs\n", who, n, cut.groups.size(), cut.chunks.size(), cut.runs.size());
    ResultOwner res(ctx);
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    std::vector<ipx_jpeg_frame> frames(n, ipx_jpeg_frame{});
    for (const MixGroup &grp : cut.groups) {
        StreamSync sync{s};
        OwnedBlocks<ipx_jpeg_planes> planes(ctx, s);            // the group's planes: they go back, in stream order, with the group
        rc = jpeg_mixed_decode(ctx, s, env_int("IPX_JPEG_LANE_ARENA", 1) ? &lane.get() : nullptr, files, parsed, cut.order.data() + grp.first, grp.n,
                               planes, frames.data(), status);
        if (rc) return rc;
        for (int ci = grp.chunk0; ci < grp.chunk0 + grp.nchunks; ci++) {
            const MixChunk &ch = cut.chunks[ci];
            const int *file = cut.order.data() + ch.first;          // the chunk's files, by the caller's index
            bool any = false;
            for (int p = 0; p < ch.n; p++) any |= status[file[p]] == IPX_OK;
            if (!any) continue;
            ChunkBlock b = chunk_block(c, file, ch.n);
            if (!b.bytes) continue;
            if ((rc = lane_reserve(lane.get(), b.bytes + 256))) return rc;
            b.base = (uint8_t *)(((uintptr_t)lane->dev + 255) & ~(uintptr_t)255);
            AsyncFree omem{s, {}};
            for (int r = ch.run0; r < ch.run0 + ch.nruns; r++) {
                const MixRun &run = cut.runs[r];
                // (a run whose first file failed in the decode has no planes to start from: its files run one by one)
                if (frames[file[run.first - ch.first]].y) { rc = mixed_run(c, s, frames.data(), file, run.first - ch.first, run.n, b, &omem, res); if (rc) return rc; continue; }
                for (int q = 0; q < run.n; q++)
                    if (frames[file[run.first - ch.first + q]].y)
                        if ((rc = mixed_run(c, s, frames.data(), file, run.first - ch.first + q, 1, b, &omem, res))) return rc;
            }
            std::vector<int> ks;
            for (int k = 0; k < kOuts; k++) if (b.same_size[k]) ks.push_back(k);
            if ((rc = mixed_encode(c, s, file, 0, ch.n, b, ks, res))) return rc;
            (void)hipStreamSynchronize(s);                          // the next chunk takes the block over
        }
    }
    *result = res.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

}  // extern "C"
