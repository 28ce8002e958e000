// ipx_png_legs.hip -- the two PNG-in, PNG-out legs: the uniform one (ipx_plan_run_png_png and its _texts twin: one plan, every file of
// the plan's size) and the mixed-size one (ipx_run_png_png_mixed: a plan per size, cut by ipx_png_mixed_plan.h).  Both parse and decode
// through ipx_png_dec_runtime.hip and encode through ipx_png.hip / ipx_png_mixed.hip.  DESIGN.md sections 4.10 and 7.
#include <map>
#include <vector>

#include "ipx_png.h"
#include "ipx_png_dec.h"
#include "ipx_png_mixed_plan.h"
#include "ipx_size_plans.h"
#include "ipx_decode_common.h"

// ---- the PNG leg -----------------------------------------------------------------------------------------------------------------

extern "C" {

// The PNG task's GPU leg from the uploads on: the host parse of every file, then per kind, per decode group (IPX_HOST_CHUNK_PNG_DEC
// files, at most ~4 GiB of frames): upload, CRC, inflate and unfilter into HBM; then per chunk of IPX_HOST_CHUNK_PNG frames the
// operators on frames of that kind and png.Encode of all three outputs (run_chunk).  The operators run on every slot of a chunk (a failed file's slot
// holds whatever its frame holds); only OK files' streams are handed out.
// (the body of ipx_plan_run_png_png -- texts == NULL: no text launch -- and of ipx_plan_run_png_png_texts, where texts[i] is drawn on
// file i's watermark frame between the operators and the encoder: one text set per call, indexed by the caller's index; the files are
// sorted by kind here, so a group is a selection through its idx and run_chunk takes texts, statuses and output slots through it)
static int run_png_png(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, const ipx_text *texts,
                       ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result)
{
    *result = nullptr;
    const int sw = pl->p.sw, sh = pl->p.sh;
    const PlanOutputs outs(pl, resize_out, thumb_out, wm_out, Codec::Png, Codec::Png, Codec::Png);
    outs.clear(n);
    if (n == 0) return IPX_OK;
    std::vector<PngFileInfo> info(n);
    int rc = png_parse_all(files, n, info, status);
    if (rc) return rc;
    for (int i = 0; i < n; i++)
        if (status[i] == IPX_OK && (info[i].w != sw || info[i].h != sh)) status[i] = IPX_ERR_UNSUPPORTED;
    const size_t per_out = outs.frame_bytes();
    const int chunk_max = std::max(1, env_int("IPX_HOST_CHUNK_PNG", 64)), group_max = std::max(1, env_int("IPX_HOST_CHUNK_PNG_DEC", 1024));
    ResultOwner res(ctx);
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    LegTexts lt;                        // one set per call, indexed by the caller's index: a group's chunks select through its idx
    if ((rc = lt.build(s, who, pl, outs, texts, all_files(n), false))) return rc;
    for (int kind = 0; kind < kPngKinds; kind++) {
        std::vector<int> of_kind;
        for (int i = 0; i < n; i++)
            if (status[i] == IPX_OK && info[i].kind == kind) of_kind.push_back(i);
        if (of_kind.empty()) continue;
        const int kb = png_kind_bpp(kind);
        const size_t fs = align256((size_t)sw * sh * kb);
        const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)group_max, ((size_t)4 << 30) / (fs + 1024)));
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)chunk_max, per_out ? ((size_t)1 << 30) / per_out : (size_t)chunk_max));
        for (size_t g0 = 0; g0 < of_kind.size(); g0 += group) {
            const int m = (int)std::min<size_t>(group, of_kind.size() - g0);
            const PngFrameLayout at = png_layout_strided(std::vector<int>(of_kind.begin() + g0, of_kind.begin() + g0 + m), fs, false);
            const std::vector<int> &idx = at.idx;
            StreamSync sync{s};
            AsyncFree mem{s, {}};
            uint8_t *dfr, *dpal = nullptr;
            IPX_HIP(mem.get(&dfr, at.bytes));
            if (kind == IPX_PNG_PALETTED) IPX_HIP(mem.get(&dpal, (size_t)1024 * at.pal_slots));
            rc = png_decode_files(ctx, s, files, at, info, dfr, dpal, status);
            if (rc) return rc;
            for (int c0 = 0; c0 < m; c0 += chunk) {
                const int cm = std::min(chunk, m - c0);
                bool any = false;
                for (int g = c0; g < c0 + cm; g++) any |= status[idx[g]] == IPX_OK;
                if (!any) continue;
                AsyncFree omem{s, {}};
                uint8_t *dout = nullptr;
                if (per_out) IPX_HIP(omem.get(&dout, per_out * cm));
                const BatchSrc d = packed_src(src_of_png(kind), dfr, sw * kb, fs, dpal).from(c0);
                // (idx outlives the group's wait for the stream, and with it the copy of this chunk's slice in omem)
                rc = run_chunk(ctx, s, pl, outs, dout, cm, d, FileSel{idx.data(), 0, m}, c0, cm, &lt, &omem, 0, status, res);
                if (rc) return rc;
            }
        }
    }
    *result = res.release();
    return IPX_OK;
}

int ipx_plan_run_png_png(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, ipx_bytes *resize_out, ipx_bytes *thumb_out,
                         ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (const int rc = leg_entry_check("ipx_plan_run_png_png", pl, n, files, status, result, false, nullptr)) return rc;
    return run_png_png("ipx_plan_run_png_png", ctx, pl, n, files, nullptr, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

int ipx_plan_run_png_png_texts(ipx_ctx *ctx, const ipx_plan *pl, int n, const ipx_bytes *files, const ipx_text *texts, ipx_bytes *resize_out,
                               ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (const int rc = leg_entry_check("ipx_plan_run_png_png_texts", pl, n, files, status, result, true, texts)) return rc;
    return run_png_png("ipx_plan_run_png_png_texts", ctx, pl, n, files, texts, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

}  // extern "C"

// ---- the mixed-size PNG leg ------------------------------------------------------------------------------------------------------

namespace {
// what output k of a plan costs a chunk: the frame itself and the encoder's scratch for it -- the filtered stream, a word of match
// scratch per filtered byte, and the frame's region
size_t mixed_out_cost(const OutShape &sh)
{
    if (!sh.bytes || sh.w <= 0 || sh.h <= 0) return 0;
    const size_t filt = (size_t)sh.h * (1 + 4 * (size_t)sh.w);
    return align256(sh.bytes) + 5 * align256(filt) + align256(kPngSegBase + png_segs_bytes(sh.w, sh.h, 4) + kPngTailBytes);
}

const char who[] = "ipx_run_png_png_mixed";

// what the steps of one call share: the caller's arrays, the parse, and every file's plan
struct MixedCall {
    ipx_ctx *ctx;
    const ipx_text *texts;
    ipx_bytes *const *dst;                  // [kOuts]; null: the output is not asked for
    int *status;
    const std::vector<PngFileInfo> &info;
    std::vector<ipx_plan *> plan_of;        // null: the file is not OK
    // how far apart the frames of file i's size lie in the arena of output k; 0: no such output
    size_t out_fs(int i, int k) const { return dst[k] ? align256(out_shape(plan_of[i]->info, k).bytes) : 0; }
};

// a plan per size (ipx_size_plans.h); files of a size no plan can be made for get ipx_plan_create's status, alone
int mixed_plans(MixedCall &c, const ipx_pool_ops *ops, int n, SizePlans &plans)
{
    std::vector<int> w(n), h(n);
    for (int i = 0; i < n; i++) { w[i] = c.info[i].w; h[i] = c.info[i].h; }
    return size_plans_acquire(c.ctx, ops, n, w.data(), h.data(), c.status, plans, &c.plan_of);
}

// a chunk's three arenas: file p's frame of output k at arena[k] + off[k][p]
struct ChunkArenas {
    std::vector<size_t> off[kOuts];
    uint8_t *arena[kOuts] = {nullptr, nullptr, nullptr};
};
int mixed_arenas(const MixedCall &c, const int *file, int n, AsyncFree &omem, ChunkArenas &a)
{
    for (int k = 0; k < kOuts; k++) {
        a.off[k].resize(n);
        size_t total = 0;
        for (int p = 0; p < n; p++) { a.off[k][p] = total; total += c.out_fs(file[p], k); }
        if (total) IPX_HIP(omem.get(&a.arena[k], total));
    }
    return IPX_OK;
}

// one run -- files [p0, p0 + n) of the chunk, of one size and kind, decoded at d: the operators into the run's slice of the arenas,
// then its texts in one launch
int mixed_run(const MixedCall &c, hipStream_t s, const BatchSrc &d, const int *file, int p0, int n, const ChunkArenas &a, AsyncFree *omem)
{
    const int i0 = file[p0];
    const ipx_plan *pl = c.plan_of[i0];
    BatchDst bd;
    for (int k = 0; k < kOuts; k++)
        if (const size_t fs = c.out_fs(i0, k)) { bd.out[k] = a.arena[k] + a.off[k][p0]; bd.frame_stride[k] = fs; }
    int rc = run_dev_src(c.ctx, s, pl, n, d, bd);
    if (rc) return rc;
    if (c.texts && pl->p.do_watermark && bd.out[kOutWm]) {
        const OutShape sh = out_shape(pl->info, kOutWm);
        std::vector<ipx_text> own(n);
        for (int q = 0; q < n; q++) own[q] = c.texts[file[p0 + q]];
        ipx_textset ts;                             // (its memory goes back in stream order, behind the launch)
        if ((rc = textset_build(s, who, own.data(), n, sh.w, sh.h, &ts))) return rc;
        if ((rc = dev_composite_texts(s, omem, bd.out[kOutWm], sh.w * 4, bd.frame_stride[kOutWm], n, ts, 0, nullptr))) return rc;
    }
    return IPX_OK;
}

// one mixed-size png.Encode per present output over every frame of the chunk; the OK files' streams are handed out
int mixed_encode(const MixedCall &c, hipStream_t s, const int *file, int n, const ChunkArenas &a, ResultOwner &res)
{
    for (int k = 0; k < kOuts; k++) {
        std::vector<ipx_rgba_frame> fr;
        std::vector<int> owner_of;
        for (int p = 0; p < n; p++) {
            const OutShape sh = out_shape(c.plan_of[file[p]]->info, k);
            if (!c.out_fs(file[p], k) || sh.w <= 0 || sh.h <= 0) continue;
            fr.push_back(ipx_rgba_frame{a.arena[k] + a.off[k][p], sh.w, sh.h, sh.w * 4});
            owner_of.push_back(file[p]);
        }
        if (fr.empty()) continue;
        std::vector<size_t> offs(fr.size()), lens(fr.size());
        uint8_t *blob = nullptr;
        const int rc = png_encode_mixed_core(c.ctx, s, fr.data(), (int)fr.size(), &blob, offs.data(), lens.data());
        if (rc) return rc;
        res.add(blob);
        for (size_t j = 0; j < fr.size(); j++)
            if (c.status[owner_of[j]] == IPX_OK) c.dst[k][owner_of[j]] = ipx_bytes{blob + offs[j], lens[j]};
    }
    return IPX_OK;
}
}  // namespace

extern "C" {

// The PNG leg for uploads of any sizes and kinds: the host parse; a plan per size from the context's cache; the cut of
// ipx_png_mixed_plan.h (order by size and kind, decode groups, chunks, runs); per group ONE png_decode_files call whatever it holds;
// per chunk the operators once per run, into the run's slice of three arenas, its texts in one launch from a set clipped to its size;
// then one mixed-size png.Encode per present output over every frame of the chunk.  The host does not wait for the stream between
// runs beyond what those stages contain (the upload of a run's texts).
int ipx_run_png_png_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts,
                          ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    if (!ops || n < 0 || !result || (n && (!files || !status))) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *result = nullptr;
    if (ops->sw != 0 || ops->sh != 0) { set_error("%s: ops->sw and ops->sh must be 0: every file's own size is used", who); return IPX_ERR_INVALID; }
    if (ops->glyphs || ops->n_glyphs) {
        set_error("%s: ops->glyphs must be NULL: a positioned glyph list is anchored for one frame size; pass a text per file", who);
        return IPX_ERR_INVALID;
    }
    if (texts)
        if (const int rc = texts_check(who, texts, n)) return rc;
    ipx_bytes *const dst[kOuts] = {resize_out, thumb_out, wm_out};
    for (int k = 0; k < kOuts; k++)
        if (dst[k])
            for (int i = 0; i < n; i++) dst[k][i] = ipx_bytes{nullptr, 0};
    if (n == 0) return IPX_OK;
    std::vector<PngFileInfo> info(n);
    int rc = png_parse_all(files, n, info, status);
    if (rc) return rc;
    // given up in reverse order: the plans go back last, behind everything that ran through them
    SizePlans plans(ctx);
    MixedCall c{ctx, texts, dst, status, info, {}};
    if ((rc = mixed_plans(c, ops, n, plans))) return rc;
    std::vector<MixItem> items(n);
    for (int i = 0; i < n; i++) {
        MixItem &it = items[i];
        it = MixItem{status[i] == IPX_OK, info[i].w, info[i].h, info[i].kind, 0, 0};
        if (!it.ok) continue;
        it.frame_bytes = align256((size_t)it.w * it.h * png_kind_bpp(it.kind)) + 1024;
        for (int k = 0; k < kOuts; k++)
            if (dst[k]) it.chunk_bytes += mixed_out_cost(out_shape(c.plan_of[i]->info, k));
    }
    const int group_max = std::min(65535, std::max(1, env_int("IPX_HOST_CHUNK_PNG_DEC", 1024)));
    const size_t chunk_bytes = (size_t)std::max(0, env_int("IPX_PNG_MIXED_CHUNK_MB", 1024)) << 20;
    const MixCut cut = png_mixed_cut(items.data(), n, group_max, (size_t)4 << 30, chunk_bytes);
    ResultOwner res(ctx);
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    for (const MixGroup &grp : cut.groups) {
        const PngFrameLayout at = png_layout_packed(std::vector<int>(cut.order.begin() + grp.first, cut.order.begin() + grp.first + grp.n),
                                                    [&](int i) { return png_frame_need(info[i]); });
        StreamSync sync{s};
        AsyncFree mem{s, {}};
        uint8_t *dfr, *dpal = nullptr;
        IPX_HIP(mem.get(&dfr, at.bytes));
        if (at.pal_slots) IPX_HIP(mem.get(&dpal, (size_t)1024 * at.pal_slots));
        rc = png_decode_files(ctx, s, files, at, info, dfr, dpal, status);     // every size and kind of the group at once
        if (rc) return rc;
        for (int ci = grp.chunk0; ci < grp.chunk0 + grp.nchunks; ci++) {
            const MixChunk &ch = cut.chunks[ci];
            const int *file = cut.order.data() + ch.first;          // the chunk's files, by the caller's index
            bool any = false;
            for (int p = 0; p < ch.n; p++) any |= status[file[p]] == IPX_OK;
            if (!any) continue;
            AsyncFree omem{s, {}};
            ChunkArenas a;
            if ((rc = mixed_arenas(c, file, ch.n, omem, a))) return rc;
            for (int r = ch.run0; r < ch.run0 + ch.nruns; r++) {
                const MixRun &run = cut.runs[r];
                const int g0 = run.first - grp.first;
                const PngFileInfo &f = info[at.idx[g0]];
                const int kb = png_kind_bpp(f.kind);
                const BatchSrc d = packed_src(src_of_png(f.kind), dfr + at.off[g0], f.w * kb, align256((size_t)f.w * f.h * kb),
                                              at.pal_slot[g0] >= 0 ? dpal + (size_t)at.pal_slot[g0] * 1024 : nullptr);
                if ((rc = mixed_run(c, s, d, file, run.first - ch.first, run.n, a, &omem))) return rc;
            }
            if ((rc = mixed_encode(c, s, file, ch.n, a, res))) return rc;
        }
    }
    *result = res.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

}  // extern "C"
