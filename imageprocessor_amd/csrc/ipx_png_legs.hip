// ipx_png_legs.hip -- the two PNG-in, PNG-out legs: the uniform one (ipx_plan_run_png_png and its _texts twin: one plan, every file of
// the plan's size) and what PNG supplies to the mixed-size one (ipx_run_png_png_mixed: the walk is mixed_leg in ipx_mixed_leg.h).  Both
// parse and decode through ipx_png_dec_runtime.hip and encode through ipx_png.hip / ipx_png_mixed.hip.  DESIGN.md sections 4.10 and 7.
#include <vector>

#include "ipx_png.h"
#include "ipx_png_dec.h"
#include "ipx_mixed_leg.h"

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

// ---- the mixed-size PNG leg: what PNG supplies to the walk of ipx_mixed_leg.h --------------------------------------------------------

namespace {
struct PngMixed {
    static constexpr const char *kWho = "ipx_run_png_png_mixed";
    static constexpr const char *kGroupEnv = "IPX_HOST_CHUNK_PNG_DEC", *kChunkEnv = "IPX_PNG_MIXED_CHUNK_MB";
    static constexpr int kGroupFiles = 1024, kChunkMB = 1024;
    // the operators run on every slot of every run, whatever the decode did to a file (a failed file's slot holds whatever its frame
    // holds), and on a run no output is made for
    static constexpr bool kRunsWithoutOutputs = true;
    bool decoded(int) const { return true; }

    std::vector<PngFileInfo> info;
    // a group's frames and palettes: stream-ordered, they go back with the group
    struct Group {
        AsyncFree mem;
        PngFrameLayout at;
        uint8_t *dfr = nullptr, *dpal = nullptr;
        Group(ipx_ctx *, hipStream_t s) : mem{s, {}} {}
    };
    using Chunk = ChunkFrames;              // three arenas

    int refuse(const ipx_pool_ops *ops, int, const ipx_text *) const
    {
        if (ops->sw != 0 || ops->sh != 0) { set_error("%s: ops->sw and ops->sh must be 0: every file's own size is used", kWho); return IPX_ERR_INVALID; }
        if (ops->glyphs || ops->n_glyphs) {
            set_error("%s: ops->glyphs must be NULL: a positioned glyph list is anchored for one frame size; pass a text per file", kWho);
            return IPX_ERR_INVALID;
        }
        return IPX_OK;
    }
    int parse(const ipx_bytes *files, int n, int *status) { info.resize(n); return png_parse_all(files, n, info, status); }
    std::pair<int, int> size(int i) const { return {info[i].w, info[i].h}; }
    int kind(int i) const { return info[i].kind; }
    int admit(const MixedCall &, int) const { return IPX_OK; }      // a file that has a plan is taken
    size_t decode_cost(int i) const { return align256((size_t)info[i].w * info[i].h * png_kind_bpp(info[i].kind)) + 1024; }
    // what an output costs a chunk: the frame itself and the encoder's scratch for it -- the filtered stream, a word of match scratch
    // per filtered byte, and the frame's region
    size_t out_cost(const OutShape &sh, int) const
    {
        const size_t filt = (size_t)sh.h * (1 + 4 * (size_t)sh.w);
        return align256(sh.bytes) + 5 * align256(filt) + align256(kPngSegBase + png_segs_bytes(sh.w, sh.h, 4) + kPngTailBytes);
    }
    void trace(int, const MixCut &) const {}

    // ONE png_decode_files call for every size and kind of the group
    int decode(const MixedCall &c, Lane &, hipStream_t s, const ipx_bytes *files, const int *idx, int m, Group &g)
    {
        g.at = png_layout_packed(std::vector<int>(idx, idx + m), [&](int i) { return png_frame_need(info[i]); });
        IPX_HIP(g.mem.get(&g.dfr, g.at.bytes));
        if (g.at.pal_slots) IPX_HIP(g.mem.get(&g.dpal, (size_t)1024 * g.at.pal_slots));
        return png_decode_files(c.ctx, s, files, g.at, info, g.dfr, g.dpal, c.status);
    }
    // the frames from file i, which sits in slot `slot` of the group's layout, on
    BatchSrc src(const Group &g, int i, int slot) const
    {
        const PngFileInfo &f = info[i];
        const int kb = png_kind_bpp(f.kind);
        return packed_src(src_of_png(f.kind), g.dfr + g.at.off[slot], f.w * kb, align256((size_t)f.w * f.h * kb),
                          g.at.pal_slot[slot] >= 0 ? g.dpal + (size_t)g.at.pal_slot[slot] * 1024 : nullptr);
    }
    int chunk_memory(const MixedCall &c, Lane &, AsyncFree &omem, const int *file, int n, Chunk &a) const
    {
        for (int k = 0; k < kOuts; k++)
            if (const size_t total = a.lay(c, file, n, k, 0)) IPX_HIP(omem.get(&a.base[k], total));
        return IPX_OK;
    }
    int encode_run(const MixedCall &, hipStream_t, const int *, int, int, const Chunk &, ResultOwner &) const { return IPX_OK; }
    // one mixed-size png.Encode per present output over every frame of the chunk
    int encode_chunk(const MixedCall &c, hipStream_t s, const int *file, int n, const Chunk &a, ResultOwner &res) const
    {
        for (int k = 0; k < kOuts; k++) {
            std::vector<ipx_rgba_frame> fr;
            std::vector<int> owner_of;
            for (int p = 0; p < n; p++) {
                if (!c.has(file[p], k)) continue;
                const OutShape sh = c.shape(file[p], k);
                fr.push_back(ipx_rgba_frame{a.at(k, p), sh.w, sh.h, sh.w * 4});
                owner_of.push_back(file[p]);
            }
            if (fr.empty()) continue;
            std::vector<size_t> offs(fr.size()), lens(fr.size());
            uint8_t *blob = nullptr;
            const int rc = png_encode_mixed_core(c.ctx, s, fr.data(), (int)fr.size(), &blob, offs.data(), lens.data());
            if (rc) return rc;
            res.add(blob);
            for (size_t j = 0; j < fr.size(); j++) c.publish(owner_of[j], k, blob + offs[j], lens[j]);
        }
        return IPX_OK;
    }
};
}  // namespace

extern "C" int ipx_run_png_png_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts,
                                     ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result) try
{
    IPX_ENTER(ctx);
    PngMixed cx;
    return mixed_leg(cx, ctx, ops, n, files, texts, resize_out, thumb_out, wm_out, status, result);
}
IPX_CATCH_STATUS

