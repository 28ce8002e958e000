// ipx_mixed_leg.h -- the walk the mixed-size legs share (ipx_run_png_png_mixed in ipx_png_legs.hip, ipx_run_jpeg_jpeg_mixed in
// ipx_jpeg_legs.hip, ipx_run_gif_gif_mixed in ipx_gif_dec.hip): the entry's checks, a plan per frame size from the context's cache, the cut (ipx_mixed_cut.h), then groups ->
// chunks -> runs with the operators and the texts of a run.  What is a codec's -- parse, costs, decode, a run's source, the chunk's
// memory, encode -- comes in as the struct mixed_leg is instantiated on; DESIGN.md section 7 lists it.  Not part of the ABI.
#pragma once

#include <map>
#include <utility>
#include <vector>

#include "ipx_decode_common.h"
#include "ipx_mixed_cut.h"

// the plans of one call, one per frame size; handed back on every way out
struct SizePlans {
    struct Held { ipx_plan *pl; int cached; };
    ipx_ctx *ctx;
    std::map<std::pair<int, int>, Held> held;
    explicit SizePlans(ipx_ctx *c) : ctx(c) {}
    SizePlans(const SizePlans &) = delete;
    ~SizePlans()
    {
        for (auto &kv : held)
            if (kv.second.pl) ipx_plan_release(ctx, kv.second.pl, kv.second.cached);
    }
};

// A plan per size: (*plan_of)[i] for every file whose status is IPX_OK, of its size size_of(i) = (w, h), with ops' operators.  Files of
// a size no plan can be made for get ipx_plan_create's status, alone, and a null plan.  Every distinct size of the call holds its plan
// until `plans` goes: at most one per file (65535), of which the context's cache keeps IPX_PLAN_CACHE_MAX (256) and the rest live and
// die with the call -- a call with more sizes than that also turns the cache over once.
template <class SizeOf>
inline int size_plans_acquire(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, SizeOf size_of, int *status, SizePlans &plans, std::vector<ipx_plan *> *plan_of)
{
    std::map<std::pair<int, int>, int> plan_rc;
    plan_of->assign(n, nullptr);
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        const std::pair<int, int> key = size_of(i);
        auto it = plan_rc.find(key);
        if (it == plan_rc.end()) {
            ipx_pool_ops o = *ops;
            o.sw = key.first;
            o.sh = key.second;
            SizePlans::Held hd{nullptr, 0};
            const int prc = ipx_plan_acquire(ctx, &o, &hd.pl, &hd.cached);
            // a size the operators cannot be planned for is that size's verdict; anything else (memory, the device) fails the call
            if (prc != IPX_OK && prc != IPX_ERR_INVALID && prc != IPX_ERR_UNSUPPORTED) return prc;
            if (prc == IPX_OK) plans.held[key] = hd;
            it = plan_rc.emplace(key, prc).first;
        }
        if (it->second != IPX_OK) { status[i] = it->second; continue; }
        (*plan_of)[i] = plans.held[key].pl;
    }
    return IPX_OK;
}

// what the steps of one call share: the caller's arrays and every file's plan
struct MixedCall {
    ipx_ctx *ctx;
    const char *who;
    const ipx_text *texts;
    ipx_bytes *dst[kOuts];                  // null: the output is not asked for
    int *status;
    std::vector<ipx_plan *> plan_of;        // null: the file is not OK
    OutShape shape(int i, int k) const { return out_shape(plan_of[i]->info, k); }
    // an output that is wanted and made for file i.  A plan's bytes are w * h * 4 of sizes that are never negative (ipx_plan_create), so
    // bytes != 0 says that neither w nor h is 0: one test serves every leg.
    bool has(int i, int k) const { return dst[k] && shape(i, k).bytes; }
    // how far apart the frames of file i's size lie in the chunk's memory for output k; 0: no such output
    size_t out_fs(int i, int k) const { return has(i, k) ? align256(shape(i, k).bytes) : 0; }
    // a stream goes to the caller only for a file that is still IPX_OK
    void publish(int i, int k, uint8_t *data, size_t len) const { if (status[i] == IPX_OK) dst[k][i] = ipx_bytes{data, len}; }
};

// where a chunk's output frames lie: file p's frame of output k at base[k] + off[k][p]
struct ChunkFrames {
    std::vector<size_t> off[kOuts];
    uint8_t *base[kOuts] = {nullptr, nullptr, nullptr};
    bool empty = false;                     // set by the codec's chunk_memory: nothing to write, the chunk is skipped
    uint8_t *at(int k, int p) const { return base[k] + off[k][p]; }
    // lays the frames of output k of the chunk's n files out from `from` on; -> where they end
    size_t lay(const MixedCall &c, const int *file, int n, int k, size_t from)
    {
        off[k].resize(n);
        for (int p = 0; p < n; p++) { off[k][p] = from; from += c.out_fs(file[p], k); }
        return from;
    }
};

// one run -- files [p0, p0 + n) of the chunk, of one size and kind, decoded at d: the operators into the run's slice of the chunk's
// memory, its texts in one launch from a set clipped to the run's size, then what the codec encodes per run
template <class Codec>
int mixed_run(Codec &cx, const MixedCall &c, hipStream_t s, const BatchSrc &d, const int *file, int p0, int n, const typename Codec::Chunk &b,
              AsyncFree *omem, ResultOwner &res)
{
    const int i0 = file[p0];
    const ipx_plan *pl = c.plan_of[i0];
    BatchDst bd;
    for (int k = 0; k < kOuts; k++)
        if (const size_t fs = c.out_fs(i0, k)) { bd.out[k] = b.at(k, p0); bd.frame_stride[k] = fs; }
    if (!Codec::kRunsWithoutOutputs && !bd.out[0] && !bd.out[1] && !bd.out[2]) return IPX_OK;
    int rc = run_dev_src(c.ctx, s, pl, n, d, bd);
    if (rc) return rc;
    if (c.texts && pl->p.do_watermark && bd.out[kOutWm]) {
        const OutShape sh = c.shape(i0, kOutWm);
        std::vector<ipx_text> own(n);
        for (int q = 0; q < n; q++) own[q] = c.texts[file[p0 + q]];
        ipx_textset ts;                             // (its memory goes back in stream order, behind the launch)
        if ((rc = textset_build(s, c.who, own.data(), n, sh.w, sh.h, &ts))) return rc;
        if ((rc = dev_composite_texts(s, omem, bd.out[kOutWm], sh.w * 4, bd.frame_stride[kOutWm], n, ts, 0, nullptr))) return rc;
    }
    return cx.encode_run(c, s, file, p0, n, b, res);
}

// The body of a mixed-size entry behind IPX_ENTER.  The order of the checks decides which error a bad call gets: the arguments, then the
// codec's own refusals (cx.refuse), then the texts; the wanted outputs are cleared before anything is parsed.  Then the parse, a plan per
// size, the codec's verdict on a file with its plan (cx.admit: a status for that file alone), the cut, and per group ONE decode whatever
// sizes and kinds it holds; per chunk the operators once per run into the chunk's
// memory and the codec's encode.  The host does not wait for the stream between runs beyond what those stages contain.
template <class Codec>
int mixed_leg(Codec &cx, ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts, ipx_bytes *resize_out,
              ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result)
{
    const char *who = Codec::kWho;
    if (!ops || n < 0 || !result || (n && (!files || !status))) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *result = nullptr;
    int rc = cx.refuse(ops, n, texts);
    if (rc) return rc;
    if (texts && (rc = texts_check(who, texts, n))) return rc;
    MixedCall c{ctx, who, texts, {resize_out, thumb_out, wm_out}, status, {}};
    for (int k = 0; k < kOuts; k++)
        if (c.dst[k])
            for (int i = 0; i < n; i++) c.dst[k][i] = ipx_bytes{nullptr, 0};
    if (n == 0) return IPX_OK;
    if ((rc = cx.parse(files, n, status))) return rc;
    // given up in reverse order: the plans go back last, behind everything declared below that ran through them
    SizePlans plans(ctx);
    if ((rc = size_plans_acquire(ctx, ops, n, [&](int i) { return cx.size(i); }, status, plans, &c.plan_of))) return rc;
    std::vector<MixItem> items(n, MixItem{false, 0, 0, 0, 0, 0});
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        if ((status[i] = cx.admit(c, i)) != IPX_OK) { c.plan_of[i] = nullptr; continue; }
        items[i] = MixItem{true, cx.size(i).first, cx.size(i).second, cx.kind(i), cx.decode_cost(i), 0};
        for (int k = 0; k < kOuts; k++)
            if (c.has(i, k)) items[i].chunk_bytes += cx.out_cost(c.shape(i, k), k);
    }
    const int group_max = std::min(65535, std::max(1, env_int(Codec::kGroupEnv, Codec::kGroupFiles)));
    const size_t chunk_bytes = (size_t)std::max(0, env_int(Codec::kChunkEnv, Codec::kChunkMB)) << 20;
    const MixCut cut = mixed_cut(items.data(), n, group_max, (size_t)4 << 30, chunk_bytes);
    cx.trace(n, cut);
    ResultOwner res(ctx);                   // (released on the success path only: a failing call frees what it had encoded)
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    for (const MixGroup &grp : cut.groups) {
        StreamSync sync{s};                 // before the group's memory: the stream is waited for after that memory is given back to it
        typename Codec::Group mem(ctx, s);  // what the group decodes into: it goes back, in stream order, with the group
        if ((rc = cx.decode(c, lane.get(), s, files, cut.order.data() + grp.first, grp.n, mem))) return rc;
        for (int ci = grp.chunk0; ci < grp.chunk0 + grp.nchunks; ci++) {
            const MixChunk &ch = cut.chunks[ci];
            const int *file = cut.order.data() + ch.first;          // the chunk's files, by the caller's index
            if (!std::any_of(file, file + ch.n, [&](int i) { return status[i] == IPX_OK; })) continue;
            AsyncFree omem{s, {}};
            typename Codec::Chunk b;
            if ((rc = cx.chunk_memory(c, lane.get(), omem, file, ch.n, b))) return rc;
            if (b.empty) continue;
            for (int r = ch.run0; r < ch.run0 + ch.nruns; r++) {
                const int p0 = cut.runs[r].first - ch.first, g0 = cut.runs[r].first - grp.first, rn = cut.runs[r].n;
                // (a run whose first file the decode left without a frame has nothing to start from: its other files run one by one)
                const bool whole = cx.decoded(file[p0]);
                for (int q = 0; q < (whole ? 1 : rn); q++)
                    if (cx.decoded(file[p0 + q]))
                        if ((rc = mixed_run(cx, c, s, cx.src(mem, file[p0 + q], g0 + q), file, p0 + q, whole ? rn : 1, b, &omem, res))) return rc;
            }
            if ((rc = cx.encode_chunk(c, s, file, ch.n, b, res))) return rc;
        }
    }
    *result = res.release();
    return IPX_OK;
}
