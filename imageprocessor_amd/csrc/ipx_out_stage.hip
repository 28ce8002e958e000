// ipx_out_stage.hip -- the output stage of the compressed-out batch legs (JPEG, PNG and GIF alike; declared in ipx_runtime_internal.h):
// the result that owns a call's pinned blocks, the plan's three outputs as such a leg hands them out, the chunk step every leg takes
// (run_chunk: operators, texts, one encode per codec, the streams published in the caller's arrays) and the leg of the entries that
// take frames in host memory on one lane (run_host_streams).  The encoders it calls: ipx_jpeg_runtime.hip, ipx_png.hip, ipx_gif.hip.
// DESIGN.md section 4.11.
#include <vector>

#include "ipx_png.h"
#include "ipx_runtime_internal.h"

extern "C" void ipx_jpeg_result_free(ipx_ctx *ctx, ipx_jpeg_result *r)
{
    if (!r) return;
    for (uint8_t *b : r->blobs) (void)ipx_host_free(ctx, b);
    delete r;
}

void ResultOwner::adopt(ipx_jpeg_result *o)
{
    if (!o) return;
    r_->blobs.insert(r_->blobs.end(), o->blobs.begin(), o->blobs.end());
    delete o;
}

PlanOutputs::PlanOutputs(const ipx_plan *pl, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, Codec res, Codec thumb, Codec wm)
{
    ipx_bytes *const dst[kOuts] = {resize_out, thumb_out, wm_out};
    const Codec codec[kOuts] = {res, thumb, wm};
    for (int k = 0; k < kOuts; k++) {
        const OutShape sh = out_shape(pl->info, k);
        o[k] = {dst[k], sh.w, sh.h, dst[k] ? align256(sh.bytes) : 0, 0, codec[k]};
    }
    for (Output &x : o)
        if (x.fs && x.codec == Codec::Jpeg) x.coef = align256(ipx_jpeg_coef_count(x.w, x.h) * 2);
}

PlanOutputs::Frames PlanOutputs::place(uint8_t *block, int chunk) const
{
    Frames f{};
    size_t at = 0;
    for (int k = 0; k < 3; k++) { f.dev[k] = o[k].fs ? block + at * chunk : nullptr; at += o[k].fs; }
    for (int k = 0; k < 3; k++) { f.coef[k] = o[k].coef ? (int16_t *)(block + at * chunk) : nullptr; at += o[k].coef; }
    return f;
}

void PlanOutputs::clear(int n) const
{
    for (const Output &x : o)
        if (x.dst)
            for (int i = 0; i < n; i++) x.dst[i] = ipx_bytes{nullptr, 0};
}

int PlanOutputs::check_gif() const
{
    for (const Output &x : o)
        if (x.codec == Codec::Gif && x.fs && (x.w >= 1 << 16 || x.h >= 1 << 16)) { set_error("gif: image is too large to encode"); return IPX_ERR_INVALID; }
    return IPX_OK;
}

// Encodes the sel.n frames of every present output and publishes {blob + off, len} of frame i into dst[sel.at(i)].  All JPEG outputs go
// into one jpeg_encode_sets call (three waits for the device in all); PNG and GIF outputs are encoded one after the other.
static int encode_outputs(ipx_ctx *ctx, hipStream_t s, const PlanOutputs &outs, const PlanOutputs::Frames &f, const FileSel &sel, int quality,
                   const int *status, ResultOwner &res)
{
    const int m = sel.n;
    std::vector<size_t> offs(3 * (size_t)m), lens(3 * (size_t)m);
    auto publish = [&](const PlanOutputs::Output &o, const uint8_t *blob, const size_t *off, const size_t *len) {
        for (int i = 0; i < m; i++) {
            const int j = sel.at(i);
            if (!status || status[j] == IPX_OK) o.dst[j] = ipx_bytes{blob + off[i], len[i]};
        }
    };
    JpegEncSet sets[3];
    int who[3], K = 0;
    for (int k = 0; k < 3; k++) {
        const PlanOutputs::Output &o = outs.o[k];
        if (!o.fs || o.w <= 0 || o.h <= 0) continue;
        if (o.codec == Codec::Jpeg) {
            sets[K] = JpegEncSet{f.coef[k], f.dev[k], o.w, o.h, o.w * 4, o.fs, offs.data() + (size_t)K * m, lens.data() + (size_t)K * m};
            who[K++] = k;
            continue;
        }
        uint8_t *blob = nullptr;
        const int rc = (o.codec == Codec::Png ? png_encode_core : gif_encode_core)(ctx, s, f.dev[k], o.w, o.h, o.w * 4, o.fs, m, &blob,
                                                                                   offs.data(), lens.data());
        if (rc) return rc;
        res.add(blob);
        publish(o, blob, offs.data(), lens.data());
    }
    if (K == 0) return IPX_OK;
    uint8_t *blob = nullptr;
    const int rc = jpeg_encode_sets(ctx, s, sets, K, m, quality, &blob);
    if (rc) return rc;
    res.add(blob);
    for (int k = 0; k < K; k++) publish(outs.o[who[k]], blob, sets[k].offs, sets[k].lens);
    return IPX_OK;
}

int LegTexts::build(hipStream_t s, const char *who, const ipx_plan *pl, const PlanOutputs &outs, const ipx_text *texts, const FileSel &sel, bool slots)
{
    draw = texts && pl->p.do_watermark && outs.o[2].fs;
    by_slot = slots;
    if (!draw) return IPX_OK;
    std::vector<ipx_text> own(sel.idx ? sel.n : 0);           // (textset_build returns with its uploads finished)
    for (size_t g = 0; g < own.size(); g++) own[g] = texts[sel.idx[g]];
    return textset_build(s, who, sel.idx ? own.data() : texts + sel.first, sel.n, outs.o[2].w, outs.o[2].h, &ts);
}

int run_chunk(ipx_ctx *ctx, hipStream_t s, const ipx_plan *pl, const PlanOutputs &outs, uint8_t *block, int slots, const BatchSrc &d,
              const FileSel &sel, int c0, int m, const LegTexts *texts, AsyncFree *mem, int quality, const int *status, ResultOwner &res)
{
    const PlanOutputs::Frames f = outs.place(block, slots);
    const FileSel here = sel.slice(c0, m);
    int rc = run_dev_src(ctx, s, pl, m, d, outs.dst(f));
    if (!rc && texts && texts->draw) {
        const bool map = !texts->by_slot && here.idx;
        rc = dev_composite_texts(s, mem, f.dev[2], outs.o[2].w * 4, outs.o[2].fs, m, texts->ts, map ? 0 : texts->by_slot ? c0 : here.first,
                                 map ? here.idx : nullptr);
    }
    if (!rc) rc = encode_outputs(ctx, s, outs, f, here, quality, status, res);
    return rc;
}

int run_host_streams(const char *who, ipx_ctx *ctx, const ipx_plan *pl, int n, const BatchSrc &host, Codec res_codec, Codec thumb_codec,
                     Codec wm_codec, const char *chunk_env, int chunk_default, int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out,
                     ipx_bytes *wm_out, ipx_jpeg_result **result)
{
    if (!result) { set_error("%s: bad argument", who); return IPX_ERR_INVALID; }
    *result = nullptr;
    int rc0 = src_check(who, pl, host, n, false);
    if (rc0) return rc0;
    const PlanOutputs outs(pl, resize_out, thumb_out, wm_out, res_codec, thumb_codec, wm_codec);
    rc0 = outs.check_gif();                       // every frame handed to gif.Encode must fit its limits: checked before anything runs
    if (rc0) return rc0;
    if (n == 0) return IPX_OK;
    const SrcLayout L = src_layout(pl, host);
    const size_t per_frame = L.frame_bytes() + outs.frame_bytes();
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)env_int(chunk_env, chunk_default), ((size_t)1 << 30) / per_frame}));
    ResultOwner res(ctx);                         // the blocks of finished chunks go back to the cache on every way out but success
    LaneLease lane(ctx);
    hipStream_t s = lane->stream;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        StreamSync sync{s};
        AsyncFree mem{s, {}};
        uint8_t *dsrc, *dout = nullptr;
        IPX_HIP(mem.get(&dsrc, L.frame_bytes() * m));        // [m x plane 0][m x palette, for paletted frames]
        if (outs.frame_bytes()) IPX_HIP(mem.get(&dout, outs.frame_bytes() * m));
        BatchSrc d;
        IPX_HIP(src_upload(host, L, i0, m, dsrc, m, s, kCopyFrameRows, &d));
        const int rc = run_chunk(ctx, s, pl, outs, dout, m, d, all_files(n), i0, m, nullptr, nullptr, quality, nullptr, res);
        if (rc) return rc;
    }
    *result = res.release();
    return IPX_OK;
}
