// ipx_jpeg_legs.hip -- what JPEG supplies to the mixed-size JPEG-in, JPEG-out leg (ipx_run_jpeg_jpeg_mixed; the walk is mixed_leg in
// ipx_mixed_leg.h): the sampling class as the cut's kind, one decode pass per group (jpeg_mixed_decode in ipx_jpeg_dec_runtime.hip), a
// chunk's block out of the lane's scratch, one jpeg.Encode per chunk: jpeg_encode_sets where every output has one size, else
// jpeg_encode_mixed_core over every frame of the chunk.  The uniform leg is in ipx_jpeg_runtime.hip.
// DESIGN.md sections 4.6 and 7.
#include <vector>

#include "ipx_mixed_leg.h"

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
    size_t out_cost(const OutShape &sh) const { return align256(sh.bytes) + 2 * coef_bytes(sh); }
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
