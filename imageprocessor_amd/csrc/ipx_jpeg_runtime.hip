// ipx_jpeg_runtime.hip -- the ABI entries of the codec legs: jpeg.Encode on the GPU, and the legs that chain it with the operators
// (host frames -> streams, planes -> streams, files -> streams; image.Decode for JPEG: ipx_jpeg_dec_runtime.hip).  Kernels: ipx_jpeg.hip,
// ipx_jpeg_entropy.hip; host half: ipx_jpeg_host.cpp.
#include <atomic>
#include <chrono>
#include <optional>
#include <string>

#include "ipx_png.h"
#include "ipx_decode_common.h"

// ---- jpeg.Encode: the entries that touch the device (tables / entropy coder: ipx_jpeg_host.cpp) ----------

extern "C" {

static int fdct_rgba8(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, int quality,
                      int16_t *coefs, const uint32_t *huff, uint32_t *aclen, int16_t *dcq);

int ipx_dev_jpeg_fdct_rgba8(ipx_ctx *ctx, void *stream, const uint8_t *src, int w, int h, int stride, size_t frame_stride,
                            int n, int quality, int16_t *coefs) try
{
    IPX_ENTER(ctx);
    return fdct_rgba8(ctx, stream ? (hipStream_t)stream : ctx->stream, src, w, h, stride, frame_stride, n, quality, coefs, nullptr, nullptr, nullptr);
}
IPX_CATCH_STATUS

}  // extern "C"

// huff / aclen / dcq: all or none -- the transform kernel then also sizes every block's AC symbols and leaves the DC terms in a dense array
static int fdct_rgba8(ipx_ctx *ctx, hipStream_t s, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, int quality,
                      int16_t *coefs, const uint32_t *huff, uint32_t *aclen, int16_t *dcq)
{
    (void)ctx;
    if (!src || !coefs || n < 0 || w <= 0 || h <= 0 || (long long)stride < (long long)w * 4) {
        set_error("ipx_dev_jpeg_fdct_rgba8: bad argument");
        return IPX_ERR_INVALID;
    }
    if (w >= 1 << 16 || h >= 1 << 16) { set_error("jpeg: image is too large to encode"); return IPX_ERR_INVALID; }
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_dev_jpeg_fdct_rgba8: at most 65535 frames per call"); return IPX_ERR_UNSUPPORTED; }
    JpegTables t;
    jpeg_tables(quality, &t);
    JpegArgs a;
    a.src = src; a.frame_stride = frame_stride; a.stride = stride; a.w = w; a.h = h;
    a.aligned16 = ((((uintptr_t)src) | (uintptr_t)stride | frame_stride) & 15) == 0;
    a.coefs = coefs; a.mcus_per_frame = ((w + 15) / 16) * ((h + 15) / 16);
    a.huff = huff; a.aclen = aclen; a.dcq = dcq;
    memcpy(a.recip, t.recip, sizeof a.recip);
    memcpy(a.div8, t.div8, sizeof a.div8);
    IPX_HIP(launch_jpeg_fdct(a, n, s));
    return IPX_OK;
}

// host entropy coding of a downloaded coefficient batch (IPX_JPEG_HOST_ENTROPY=1, and the reference point of tools/bench_jpeg.py)
static int jpeg_batch_host_entropy(ipx_ctx *ctx, Lane &lane, const int16_t *dcoefs, int w, int h, int n, int quality,
                                   uint8_t **blob, size_t *offs, size_t *lens)
{
    const size_t per = ipx_jpeg_coef_count(w, h) * sizeof(int16_t);
    hipStream_t s = lane.stream;
    int16_t *host = nullptr;
    IPX_HIP(hipHostMalloc((void **)&host, per * n, hipHostMallocDefault));
    hipError_t e = hipMemcpyAsync(host, dcoefs, per * n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipHostFree(host); set_error("coefficient download failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
    JpegTables t;
    jpeg_tables(quality, &t);
    std::vector<std::vector<uint8_t>> streams(n);
    std::atomic<int> failed{IPX_OK};
    HostPool::instance().parallel_for(n, 16, [&](int i) {
        const int rc = guarded_status([&] { jpeg_write_stream(host + (per / sizeof(int16_t)) * (size_t)i, w, h, t, &streams[i]); }, nullptr);
        if (rc) failed = rc;
    });
    (void)hipHostFree(host);
    if (failed) { set_error("entropy coding on the host failed (out of memory)"); return failed; }
    size_t total = 0;
    for (int i = 0; i < n; i++) { offs[i] = total; lens[i] = streams[i].size(); total += (lens[i] + 15) & ~(size_t)15; }
    uint8_t *b = (uint8_t *)ipx_host_alloc(ctx, total ? total : 1);
    if (!b) return IPX_ERR_NOMEM;
    for (int i = 0; i < n; i++) memcpy(b + offs[i], streams[i].data(), lens[i]);
    *blob = b;
    return IPX_OK;
}


extern "C" {

}  // extern "C"

// n frames in HBM -> streams in one pinned block, everything on stream s; dcoefs = n * ipx_jpeg_coef_count int16 of scratch
static int jpeg_encode_core(ipx_ctx *ctx, hipStream_t s, int16_t *dcoefs, const uint8_t *src, int w, int h, int stride, size_t frame_stride,
                            int n, int quality, uint8_t **blob, size_t *offs, size_t *lens);

extern "C" {

int ipx_jpeg_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                              int quality, uint8_t **blob, size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    if (!blob || !offs || !lens || n < 0) { set_error("ipx_jpeg_encode_batch_dev: bad argument"); return IPX_ERR_INVALID; }
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    const size_t per = ipx_jpeg_coef_count(w, h) * sizeof(int16_t);
    LaneLease lane(ctx);
    int rc = lane_reserve(lane.get(), per * n);
    if (rc) return rc;
    int16_t *dcoefs = (int16_t *)lane->dev;
    if (env_int("IPX_JPEG_HOST_ENTROPY", 0)) {
        rc = ipx_dev_jpeg_fdct_rgba8(ctx, lane->stream, src, w, h, stride, frame_stride, n, quality, dcoefs);
        if (rc) return rc;
        return jpeg_batch_host_entropy(ctx, lane.get(), dcoefs, w, h, n, quality, blob, offs, lens);
    }
    return jpeg_encode_core(ctx, lane->stream, dcoefs, src, w, h, stride, frame_stride, n, quality, blob, offs, lens);
}
IPX_CATCH_STATUS

}  // extern "C"

// jpeg.Encode of up to three sets of n frames (the three operators' outputs of one batch) with THREE waits for the device in all: every
// set's transform + symbol sizing, one read-back of the sizes; every set's bit packing + 0xff count, one read-back; every set's byte
// stuffing into one block, one download.  (One set after the other, as rounds 1 and 2 ran it, is nine waits: 5.5 ms for a batch of 8.)
int jpeg_encode_sets(ipx_ctx *ctx, hipStream_t s, const JpegEncSet *sets, int K, int n, int quality, uint8_t **blob)
{
    *blob = nullptr;
    if (K <= 0 || K > 3 || n <= 0) return IPX_OK;
    const bool trace = env_int("IPX_DEBUG_J2J", 0) != 0;
    const auto te0 = std::chrono::steady_clock::now();
    auto ems = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te0).count(); };
    double t_q1 = 0, t_s1 = 0, t_q2 = 0, t_s2 = 0, t_q3 = 0;

    // ---- entropy coding on the GPU: size, scan, place, stuff (ipx_jpeg_entropy.hip) ----
    JpegTables t;
    jpeg_tables(quality, &t);
    uint32_t packed[1024];
    jpeg_huff_packed(packed);
    struct Dev {
        int nblk = 0, max_chunks = 0;
        std::vector<uint8_t> hdr;
        uint32_t *d_len = nullptr, *d_ubytes = nullptr, *d_ff = nullptr;
        unsigned long long *d_ubase = nullptr, *d_obase = nullptr;
        uint8_t *d_hdr = nullptr;
    } dv[3];
    std::vector<uint32_t> ubytes((size_t)K * n), ff((size_t)K * n);
    std::vector<unsigned long long> tot((size_t)K * n), ubase((size_t)K * n), obase((size_t)K * n);
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    uint32_t *d_tab;
    IPX_HIP(mem.get(&d_tab, sizeof packed));
    IPX_HIP(hipMemcpyAsync(d_tab, packed, sizeof packed, hipMemcpyHostToDevice, s));
    unsigned long long *d_tot;                    // [K][n]: bits of every frame's scan, in 64 bits (the block offsets are 32-bit)
    uint32_t *d_fftot;                            // [K][n]
    IPX_HIP(mem.get(&d_tot, (size_t)K * n * 8));
    IPX_HIP(mem.get(&d_fftot, (size_t)K * n * 4));
    if (trace) fprintf(stderr, "[ipx]   tables queued at %.2f ms\n", ems());
    for (int k = 0; k < K; k++) {
        const JpegEncSet &o = sets[k];
        Dev &d = dv[k];
        d.nblk = (int)(ipx_jpeg_coef_count(o.w, o.h) * sizeof(int16_t) / 128);
        jpeg_write_header(o.w, o.h, t, &d.hdr);
        IPX_HIP(mem.get(&d.d_len, (size_t)n * d.nblk * 4));
        IPX_HIP(mem.get(&d.d_ubytes, (size_t)n * 4));
        IPX_HIP(mem.get(&d.d_ubase, (size_t)n * 8));
        IPX_HIP(mem.get(&d.d_obase, (size_t)n * 8));
        IPX_HIP(mem.get(&d.d_hdr, d.hdr.size()));
        IPX_HIP(hipMemcpyAsync(d.d_hdr, d.hdr.data(), d.hdr.size(), hipMemcpyHostToDevice, s));
        if (env_int("IPX_JPEG_FUSED_LEN", 1)) {
            // the transform kernel sizes the AC symbols of every block while it has the block in LDS; a small kernel adds the DC symbols
            int16_t *d_dcq;
            IPX_HIP(mem.get(&d_dcq, (size_t)n * d.nblk * 2));
            int rc = fdct_rgba8(ctx, s, o.src, o.w, o.h, o.stride, o.frame_stride, n, quality, o.dcoefs, d_tab, d.d_len, d_dcq);
            if (rc) return rc;
            IPX_HIP(launch_jpeg_dclen(d_dcq, d.nblk, n, d_tab, d.d_len, s));
        } else {
            int rc = fdct_rgba8(ctx, s, o.src, o.w, o.h, o.stride, o.frame_stride, n, quality, o.dcoefs, nullptr, nullptr, nullptr);
            if (rc) return rc;
            IPX_HIP(launch_jpeg_len(o.dcoefs, d.nblk, n, d_tab, d.d_len, s));     // the earlier separate pass over the coefficients
        }
        IPX_HIP(launch_scan64(d.d_len, d.nblk, n, d_tot + (size_t)k * n, s));
        if (trace) fprintf(stderr, "[ipx]   set %d (%dx%d) transform and sizes queued at %.2f ms\n", k, o.w, o.h, ems());
    }
    IPX_HIP(hipMemcpyAsync(tot.data(), d_tot, (size_t)K * n * 8, hipMemcpyDeviceToHost, s));
    t_q1 = ems();
    IPX_HIP(hipStreamSynchronize(s));
    t_s1 = ems();
    // The block offsets (d_len after the scan) and ubytes are 32-bit: a frame whose scan reaches 2^32 - 1 bits (some 200 M pixels of
    // binary noise at quality 100) would wrap them, and the bit packer would then write beyond d_ustream.  Refused here, before
    // anything reads the offsets or is sized from them; IPX_JPEG_MAX_SCAN_BITS can only lower the limit (for the tests).
    {
        const unsigned long long top = 0xffffffffull;
        const int knob = env_int("IPX_JPEG_MAX_SCAN_BITS", 0);
        const unsigned long long limit = knob > 0 ? std::min<unsigned long long>((unsigned long long)knob, top) : top;
        for (size_t j = 0; j < (size_t)K * n; j++)
            if (tot[j] >= limit) {
                set_error("jpeg: scan too long for the GPU entropy coder (%llu bits in frame %d of output %d; the limit is %llu)", tot[j],
                          (int)(j % n), (int)(j / n), limit);
                return IPX_ERR_UNSUPPORTED;        // (AsyncFree and StreamSync release and wait on the way out)
            }
    }
    unsigned long long utotal = 0;
    const int chunk = jpeg_chunk_bytes();
    size_t ff_words = 0;
    for (int k = 0; k < K; k++) {
        uint32_t umax = 0;
        for (int i = 0; i < n; i++) {
            const size_t j = (size_t)k * n + i;
            ubytes[j] = (uint32_t)((tot[j] + 7) / 8);
            ubase[j] = utotal;
            utotal += align256((size_t)ubytes[j] + 8);
            umax = std::max(umax, ubytes[j]);
        }
        dv[k].max_chunks = (int)((umax + chunk - 1) / chunk);
        ff_words += (size_t)n * dv[k].max_chunks;
    }
    uint8_t *d_ustream = nullptr, *d_ostream = nullptr;
    uint32_t *d_ffall = nullptr;
    IPX_HIP(mem.get(&d_ustream, (size_t)utotal));
    IPX_HIP(mem.get(&d_ffall, std::max<size_t>(ff_words, 1) * 4));
    IPX_HIP(hipMemsetAsync(d_ustream, 0, (size_t)utotal, s));
    {
        size_t at = 0;
        for (int k = 0; k < K; k++) {
            Dev &d = dv[k];
            d.d_ff = d_ffall + at;
            at += (size_t)n * d.max_chunks;
            IPX_HIP(hipMemcpyAsync(d.d_ubase, ubase.data() + (size_t)k * n, (size_t)n * 8, hipMemcpyHostToDevice, s));
            IPX_HIP(hipMemcpyAsync(d.d_ubytes, ubytes.data() + (size_t)k * n, (size_t)n * 4, hipMemcpyHostToDevice, s));
            IPX_HIP(launch_jpeg_bits(sets[k].dcoefs, d.nblk, n, d_tab, d.d_len, d_tot + (size_t)k * n, d.d_ubase, d_ustream, s));
            IPX_HIP(launch_jpeg_ffcount(d_ustream, d.d_ubase, d.d_ubytes, d.max_chunks, n, d.d_ff, s));
            IPX_HIP(launch_scan(d.d_ff, d.max_chunks, n, d_fftot + (size_t)k * n, s));
        }
    }
    IPX_HIP(hipMemcpyAsync(ff.data(), d_fftot, (size_t)K * n * 4, hipMemcpyDeviceToHost, s));
    t_q2 = ems();
    IPX_HIP(hipStreamSynchronize(s));
    t_s2 = ems();
    unsigned long long ototal = 0;
    for (int k = 0; k < K; k++)
        for (int i = 0; i < n; i++) {
            const size_t j = (size_t)k * n + i;
            sets[k].lens[i] = dv[k].hdr.size() + ubytes[j] + ff[j] + 2;
            obase[j] = ototal;
            sets[k].offs[i] = (size_t)ototal;
            ototal += (sets[k].lens[i] + 15) & ~(size_t)15;
        }
    IPX_HIP(mem.get(&d_ostream, (size_t)ototal));
    for (int k = 0; k < K; k++) {
        Dev &d = dv[k];
        IPX_HIP(hipMemcpyAsync(d.d_obase, obase.data() + (size_t)k * n, (size_t)n * 8, hipMemcpyHostToDevice, s));
        IPX_HIP(launch_jpeg_stuff(d_ustream, d.d_ubase, d.d_ubytes, d.max_chunks, n, d.d_ff, d.d_hdr, (int)d.hdr.size(), d.d_obase, d_ostream, s));
    }
    uint8_t *host = (uint8_t *)ipx_host_alloc(ctx, (size_t)ototal ? (size_t)ototal : 1);   // pinned: the download runs at link speed
    if (!host) return IPX_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(host, d_ostream, (size_t)ototal, hipMemcpyDeviceToHost, s);
    t_q3 = ems();
    { const hipError_t e2 = hipStreamSynchronize(s); if (e == hipSuccess) e = e2; }          // (ubase / obase are read by the queued copies until here)
    if (trace)
        fprintf(stderr, "[ipx] encode of %d sets x %d frames: sized (queued %.2f ms, done %.2f), packed (queued %.2f, done %.2f), streams of %.1f MB queued %.2f, down at %.2f\n",
                K, n, t_q1, t_s1, t_q2, t_s2, (double)ototal / 1e6, t_q3, ems());
    if (e != hipSuccess) { (void)ipx_host_free(ctx, host); set_error("stream download failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
    *blob = host;
    return IPX_OK;
}

static int jpeg_encode_core(ipx_ctx *ctx, hipStream_t s, int16_t *dcoefs, const uint8_t *src, int w, int h, int stride, size_t frame_stride,
                            int n, int quality, uint8_t **blob, size_t *offs, size_t *lens)
{
    const JpegEncSet one{dcoefs, src, w, h, stride, frame_stride, offs, lens};
    return jpeg_encode_sets(ctx, s, &one, 1, n, quality, blob);
}

// jpeg.Encode of n frames of ANY sizes with the same three waits for the device as jpeg_encode_sets -- sizes back, 0xff counts back,
// streams down -- for the whole list: every stage is one launch over all frames, which read their geometry, bases and first workgroups
// from a per-frame record in HBM (ipx_jpeg_enc_mixed_plan.h).  The records go up three times, each time with what the host has learnt
// since.  The same single pinned block, the same 16-byte-aligned stream starts; stream i is byte for byte what jpeg_encode_sets writes
// for frame i alone.  Scratch and grids are sums over the frames, not n x the largest.  A scan of 2^32 - 1 bits or more (lowered by
// IPX_JPEG_MAX_SCAN_BITS) refuses the call with IPX_ERR_UNSUPPORTED before anything reads the offsets, and names the frame.  It always
// sizes the blocks in the transform kernel: IPX_JPEG_FUSED_LEN and IPX_JPEG_HOST_ENTROPY do not apply to it.  Frames are taken as checked
// (ipx_jpeg_encode_mixed_dev checks them; the leg's come from plans).
int jpeg_encode_mixed_core(ipx_ctx *ctx, hipStream_t s, const JpegEncSrc *frames, int n, int quality, uint8_t **blob, size_t *offs, size_t *lens)
{
    *blob = nullptr;
    if (n <= 0) return IPX_OK;
    JpegTables t;
    jpeg_tables(quality, &t);
    uint32_t packed[1024];
    jpeg_huff_packed(packed);
    std::vector<uint8_t> hdr;
    jpeg_write_header(frames[0].w, frames[0].h, t, &hdr);     // one header for the call: a frame's differs in the SOF0 height and width alone
    if (hdr.size() < (size_t)kJpegSofDims + 4 || hdr[kJpegSofDims] != (uint8_t)(frames[0].h >> 8) || hdr[kJpegSofDims + 1] != (uint8_t)frames[0].h ||
        hdr[kJpegSofDims + 2] != (uint8_t)(frames[0].w >> 8) || hdr[kJpegSofDims + 3] != (uint8_t)frames[0].w) {
        set_error("jpeg: the header's SOF0 is not where the mixed-size encoder writes a frame's size");
        return IPX_ERR_INVALID;
    }
    std::vector<JpegEncFrame> recs;
    JpegEncTotals tot;
    if (!jpeg_enc_build(frames, n, &recs, &tot)) {
        set_error("jpeg: %d frames are more than one mixed-size encode takes (a grid of 2^31 - 1 workgroups)", n);
        return IPX_ERR_UNSUPPORTED;
    }
    std::vector<unsigned long long> bits((size_t)n);
    std::vector<uint32_t> ff((size_t)n);
    StreamSync sync{s};                           // after the host buffers above: the queued copies read and write them
    AsyncFree mem{s, {}};
    const size_t nblk = (size_t)tot.mcus * 6, rec_bytes = (size_t)n * sizeof(JpegEncFrame);
    uint32_t *d_tab, *d_len, *d_fftot;
    int16_t *d_dcq;
    uint8_t *d_hdr;
    JpegEncFrame *d_recs;
    unsigned long long *d_bits;
    IPX_HIP(mem.get(&d_tab, sizeof packed));
    IPX_HIP(mem.get(&d_hdr, hdr.size()));
    IPX_HIP(mem.get(&d_recs, rec_bytes));
    IPX_HIP(mem.get(&d_bits, (size_t)n * 8));
    IPX_HIP(mem.get(&d_fftot, (size_t)n * 4));
    IPX_HIP(mem.get(&d_len, nblk * 4));
    IPX_HIP(mem.get(&d_dcq, nblk * 2));
    IPX_HIP(hipMemcpyAsync(d_tab, packed, sizeof packed, hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, s));
    IPX_HIP(hipMemcpyAsync(d_recs, recs.data(), rec_bytes, hipMemcpyHostToDevice, s));
    // ---- transform and symbol sizing; the sizes come back ----
    JpegArgs a{};
    a.huff = d_tab; a.aclen = d_len; a.dcq = d_dcq;
    memcpy(a.recip, t.recip, sizeof a.recip);
    memcpy(a.div8, t.div8, sizeof a.div8);
    IPX_HIP(launch_jpeg_fdct_mixed(a, d_recs, n, tot.fdct_wgs, s));
    IPX_HIP(launch_jpeg_dclen_mixed(d_recs, n, tot.blk_wgs, d_dcq, d_tab, d_len, s));
    IPX_HIP(launch_scan_mixed_len(d_recs, n, d_len, d_bits, s));
    IPX_HIP(hipMemcpyAsync(bits.data(), d_bits, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    {
        const unsigned long long top = 0xffffffffull;
        const int knob = env_int("IPX_JPEG_MAX_SCAN_BITS", 0);
        const unsigned long long limit = knob > 0 ? std::min<unsigned long long>((unsigned long long)knob, top) : top;
        for (int i = 0; i < n; i++)
            if (bits[(size_t)i] >= limit) {
                set_error("jpeg: scan too long for the GPU entropy coder (%llu bits in frame %d, %dx%d; the limit is %llu)", bits[(size_t)i], i,
                          frames[i].w, frames[i].h, limit);
                return IPX_ERR_UNSUPPORTED;        // (AsyncFree and StreamSync release and wait on the way out)
            }
    }
    // ---- bit packing and the 0xff counts; the counts come back ----
    if (!jpeg_enc_place_scans(bits.data(), n, &recs, &tot)) {
        set_error("jpeg: %d frames are more than one mixed-size encode takes (a grid of 2^31 - 1 workgroups)", n);
        return IPX_ERR_UNSUPPORTED;
    }
    uint8_t *d_ustream, *d_ostream;
    uint32_t *d_ff;
    IPX_HIP(mem.get(&d_ustream, (size_t)tot.ubytes));
    IPX_HIP(mem.get(&d_ff, std::max<size_t>((size_t)tot.chunks, 1) * 4));
    IPX_HIP(hipMemsetAsync(d_ustream, 0, (size_t)tot.ubytes, s));
    IPX_HIP(hipMemcpyAsync(d_recs, recs.data(), rec_bytes, hipMemcpyHostToDevice, s));
    IPX_HIP(launch_jpeg_bits_mixed(d_recs, n, tot.blk_wgs, d_tab, d_len, d_bits, d_ustream, s));
    IPX_HIP(launch_jpeg_ffcount_mixed(d_recs, n, tot.chunk_wgs, d_ustream, d_ff, s));
    IPX_HIP(launch_scan_mixed_ff(d_recs, n, d_ff, d_fftot, s));
    IPX_HIP(hipMemcpyAsync(ff.data(), d_fftot, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    IPX_HIP(hipStreamSynchronize(s));
    // ---- byte stuffing into one block; the streams come down ----
    const size_t ototal = (size_t)jpeg_enc_place_streams(ff.data(), n, hdr.size(), &recs, offs, lens);
    IPX_HIP(mem.get(&d_ostream, ototal));
    IPX_HIP(hipMemcpyAsync(d_recs, recs.data(), rec_bytes, hipMemcpyHostToDevice, s));
    IPX_HIP(launch_jpeg_stuff_mixed(d_recs, n, tot.chunk_wgs, d_ustream, d_ff, d_hdr, (int)hdr.size(), d_ostream, s));
    uint8_t *host = (uint8_t *)ipx_host_alloc(ctx, ototal ? ototal : 1);   // pinned: the download runs at link speed
    if (!host) return IPX_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(host, d_ostream, ototal, hipMemcpyDeviceToHost, s);
    { const hipError_t e2 = hipStreamSynchronize(s); if (e == hipSuccess) e = e2; }          // (the records are read by the queued copy until here)
    if (e != hipSuccess) { (void)ipx_host_free(ctx, host); set_error("stream download failed: %s", hipGetErrorString(e)); return IPX_ERR_HIP; }
    *blob = host;
    return IPX_OK;
}

extern "C" {

int ipx_jpeg_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, int quality, uint8_t **blob, size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    if (!blob || !offs || !lens || n < 0 || (n && !frames)) { set_error("ipx_jpeg_encode_mixed_dev: bad argument"); return IPX_ERR_INVALID; }
    *blob = nullptr;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_jpeg_encode_mixed_dev: at most 65535 frames per call"); return IPX_ERR_UNSUPPORTED; }
    // every frame before any launch: a malformed one first (IPX_ERR_INVALID), then one beyond the span the kernels address
    for (int f = 0; f < n; f++) {
        const ipx_rgba_frame &fr = frames[f];
        if (!fr.pix || fr.w <= 0 || fr.h <= 0 || (long long)fr.stride < (long long)fr.w * 4) {
            set_error("ipx_jpeg_encode_mixed_dev: frame %d: bad argument", f);
            return IPX_ERR_INVALID;
        }
        if (fr.w >= 1 << 16 || fr.h >= 1 << 16) { set_error("ipx_jpeg_encode_mixed_dev: frame %d: jpeg: image is too large to encode", f); return IPX_ERR_INVALID; }
    }
    size_t coef_bytes = 0;
    for (int f = 0; f < n; f++) {
        if (!frame_span_ok(frames[f].w, frames[f].h, frames[f].stride, 4)) {
            set_error("ipx_jpeg_encode_mixed_dev: frame %d: %dx%d is beyond the frames the encoder addresses", f, frames[f].w, frames[f].h);
            return IPX_ERR_UNSUPPORTED;
        }
        coef_bytes += align256(ipx_jpeg_coef_count(frames[f].w, frames[f].h) * sizeof(int16_t));
    }
    LaneLease lane(ctx);
    const int rc = lane_reserve(lane.get(), coef_bytes + 256);
    if (rc) return rc;
    std::vector<JpegEncSrc> src((size_t)n);
    uint8_t *at = (uint8_t *)(((uintptr_t)lane->dev + 255) & ~(uintptr_t)255);
    for (int f = 0; f < n; f++) {
        src[(size_t)f] = JpegEncSrc{frames[f].pix, (int16_t *)at, frames[f].w, frames[f].h, frames[f].stride};
        at += align256(ipx_jpeg_coef_count(frames[f].w, frames[f].h) * sizeof(int16_t));
    }
    return jpeg_encode_mixed_core(ctx, lane->stream, src.data(), n, quality, blob, offs, lens);
}
IPX_CATCH_STATUS

}  // extern "C"

// ---- host frames in, JPEG streams out: the worker's whole GPU leg ----------------------------------------

extern "C" {

void ipx_jpeg_result_free(ipx_ctx *ctx, ipx_jpeg_result *r)
{
    if (!r) return;
    for (uint8_t *b : r->blobs) (void)ipx_host_free(ctx, b);
    delete r;
}

}  // extern "C"

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

int ipx_jpeg_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, int quality, uint8_t **out, size_t *len) try
{
    IPX_ENTER(ctx);
    if (!pix || !out || !len || w <= 0 || h <= 0 || (long long)stride < (long long)w * 4) {
        set_error("ipx_jpeg_encode_rgba8: bad argument");
        return IPX_ERR_INVALID;
    }
    if (w >= 1 << 16 || h >= 1 << 16) { set_error("jpeg: image is too large to encode"); return IPX_ERR_INVALID; }
    const size_t fbytes = align256((size_t)w * h * 4), per = ipx_jpeg_coef_count(w, h) * sizeof(int16_t);
    std::vector<int16_t> host(per / sizeof(int16_t));
    {
        LaneLease lane(ctx);
        int rc = lane_reserve(lane.get(), fbytes + per);
        if (rc) return rc;
        hipStream_t s = lane->stream;
        IPX_HIP(hipMemcpy2DAsync(lane->dev, (size_t)w * 4, pix, stride, (size_t)w * 4, h, hipMemcpyHostToDevice, s));
        rc = ipx_dev_jpeg_fdct_rgba8(ctx, s, lane->dev, w, h, w * 4, fbytes, 1, quality, (int16_t *)(lane->dev + fbytes));
        if (rc) { (void)hipStreamSynchronize(s); return rc; }
        IPX_HIP(hipMemcpyAsync(host.data(), lane->dev + fbytes, per, hipMemcpyDeviceToHost, s));
        IPX_HIP(hipStreamSynchronize(s));
    }
    return ipx_jpeg_entropy_encode(host.data(), w, h, quality, out, len);
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
