// ipx_jpeg_runtime.hip -- jpeg.Encode on the GPU, the part that touches the device: the two encode cores (jpeg_encode_sets for up to three
// sets of equally sized frames, jpeg_encode_mixed_core for frames of any sizes) and the ABI entries built on them.  Kernels: ipx_jpeg.hip,
// ipx_jpeg_entropy.hip; tables and the host's entropy coder: ipx_jpeg_host.cpp; the mixed core's records: ipx_jpeg_enc_mixed_plan.h.  The
// legs that chain the cores with the operators: ipx_out_stage.hip, ipx_jpeg_legs.hip.  DESIGN.md sections 4.5 and 4.6.
#include <atomic>
#include <chrono>

#include "ipx_runtime_internal.h"
#include "ipx_threads.h"

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

extern "C" int ipx_dev_jpeg_fdct_rgba8(ipx_ctx *ctx, void *stream, const uint8_t *src, int w, int h, int stride, size_t frame_stride,
                                       int n, int quality, int16_t *coefs) try
{
    IPX_ENTER(ctx);
    return fdct_rgba8(ctx, stream ? (hipStream_t)stream : ctx->stream, src, w, h, stride, frame_stride, n, quality, coefs, nullptr, nullptr, nullptr);
}
IPX_CATCH_STATUS

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
    for (int i = 0; i < n; i++) { offs[i] = total; lens[i] = streams[i].size(); total += align16(lens[i]); }
    uint8_t *b = (uint8_t *)ipx_host_alloc(ctx, total ? total : 1);
    if (!b) return IPX_ERR_NOMEM;
    for (int i = 0; i < n; i++) memcpy(b + offs[i], streams[i].data(), lens[i]);
    *blob = b;
    return IPX_OK;
}

// What both cores make of the quality before their first launch: the quantisation tables, and the four Huffman tables as the kernels
// read them, in stream-ordered scratch.  Declare it BEFORE the core's StreamSync: the queued upload reads `packed`.
struct JpegEncTables {
    JpegTables t;
    uint32_t packed[1024];
    uint32_t *d_tab = nullptr;
    explicit JpegEncTables(int quality) { jpeg_tables(quality, &t); jpeg_huff_packed(packed); }
    hipError_t upload(AsyncFree &mem, hipStream_t s)
    {
        const hipError_t e = mem.get(&d_tab, sizeof packed);
        return e != hipSuccess ? e : hipMemcpyAsync(d_tab, packed, sizeof packed, hipMemcpyHostToDevice, s);
    }
};

// jpeg.Encode of up to three sets of n frames (the three operators' outputs of one batch) with THREE waits for the device in all: every
// set's transform + symbol sizing, one read-back of the sizes; every set's bit packing + 0xff count, one read-back; every set's byte
// stuffing into one block, one download.  (One set after the other, as rounds 1 and 2 ran it, is nine waits: 5.5 ms for a batch of 8.)
int jpeg_encode_sets(ipx_ctx *ctx, hipStream_t s, const JpegEncSet *sets, int K, int n, int quality, uint8_t **blob)
{
    *blob = nullptr;
    if (K <= 0 || K > 3 || n <= 0) return IPX_OK;
    const bool trace = env_int("IPX_DEBUG_J2J", 0) != 0;
    const auto te0 = std::chrono::steady_clock::now();
    auto ms_at = [&](std::chrono::steady_clock::time_point at) { return std::chrono::duration<double, std::milli>(at - te0).count(); };
    auto ems = [&] { return ms_at(std::chrono::steady_clock::now()); };
    double t_q1 = 0, t_s1 = 0, t_q2 = 0, t_s2 = 0;

    // ---- entropy coding on the GPU: size, scan, place, stuff (ipx_jpeg_entropy.hip) ----
    JpegEncTables tab(quality);
    const JpegTables &t = tab.t;
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
    IPX_HIP(tab.upload(mem, s));
    uint32_t *const d_tab = tab.d_tab;
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
    {
        const unsigned long long limit = jpeg_scan_limit(env_int("IPX_JPEG_MAX_SCAN_BITS", 0));
        const long long j = jpeg_scan_too_long(tot.data(), tot.size(), limit);
        if (j >= 0) {
            set_error("jpeg: scan too long for the GPU entropy coder (%llu bits in frame %d of output %d; the limit is %llu)", tot[(size_t)j],
                      (int)(j % n), (int)(j / n), limit);
            return IPX_ERR_UNSUPPORTED;            // (AsyncFree and StreamSync release and wait on the way out)
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
            ototal += align16(sets[k].lens[i]);
        }
    IPX_HIP(mem.get(&d_ostream, (size_t)ototal));
    for (int k = 0; k < K; k++) {
        Dev &d = dv[k];
        IPX_HIP(hipMemcpyAsync(d.d_obase, obase.data() + (size_t)k * n, (size_t)n * 8, hipMemcpyHostToDevice, s));
        IPX_HIP(launch_jpeg_stuff(d_ustream, d.d_ubase, d.d_ubytes, d.max_chunks, n, d.d_ff, d.d_hdr, (int)d.hdr.size(), d.d_obase, d_ostream, s));
    }
    auto queued = te0;
    const int rc = download_streams(ctx, s, d_ostream, (size_t)ototal, "", blob, &queued);   // (ubase / obase are read by the queued copies until here)
    if (trace && rc != IPX_ERR_NOMEM)
        fprintf(stderr, "[ipx] encode of %d sets x %d frames: sized (queued %.2f ms, done %.2f), packed (queued %.2f, done %.2f), streams of %.1f MB queued %.2f, down at %.2f\n",
                K, n, t_q1, t_s1, t_q2, t_s2, (double)ototal / 1e6, ms_at(queued), ems());
    return rc;
}

extern "C" int ipx_jpeg_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
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
    int16_t *dcoefs = (int16_t *)lane->dev;       // n * ipx_jpeg_coef_count int16 of scratch
    if (env_int("IPX_JPEG_HOST_ENTROPY", 0)) {
        rc = ipx_dev_jpeg_fdct_rgba8(ctx, lane->stream, src, w, h, stride, frame_stride, n, quality, dcoefs);
        if (rc) return rc;
        return jpeg_batch_host_entropy(ctx, lane.get(), dcoefs, w, h, n, quality, blob, offs, lens);
    }
    const JpegEncSet one{dcoefs, src, w, h, stride, frame_stride, offs, lens};
    return jpeg_encode_sets(ctx, lane->stream, &one, 1, n, quality, blob);
}
IPX_CATCH_STATUS

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
    JpegEncTables tab(quality);
    const JpegTables &t = tab.t;
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
    uint32_t *d_len, *d_fftot;
    int16_t *d_dcq;
    uint8_t *d_hdr;
    JpegEncFrame *d_recs;
    unsigned long long *d_bits;
    IPX_HIP(tab.upload(mem, s));
    uint32_t *const d_tab = tab.d_tab;
    IPX_HIP(mem.get(&d_hdr, hdr.size()));
    IPX_HIP(mem.get(&d_recs, rec_bytes));
    IPX_HIP(mem.get(&d_bits, (size_t)n * 8));
    IPX_HIP(mem.get(&d_fftot, (size_t)n * 4));
    IPX_HIP(mem.get(&d_len, nblk * 4));
    IPX_HIP(mem.get(&d_dcq, nblk * 2));
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
        const unsigned long long limit = jpeg_scan_limit(env_int("IPX_JPEG_MAX_SCAN_BITS", 0));
        const long long i = jpeg_scan_too_long(bits.data(), bits.size(), limit);
        if (i >= 0) {
            set_error("jpeg: scan too long for the GPU entropy coder (%llu bits in frame %d, %dx%d; the limit is %llu)", bits[(size_t)i], (int)i,
                      frames[i].w, frames[i].h, limit);
            return IPX_ERR_UNSUPPORTED;            // (AsyncFree and StreamSync release and wait on the way out)
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
    return download_streams(ctx, s, d_ostream, ototal, "", blob);   // (the records are read by the queued copy until here)
}

extern "C" {

int ipx_jpeg_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, int quality, uint8_t **blob, size_t *offs, size_t *lens) try
{
    IPX_ENTER(ctx);
    const auto encodable = [](const char *who, int f, const ipx_rgba_frame &fr) -> int {
        if (fr.w < 1 << 16 && fr.h < 1 << 16) return IPX_OK;
        set_error("%s: frame %d: jpeg: image is too large to encode", who, f);
        return IPX_ERR_INVALID;
    };
    int rc = rgba_frames_check("ipx_jpeg_encode_mixed_dev", frames, n, blob, offs, lens, encodable, true);
    if (rc || n == 0) return rc;
    size_t coef_bytes = 0;
    for (int f = 0; f < n; f++) coef_bytes += align256(ipx_jpeg_coef_count(frames[f].w, frames[f].h) * sizeof(int16_t));
    LaneLease lane(ctx);
    rc = lane_reserve(lane.get(), coef_bytes + 256);
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
