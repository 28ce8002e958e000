// ipx_jpeg_dec_runtime.hip -- the driver of image.Decode for JPEG batches: the host plan (ipx_jpeg_dec_host.cpp), then the device
// blocks, the upload, the scan walk of progressive files (opt-in), the Huffman passes and the reconstruction as stages of
// jpeg_decode_files.  Kernels: ipx_jpeg_dec.hip, ipx_jpeg_dec_par.hip, ipx_jpeg_dec_scans.hip; the host scan decoder of progressive
// files, and the marker pre-pass of the GPU scan walk: ipx_jpeg_dec_prog.cpp.
#include <chrono>

#include "ipx_decode_common.h"

namespace {

// the one conversion of a HIP result of the driver into a status
int hip_status(hipError_t e, const char *what)
{
    if (e != hipSuccess) set_error("%s: %s", what, hipGetErrorString(e));
    return e == hipSuccess ? IPX_OK : IPX_ERR_HIP;
}
#define DEC_HIP(what, call) do { const int rc_ = hip_status((call), what); if (rc_) return rc_; } while (0)

struct Events { hipEvent_t ev[2] = {nullptr, nullptr}; ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); } };   // of the two pinned halves

// What the stages of one call share.  The members go in reverse order: the wait for the stream first, then the pinned blocks, the
// scratch, and only then the host vectors that copies queued on the stream read (the plan) or write (dev_status).
struct DecRun {
    ipx_ctx *ctx; hipStream_t s; const ipx_bytes *jpegs; int n; int *status;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double t_alloc = 0, t_pin = 0, t_pack = 0, t_launch = 0;
    JpegBatchPlan plan;
    bool s411 = false;                 // IPX_JPEG_411=1 as this call read it
    // A mixed-size call: the run is one sampling class, of any sizes.  geom holds a record per file (ipx_jpeg_mixed_plan.h; a file
    // that is not decodable counts as 1 x 1), tot their sums; the launch arguments mxx, myy, nblk, w, h and the strides stay 0.
    bool mixed = false;
    std::vector<JpegMixGeom> geom;
    JpegMixTotals tot;
    JpegMixGeom *d_geom = nullptr;
    size_t blocks = 0;                 // of all images: n * nblk, or the sum over the records
    int max_nsub = 0;
    size_t plane_bytes = 0, scratch_bytes = 0;   // of this run: the planes; the estimate of everything else in HBM (the timing line)
    size_t blk0(int i) const { return mixed ? (size_t)geom[i].blk0 : (size_t)i * a.nblk; }
    size_t nblk(int i) const { return mixed ? (size_t)geom[i].nblk : (size_t)a.nblk; }
    std::vector<int> dev_status;
    std::vector<uint8_t> prog_block;   // the scan programs of the GPU-walked files as uploaded (dec_scans)
    JpegDecArgs a{};
    JpegPlanes pl{};
    uint8_t *d_blob = nullptr, *d_valid = nullptr; JpegDecImage *d_img = nullptr; JpegDecTables *d_tab = nullptr;
    AsyncFree mem;                     // scratch of this call: stream-ordered, or bumped out of the lane's decode buffer
    PinnedBlocks pinned;
    StreamSync sync;
    DecRun(ipx_ctx *c, hipStream_t st, const ipx_bytes *f, int n_, int *status_)
        : ctx(c), s(st), jpegs(f), n(n_), status(status_), mem{st, {}}, pinned(c, st), sync{st} {}
    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Stage 2: the batch's geometry, the planes and the scratch.  lane != NULL: everything is bumped out of the lane's decode buffer, grown
// once to an estimate of the whole call.
int dec_blocks(DecRun &r, Lane *lane, bool planes_in_lane, OwnedBlocks<ipx_jpeg_planes> &own)
{
    const JpegBatchPlan &P = r.plan;
    const JpegDecInfo &R = P.info[P.ref];
    const int n = r.n;
    JpegDecArgs &a = r.a;
    JpegPlanes &pl = r.pl;
    a.n = n; a.h0 = R.h0; a.v0 = R.v0;
    const bool gray = R.ncomp == 1;                        // *image.Gray: one block per MCU, no chroma planes
    a.ybl = R.h0 * R.v0; a.bpm = gray ? 1 : a.ybl + 2;
    a.nitems = (int)P.items.size();
    size_t ybytes, cbytes;                                 // the Y block; each chroma block
    if (r.mixed) {
        std::vector<int> ws(n), hs(n);
        for (int i = 0; i < n; i++) { const bool ok = r.status[i] == IPX_OK; ws[i] = ok ? P.info[i].w : 1; hs[i] = ok ? P.info[i].h : 1; }
        if (!jpeg_mix_build(JpegMixClass{R.h0, R.v0, gray ? 1 : 0}, ws.data(), hs.data(), n, &r.geom, &r.tot)) {
            set_error("jpeg decode: the files of one sampling class are too large for one decode pass");
            return IPX_ERR_UNSUPPORTED;
        }
        r.blocks = (size_t)r.tot.blocks; a.mix_wgs = (unsigned)r.tot.wgs;
        ybytes = (size_t)r.tot.ybytes; cbytes = (size_t)r.tot.cbytes;
    } else {
        a.w = R.w; a.h = R.h;
        a.mxx = (R.w + 8 * R.h0 - 1) / (8 * R.h0); a.myy = (R.h + 8 * R.v0 - 1) / (8 * R.v0);
        a.nblk = a.mxx * a.myy * a.bpm;
        pl.ystride = 8 * R.h0 * a.mxx; pl.cstride = 8 * a.mxx;
        pl.y_fs = align256((size_t)pl.ystride * 8 * R.v0 * a.myy); pl.c_fs = gray ? 0 : align256((size_t)pl.cstride * 8 * a.myy);
        r.blocks = (size_t)n * a.nblk;
        ybytes = pl.y_fs * n; cbytes = pl.c_fs * n;
    }
    r.plane_bytes = ybytes + 2 * cbytes;
    {
        size_t subs = 0;
        for (auto &pi : P.par) subs = std::max(subs, (size_t)pi.nsub);
        subs *= P.par.size();
        size_t prog_bytes = 0;                   // the scan programs as dec_scans uploads them
        for (int i : P.gfiles) prog_bytes += sizeof(JpegProgFile) + P.prog[i].scans.size() * sizeof(JpegProgScan) + P.prog[i].defs.size() * sizeof(JpegProgHuff) + 64;
        r.scratch_bytes = r.blocks * 130 + 3 * (P.blob_bytes + 1024) + P.piece_ubytes +
                           P.items.size() * (sizeof(JpegDecImage) + 8) + (size_t)n * (sizeof(JpegDecTables) + sizeof(JpegMixGeom) + 64) + P.par.size() * (sizeof(JpegParImage) + 64) +
                           subs * (32 + 12 * (size_t)jpeg_par_checkpoints()) + ((size_t)4 << 20) + prog_bytes;   // (par_setup: images x max_nsub entries)
    }
    if (lane) {
        const int rr = lane_reserve_dec(*lane, r.plane_bytes + r.scratch_bytes);
        if (rr) return rr;
        r.mem.arena = lane->dec; r.mem.cap = lane->dec_bytes;
    }
    auto plane = [&](uint8_t **p, size_t bytes) {
        if (lane && planes_in_lane) return r.mem.get(p, bytes);   // first requests of the call and counted in est: they always fit
        return own.alloc(p, bytes);
    };
    DEC_HIP("plane allocation", plane(&pl.y, ybytes));
    if (!gray) DEC_HIP("plane allocation", plane(&pl.cb, cbytes));
    if (!gray) DEC_HIP("plane allocation", plane(&pl.cr, cbytes));
    DEC_HIP("scratch allocation", r.mem.get(&r.d_blob, P.blob_bytes + 16));
    DEC_HIP("scratch allocation", r.mem.get(&r.d_img, sizeof(JpegDecImage) * P.items.size()));
    DEC_HIP("scratch allocation", r.mem.get(&r.d_valid, (size_t)n));
    DEC_HIP("scratch allocation", r.mem.get(&r.d_tab, sizeof(JpegDecTables) * n));
    DEC_HIP("scratch allocation", r.mem.get(&a.coefs, r.blocks * 128));
    DEC_HIP("scratch allocation", r.mem.get(&a.status, sizeof(int) * n));
    DEC_HIP("scratch allocation", r.mem.get(&a.dcs, r.blocks * 2 + 16));
    if (r.mixed) { DEC_HIP("scratch allocation", r.mem.get(&r.d_geom, sizeof(JpegMixGeom) * n)); a.geom = r.d_geom; }
    a.blob = r.d_blob; a.img = r.d_img; a.tab = r.d_tab; pl.valid = r.d_valid;
    r.t_alloc = r.ms();
    return IPX_OK;
}

// Stage 3: the blob, the items and the memsets; then the host-decoded files of the batch (progressive, several scans) group by group:
// their scans are walked on the pool's threads, in groups of IPX_JPEG_HOST_GROUP files, into one half of a pinned block of two groups,
// and the coefficients are copied into their slots (after the memsets, same stream) while the next group decodes into the other half.
// (One block for all of them was 6.3 MB per 1080p file, 1.6 GB for a part of 256 progressive files, per part and per feeder of a pool;
// uploading from pageable vectors took a quarter of such a call.)
int dec_upload(DecRun &r)
{
    JpegBatchPlan &P = r.plan;
    const JpegDecArgs &a = r.a;
    const int n = r.n;
    hipStream_t s = r.s;
    static const char *const kPrep = "jpeg decode: host preparation failed";
    uint8_t *hblob = r.pinned.get(P.blob_bytes + 16);
    if (!hblob) return IPX_ERR_NOMEM;
    const int group = std::max(1, env_int("IPX_JPEG_HOST_GROUP", 16));
    std::vector<int> hfiles;
    for (int i = 0; i < n; i++) if (P.hslot[i] >= 0) hfiles.push_back(i);
    // a host-decoded file's slot in its half of the pinned block: its coefficients (64 per block), then its DC values -- sized by the
    // file; a half holds the largest group (uniform batches: min(nhost, group) slots of one size)
    std::vector<size_t> hoff(hfiles.size());
    size_t half_words = 0;
    for (size_t g0 = 0; g0 < hfiles.size(); g0 += group) {
        size_t words = 0;
        for (size_t k = g0; k < std::min(hfiles.size(), g0 + group); k++) { hoff[k] = words; words += r.nblk(hfiles[k]) * 65; }
        half_words = std::max(half_words, words);
    }
    int16_t *hpin = nullptr;
    if (P.nhost) {
        hpin = (int16_t *)r.pinned.get((size_t)2 * half_words * sizeof(int16_t));
        if (!hpin) {   // no pinned memory for them: these files stay on the caller's CPU path, the rest of the batch goes on
            for (int i : hfiles) { r.status[i] = IPX_ERR_UNSUPPORTED; P.valid[i] = 0; }
            hfiles.clear();
            clear_error();
        }
    }
    r.t_pin = r.ms();
    // packing the scans walks every compressed byte
    int rc = parallel_light(n, [&](int i) {
        if (P.valid[i] && !P.info[i].host_scans) memcpy(hblob + P.blob_off[i], r.jpegs[i].data + P.info[i].scan_off, P.info[i].scan_len);
        if (P.valid[i] && P.info[i].gpu_scans) memcpy(hblob + P.blob_off[i], r.jpegs[i].data, r.jpegs[i].len);   // the whole file: its scans lie between its segments
    }, kPrep);
    if (rc) return rc;
    r.t_pack = r.ms();
    DEC_HIP("jpeg decode", hipMemcpyAsync(r.d_blob, hblob, P.blob_bytes, hipMemcpyHostToDevice, s));
    DEC_HIP("jpeg decode", hipMemcpyAsync(r.d_img, P.items.data(), sizeof(JpegDecImage) * P.items.size(), hipMemcpyHostToDevice, s));
    if (r.mixed) DEC_HIP("jpeg decode", hipMemcpyAsync(r.d_geom, r.geom.data(), sizeof(JpegMixGeom) * n, hipMemcpyHostToDevice, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(a.coefs, 0, r.blocks * 128, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(a.status, 0, sizeof(int) * n, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(a.dcs, 0, r.blocks * 2, s));
    Events ev;
    for (int g0 = 0, gi = 0; g0 < (int)hfiles.size(); g0 += group, gi++) {
        const int half = gi & 1, cnt = std::min(group, (int)hfiles.size() - g0);
        int16_t *base = hpin + (size_t)half * half_words;
        if (gi >= 2) DEC_HIP("jpeg decode", hipEventSynchronize(ev.ev[half]));          // the copies of two groups ago have left this half
        rc = parallel_heavy(cnt, [&](int j) {
            const int i = hfiles[g0 + j];
            bool prog = false;
            int alone = 0;
            JpegDecInfo full;
            int16_t *slot = base + hoff[g0 + j];
            const int st = jpeg_host_decode(r.jpegs[i].data, r.jpegs[i].len, &full, slot, slot + r.nblk(i) * 64, r.nblk(i), P.tabs[i].qnat, &prog, r.s411, &alone);
            if (st != IPX_OK) { r.status[i] = st; P.valid[i] = 0; }
            else P.valid[i] |= (uint8_t)(alone << 2);     // the blocks a non-interleaved sequential scan skips stay zero (jpeg_idct_kernel)
        }, kPrep);
        if (rc) return rc;
        for (int j = 0; j < cnt; j++) {
            const int i = hfiles[g0 + j];
            if (!P.valid[i]) continue;
            const int16_t *slot = base + hoff[g0 + j];
            DEC_HIP("jpeg decode", hipMemcpyAsync(a.coefs + r.blk0(i) * 64, slot, r.nblk(i) * 128, hipMemcpyHostToDevice, s));
            DEC_HIP("jpeg decode", hipMemcpyAsync(a.dcs + r.blk0(i), slot + r.nblk(i) * 64, r.nblk(i) * 2, hipMemcpyHostToDevice, s));
        }
        if (!ev.ev[half]) DEC_HIP("jpeg decode", hipEventCreateWithFlags(&ev.ev[half], hipEventDisableTiming));
        DEC_HIP("jpeg decode", hipEventRecord(ev.ev[half], s));
    }
    // (which files are decodable is final only now: a host-decoded file may have failed in its scans; and the host decoder fills the
    // quantisation tables of its files)
    DEC_HIP("jpeg decode", hipMemcpyAsync(r.d_valid, P.valid.data(), (size_t)n, hipMemcpyHostToDevice, s));
    DEC_HIP("jpeg decode", hipMemcpyAsync(r.d_tab, P.tabs.data(), sizeof(JpegDecTables) * n, hipMemcpyHostToDevice, s));
    return IPX_OK;
}

// Stage 3b: the progressive files whose scans the GPU walks (IPX_JPEG_PROG_GPU=1, a clean marker pre-pass): their programs -- files,
// scans, table definitions -- go up in one block, one wave per file walks the scans in file order into the coefficient slots that
// dec_upload zeroed.  The files' bytes are in the blob already.
int dec_scans(DecRun &r)
{
    const JpegBatchPlan &P = r.plan;
    if (P.gfiles.empty()) return IPX_OK;
    const JpegDecArgs &a = r.a;
    size_t nscans = 0, ndefs = 0;
    for (int i : P.gfiles) { nscans += P.prog[i].scans.size(); ndefs += P.prog[i].defs.size(); }
    const size_t nf = P.gfiles.size();
    const size_t off_scans = align16(nf * sizeof(JpegProgFile)), off_defs = align16(off_scans + nscans * sizeof(JpegProgScan));
    r.prog_block.assign(off_defs + ndefs * sizeof(JpegProgHuff) + 16, 0);
    JpegProgFile *hf = (JpegProgFile *)r.prog_block.data();
    JpegProgScan *hs = (JpegProgScan *)(r.prog_block.data() + off_scans);
    JpegProgHuff *hd = (JpegProgHuff *)(r.prog_block.data() + off_defs);
    uint32_t s0 = 0, d0 = 0;
    for (size_t k = 0; k < nf; k++) {
        const int i = P.gfiles[k];
        const JpegProgPlan &G = P.prog[i];
        hf[k] = JpegProgFile{(unsigned long long)P.blob_off[i], (uint32_t)i, (uint32_t)G.scans.size(), s0, d0};
        if (!G.scans.empty()) memcpy(hs + s0, G.scans.data(), G.scans.size() * sizeof(JpegProgScan));
        if (!G.defs.empty()) memcpy(hd + d0, G.defs.data(), G.defs.size() * sizeof(JpegProgHuff));
        s0 += (uint32_t)G.scans.size(); d0 += (uint32_t)G.defs.size();
    }
    uint8_t *d_prog = nullptr;
    DEC_HIP("jpeg decode", r.mem.get(&d_prog, r.prog_block.size()));
    DEC_HIP("jpeg decode", hipMemcpyAsync(d_prog, r.prog_block.data(), r.prog_block.size(), hipMemcpyHostToDevice, r.s));
    JpegProgArgs g{};
    g.blob = r.d_blob; g.files = (const JpegProgFile *)d_prog; g.scans = (const JpegProgScan *)(d_prog + off_scans); g.defs = (const JpegProgHuff *)(d_prog + off_defs);
    g.coefs = a.coefs; g.dcs = a.dcs; g.status = a.status;
    g.nfiles = (int)nf; g.mxx = a.mxx; g.myy = a.myy; g.h0 = a.h0; g.v0 = a.v0; g.nblk = a.nblk; g.w = a.w; g.h = a.h; g.bpm = a.bpm; g.ybl = a.ybl;
    DEC_HIP("jpeg decode", launch_jpeg_prog(g, r.s));
    return IPX_OK;
}

// the blocks and the launch arguments of the passes that are parallel inside a scan
int par_setup(DecRun &r, JpegParArgs &P, uint32_t **d_tot)
{
    std::vector<JpegParImage> &par = r.plan.par;
    const JpegDecArgs &a = r.a;
    hipStream_t s = r.s;
    const size_t blob_bytes = r.plan.blob_bytes;
    P.blob = r.d_blob; P.tab = r.d_tab; P.nimg = (int)par.size(); P.bpm = a.bpm; P.ybl = a.ybl; P.nblk = a.nblk;
    P.geom = a.geom;
    P.coefs = a.coefs; P.status = a.status; P.dcs = a.dcs;
    P.sub = r.plan.par_sub;
    for (auto &pi : par) P.max_nsub = std::max(P.max_nsub, (int)pi.nsub);
    r.max_nsub = P.max_nsub;
    for (size_t k = 0; k < par.size(); k++) par[k].sub_off = k * (size_t)P.max_nsub;
    const size_t nsubs = par.size() * (size_t)P.max_nsub, cks = (size_t)jpeg_par_checkpoints();
    // The scan bytes of a wave's 64 sub-sequences staged in LDS (small batches: a SIMD has one wave, which would wait for a global load
    // nearly every symbol), or read through L1 / L2 (big ones lose more to the occupancy the rows cost): DESIGN.md section 4.6
    P.stage_rows = env_int("IPX_JPEG_PAR_STAGE", -1);
    if (P.stage_rows < 0) P.stage_rows = nsubs <= (size_t)env_int("IPX_JPEG_PAR_STAGE_SUBS", 98304) ? 1 : 0;
    JpegParImage *d_par = nullptr;
    DEC_HIP("jpeg decode", r.mem.get(&d_par, sizeof(JpegParImage) * par.size()));
    DEC_HIP("jpeg decode", r.mem.get(&P.stuffed, nsubs * 4));
    DEC_HIP("jpeg decode", r.mem.get(&P.entry, nsubs * 8));
    DEC_HIP("jpeg decode", r.mem.get(&P.exit_a, nsubs * 8));
    DEC_HIP("jpeg decode", r.mem.get(&P.exit_b, nsubs * 8));
    DEC_HIP("jpeg decode", r.mem.get(&P.ends, nsubs * 4));
    DEC_HIP("jpeg decode", r.mem.get(&P.ck_state, nsubs * 8 * cks));
    DEC_HIP("jpeg decode", r.mem.get(&P.ck_ends, nsubs * 4 * cks));
    DEC_HIP("jpeg decode", r.mem.get(&P.total_ends, par.size() * 4));
    DEC_HIP("jpeg decode", r.mem.get(d_tot, par.size() * 4));
    DEC_HIP("jpeg decode", r.mem.get(&P.changed, 4));
    P.img = d_par;
    DEC_HIP("jpeg decode", hipMemcpyAsync(d_par, par.data(), sizeof(JpegParImage) * par.size(), hipMemcpyHostToDevice, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.stuffed, 0, nsubs * 4, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.entry, 0xff, nsubs * 8, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.ends, 0, nsubs * 4, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.ck_state, 0xff, nsubs * 8 * cks, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.ck_ends, 0, nsubs * 4 * cks, s));
    DEC_HIP("jpeg decode", r.mem.get(&P.ublob, blob_bytes + 64));
    DEC_HIP("jpeg decode", r.mem.get(&P.scan_end, par.size() * 4));
    DEC_HIP("jpeg decode", r.mem.get(&P.ulen, par.size() * 4));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.ublob, 0, blob_bytes + 64, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.scan_end, 0xff, par.size() * 4, s));
    DEC_HIP("jpeg decode", hipMemsetAsync(P.ulen, 0, par.size() * 4, s));
    return IPX_OK;
}

// a scan that never settled (it would take a pathological file): its image goes whole to the serial kernel
int par_fallback(DecRun &r)
{
    const JpegDecArgs &a = r.a;
    std::vector<JpegDecImage> serial;
    for (auto &pi : r.plan.par) {
        JpegDecImage it;
        memset(&it, 0, sizeof it);
        it.scan_off = pi.scan_off; it.scan_len = pi.scan_len; it.img = pi.img; it.first_mcu = 0; it.n_mcu = (uint32_t)(r.nblk((int)pi.img) / (size_t)a.bpm);
        memcpy(it.td, pi.td, 3); memcpy(it.ta, pi.ta, 3);
        it.valid = 1;
        serial.push_back(it);
    }
    StreamSync wait{r.s};               // `serial` must outlive the copy
    JpegDecImage *d_serial;
    DEC_HIP("jpeg decode", r.mem.get(&d_serial, sizeof(JpegDecImage) * serial.size()));
    DEC_HIP("jpeg decode", hipMemcpyAsync(d_serial, serial.data(), sizeof(JpegDecImage) * serial.size(), hipMemcpyHostToDevice, r.s));
    JpegDecArgs a2 = a;
    a2.img = d_serial; a2.nitems = (int)serial.size();
    DEC_HIP("jpeg decode", launch_jpeg_huff(a2, r.s));
    return IPX_OK;
}

// the passes that are parallel inside a scan: count and unstuff, the speculative pass, rounds until no entry state changes (the host reads
// one counter per round), then the write and DC passes -- or the serial kernel
int dec_parallel(DecRun &r)
{
    hipStream_t s = r.s;
    JpegParArgs P{};
    uint32_t *d_tot = nullptr;
    const int rc = par_setup(r, P, &d_tot);
    if (rc) return rc;
    DEC_HIP("jpeg decode", launch_par_count(P, s));
    DEC_HIP("jpeg decode", launch_scan(P.stuffed, P.max_nsub, P.nimg, d_tot, s));
    DEC_HIP("jpeg decode", launch_par_unstuff(P, s));
    DEC_HIP("jpeg decode", launch_par_sync(P, 0, s));
    bool converged = false;
    const int max_rounds = env_int("IPX_JPEG_PAR_ROUNDS", 96);
    for (int round = 1; !converged && round <= max_rounds; round++) {
        uint32_t changed = 0;
        DEC_HIP("jpeg decode", hipMemsetAsync(P.changed, 0, 4, s));
        DEC_HIP("jpeg decode", launch_par_sync(P, round, s));
        DEC_HIP("jpeg decode", hipMemcpyAsync(&changed, P.changed, 4, hipMemcpyDeviceToHost, s));
        const hipError_t e = hipStreamSynchronize(s);
        if (getenv("IPX_DEBUG")) fprintf(stderr, "[ipx] jpeg par sync round %d: %u entries changed\n", round, changed);
        DEC_HIP("jpeg decode", e);
        converged = changed == 0;
    }
    if (!converged) return par_fallback(r);
    DEC_HIP("jpeg decode", launch_scan(P.ends, P.max_nsub, P.nimg, P.total_ends, s));
    DEC_HIP("jpeg decode", launch_par_write(P, s));
    DEC_HIP("jpeg decode", launch_par_dc(P, s));
    return IPX_OK;
}

// Stage 4: the pieces (or the byte-wise kernel), then the scans that are decoded in parallel
int dec_huffman(DecRun &r)
{
    const JpegBatchPlan &P = r.plan;
    JpegDecArgs &a = r.a;
    int ref_gpu = -1;                                        // the first image the Huffman kernels decode: the one whose tables a shared-table launch carries
    for (int i = 0; i < r.n && ref_gpu < 0; i++) if (P.valid[i] && !P.info[i].host_scans) ref_gpu = i;
    a.first_valid = ref_gpu >= 0 ? ref_gpu : P.ref;
    a.shared_tables = env_int("IPX_JPEG_SHARED_TABLES", 1);
    for (int i = 0; i < r.n && a.shared_tables && ref_gpu >= 0; i++)
        if (P.valid[i] && !P.info[i].host_scans && !jpeg_same_tables(P.tabs[i], P.tabs[ref_gpu])) a.shared_tables = 0;
    if (a.nitems > 0) {
        if (env_int("IPX_JPEG_PIECE", 1)) {
            uint8_t *d_upieces; uint32_t *d_ulen;
            DEC_HIP("jpeg decode", r.mem.get(&d_upieces, P.piece_ubytes + 64));
            DEC_HIP("jpeg decode", r.mem.get(&d_ulen, sizeof(uint32_t) * P.items.size()));
            DEC_HIP("jpeg decode", launch_jpeg_pieces(a, d_upieces, d_ulen, r.s));
        } else {
            DEC_HIP("jpeg decode", launch_jpeg_huff(a, r.s));     // the earlier kernel: byte-wise reader, per-lane tables when the files of the batch carry different ones
        }
    }
    return P.par.empty() ? IPX_OK : dec_parallel(r);
}

// Stage 5: the reconstruction, the kernels' verdicts, and the planes handed out
int dec_finish(DecRun &r, ipx_ycbcr_batch *planes)
{
    DEC_HIP("jpeg decode", launch_jpeg_idct(r.a, r.pl, r.s));
    r.t_launch = r.ms();
    r.dev_status.assign(r.n, 0);
    DEC_HIP("jpeg decode", hipMemcpyAsync(r.dev_status.data(), r.a.status, sizeof(int) * r.n, hipMemcpyDeviceToHost, r.s));
    DEC_HIP("jpeg decode", hipStreamSynchronize(r.s));
    if ((getenv("IPX_DEBUG") && r.ms() > 200.0) || env_int("IPX_DEBUG_J2J", 0))
        fprintf(stderr, "[ipx] decode of %d files%s: parsed at %.1f ms, device scratch at %.1f, pinned block at %.1f, packed at %.1f, launched at %.1f, finished at %.1f; planes %.1f MB, scratch %.1f MB, %d sub-sequences at most\n",
                r.n, r.mixed ? " of mixed sizes" : "", r.plan.parse_ms, r.t_alloc, r.t_pin, r.t_pack, r.t_launch, r.ms(), r.plane_bytes / 1e6, r.scratch_bytes / 1e6, r.max_nsub);
    const JpegBatchPlan &P = r.plan;
    for (int i = 0; i < r.n; i++) {
        const bool walked = P.route[i] == IPX_JPEG_ROUTE_GPU_SCANS;
        if (r.status[i] == IPX_OK && r.dev_status[i]) r.status[i] = jpeg_status_of(r.dev_status[i]);
        if (walked && r.dev_status[i] == jpeg_status_key(kJpegProgHostVerdict, IPX_ERR_UNSUPPORTED)) {
            // a coefficient of this (damaged) file truncated to zero in int16: the host decoder, whose walk differs from there on, says
            // which way it fails -- it has no planes either way
            std::vector<int16_t> scratch((size_t)r.a.nblk * 65);
            JpegDecInfo full;
            uint16_t q[3][64];
            bool prog = false;
            const int st = jpeg_host_decode(r.jpegs[i].data, r.jpegs[i].len, &full, scratch.data(), scratch.data() + (size_t)r.a.nblk * 64, (size_t)r.a.nblk, q, &prog);
            r.status[i] = st != IPX_OK ? st : IPX_ERR_UNSUPPORTED;
        }
        // by route: every file that reached its decoder, whatever came of it
        if (P.route[i] <= IPX_JPEG_ROUTE_GPU_SCANS) r.ctx->jpeg_counts[P.route[i]]++;
        if (walked && r.status[i] != IPX_OK) r.ctx->jpeg_counts[3]++;
    }
    if (!planes) return IPX_OK;         // a mixed-size class: its caller describes every file's planes (decode_class)
    planes->y = r.pl.y; planes->cb = r.pl.cb; planes->cr = r.pl.cr;
    planes->ystride = r.pl.ystride; planes->cstride = r.pl.cstride;
    planes->y_frame_stride = r.pl.y_fs; planes->c_frame_stride = r.pl.c_fs;
    planes->ratio = r.plan.info[r.plan.ref].ratio;
    return IPX_OK;
}

// One sampling class of a mixed-size call: files [0, n) -- parsed already, `parsed` holds what jpeg_plan_parse left for them -- of any
// sizes through ONE run of the stages above.  The planes are blocks of `own`; frames[i] describes file i's, all zero unless it decoded.
int decode_class(ipx_ctx *ctx, hipStream_t s, Lane *lane, const ipx_bytes *jpegs, int n, JpegBatchPlan &&parsed, const JpegPlanOptions &opt,
                 OwnedBlocks<ipx_jpeg_planes> &own, ipx_jpeg_frame *frames, int *status)
{
    DecRun r(ctx, s, jpegs, n, status);
    r.mixed = true;
    r.plan = std::move(parsed);
    jpeg_plan_place(jpegs, n, opt, status, &r.plan);
    if (r.plan.ref < 0) return IPX_OK;
    int rc = dec_blocks(r, lane, false, own);
    if (!rc) rc = dec_upload(r);
    if (!rc) rc = dec_huffman(r);
    if (!rc) rc = dec_finish(r, nullptr);
    if (rc) return rc;
    const bool gray = r.a.bpm == 1;
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        const JpegMixGeom &g = r.geom[i];
        frames[i] = ipx_jpeg_frame{g.w, g.h, r.plan.info[i].ratio, r.pl.y + g.yoff, gray ? nullptr : r.pl.cb + g.coff, gray ? nullptr : r.pl.cr + g.coff,
                                   g.ystride, gray ? 0 : g.cstride};
    }
    return IPX_OK;
}

}  // namespace

// The two halves of a mixed-size decode (ipx_decode_common.h).  The GPU scan walk and 4:1:1 / 4:1:0 are off in both whatever their
// switches say.
static JpegPlanOptions mixed_options()
{
    return JpegPlanOptions{0, 0, env_int("IPX_JPEG_PAR", 1) != 0, env_int("IPX_JPEG_PAR_SUB", 0), jpeg_par_sub_bytes(), false, false, true};
}

int jpeg_mixed_parse(const ipx_bytes *jpegs, int n, int *status, JpegBatchPlan *all) { return jpeg_plan_parse(jpegs, n, mixed_options(), status, all); }

// one decode_class per sampling class -- (h0, v0, components) -- of the m files idx[0 .. m), each class's files in idx's order
int jpeg_mixed_decode(ipx_ctx *ctx, hipStream_t s, Lane *lane, const ipx_bytes *jpegs, JpegBatchPlan &all, const int *idx, int m,
                      OwnedBlocks<ipx_jpeg_planes> &own, ipx_jpeg_frame *frames, int *status)
{
    const JpegPlanOptions opt = mixed_options();
    std::vector<uint8_t> taken(m, 0);
    for (int first = 0; first < m; first++) {
        if (taken[first] || status[idx[first]] != IPX_OK) continue;
        const JpegDecInfo F = all.info[idx[first]];
        std::vector<int> of;                                  // the class's files, by the caller's index
        for (int g = first; g < m; g++) {
            const JpegDecInfo &I = all.info[idx[g]];
            if (!taken[g] && status[idx[g]] == IPX_OK && I.h0 == F.h0 && I.v0 == F.v0 && I.ncomp == F.ncomp) { of.push_back(idx[g]); taken[g] = 1; }
        }
        const int c = (int)of.size();
        std::vector<ipx_bytes> files(c);
        std::vector<ipx_jpeg_frame> fr(c, ipx_jpeg_frame{});
        std::vector<int> st(c, IPX_OK);
        JpegBatchPlan P;
        P.info.resize(c); P.tabs.resize(c); P.prog.resize(c); P.marks.resize(c);
        P.parse_ms = all.parse_ms;
        for (int k = 0; k < c; k++) {
            const int i = of[k];
            files[k] = jpegs[i];
            P.info[k] = all.info[i]; P.tabs[k] = all.tabs[i]; P.marks[k] = std::move(all.marks[i]);
        }
        const int rc = decode_class(ctx, s, lane, files.data(), c, std::move(P), opt, own, fr.data(), st.data());
        if (rc) return rc;
        for (int k = 0; k < c; k++) { status[of[k]] = st[k]; if (st[k] == IPX_OK) frames[of[k]] = fr[k]; }
    }
    return IPX_OK;
}

// lane != NULL: scratch is bumped out of the lane's decode buffer (no allocation in the steady state); planes_in_lane: the planes too --
// the caller then holds the lane for as long as it uses them and *owner has nothing to free
int jpeg_decode_files(ipx_ctx *ctx, hipStream_t s, Lane *lane, bool planes_in_lane, const ipx_bytes *jpegs, int n, int *w, int *h,
                      ipx_ycbcr_batch *planes, int *status, ipx_jpeg_planes **owner)
{
    OwnedBlocks<ipx_jpeg_planes> own(ctx, s);
    DecRun r(ctx, s, jpegs, n, status);
    r.s411 = jpeg_411_enabled();
    const JpegPlanOptions opt{*w, *h, env_int("IPX_JPEG_PAR", 1) != 0, env_int("IPX_JPEG_PAR_SUB", 0), jpeg_par_sub_bytes(), env_int("IPX_JPEG_PROG_GPU", 0) == 1, r.s411};
    int rc = jpeg_plan_batch(jpegs, n, opt, status, &r.plan);
    if (rc) return rc;
    if (r.plan.ref < 0) return IPX_OK;
    *w = r.plan.info[r.plan.ref].w; *h = r.plan.info[r.plan.ref].h;
    rc = dec_blocks(r, lane, planes_in_lane, own);
    if (!rc) rc = dec_upload(r);
    if (!rc) rc = dec_scans(r);
    if (!rc) rc = dec_huffman(r);
    if (!rc) rc = dec_finish(r, planes);
    if (rc) return rc;
    *owner = own.release();
    return IPX_OK;
}

bool jpeg_411_enabled() { return env_int("IPX_JPEG_411", 0) == 1; }

extern "C" {

void ipx_jpeg_planes_free(ipx_ctx *ctx, ipx_jpeg_planes *o) { dev_blocks_free(ctx, o); }

int ipx_jpeg_decode_batch(ipx_ctx *ctx, void *stream, const ipx_bytes *jpegs, int n, int *w, int *h, ipx_ycbcr_batch *planes,
                          int *status, ipx_jpeg_planes **owner) try
{
    IPX_ENTER(ctx);
    if (!jpegs || n < 0 || !w || !h || !planes || !status || !owner) { set_error("ipx_jpeg_decode_batch: bad argument"); return IPX_ERR_INVALID; }
    *owner = nullptr;
    memset(planes, 0, sizeof *planes);
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_jpeg_decode_batch: at most 65535 files per call"); return IPX_ERR_UNSUPPORTED; }
    // the scratch comes out of a lane's decode buffer for the duration of the call; the planes are the caller's (stream-ordered allocations)
    LaneLease lane(ctx);
    return jpeg_decode_files(ctx, stream ? (hipStream_t)stream : ctx->stream, env_int("IPX_JPEG_LANE_ARENA", 1) ? &lane.get() : nullptr, false, jpegs, n, w, h,
                             planes, status, owner);
}
IPX_CATCH_STATUS

int ipx_jpeg_decode_mixed(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, ipx_jpeg_frame *frames, int *status,
                          ipx_jpeg_planes **owner) try
{
    IPX_ENTER(ctx);
    if (n < 0 || !owner || (n && (!files || !frames || !status))) { set_error("ipx_jpeg_decode_mixed: bad argument"); return IPX_ERR_INVALID; }
    *owner = nullptr;
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_jpeg_decode_mixed: at most 65535 files per call"); return IPX_ERR_UNSUPPORTED; }
    memset(frames, 0, sizeof(ipx_jpeg_frame) * (size_t)n);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    OwnedBlocks<ipx_jpeg_planes> own(ctx, s);
    JpegBatchPlan all;
    int rc = jpeg_mixed_parse(files, n, status, &all);
    if (rc) return rc;
    std::vector<int> idx(n);
    for (int i = 0; i < n; i++) idx[i] = i;
    // the scratch comes out of a lane's decode buffer for the duration of the call; the planes are the caller's (stream-ordered allocations)
    LaneLease lane(ctx);
    rc = jpeg_mixed_decode(ctx, s, env_int("IPX_JPEG_LANE_ARENA", 1) ? &lane.get() : nullptr, files, all, idx.data(), n, own, frames, status);
    if (rc) return rc;
    if (any_ok(status, n)) *owner = own.release();
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_jpeg_scan_route(const uint8_t *file, size_t len, int *route) try
{
    clear_error();
    if (!file || !route) { set_error("ipx_jpeg_scan_route: bad argument"); return IPX_ERR_INVALID; }
    *route = IPX_JPEG_ROUTE_PAR;
    if (len >= ((size_t)1 << 30)) return IPX_ERR_UNSUPPORTED;
    JpegDecInfo info;
    JpegDecTables tab;
    const int st = jpeg_parse(file, len, &info, &tab, jpeg_cmyk_enabled(), jpeg_411_enabled());   // (a four-component file: the host route, under IPX_JPEG_CMYK=1)
    if (st != IPX_OK) return st;
    if (info.host_scans) {
        JpegProgPlan plan;
        const bool gpu = env_int("IPX_JPEG_PROG_GPU", 0) == 1 && info.progressive && info.h0 <= 2 && jpeg_prog_prepass(file, len, info, &plan, tab.qnat);
        *route = gpu ? IPX_JPEG_ROUTE_GPU_SCANS : IPX_JPEG_ROUTE_HOST_SCANS;
    }
    return IPX_OK;
}
IPX_CATCH_STATUS

int ipx_jpeg_decode_counts(ipx_ctx *ctx, long long counts[4])
{
    clear_error();
    if (!ctx || !counts) { set_error("ipx_jpeg_decode_counts: bad argument"); return IPX_ERR_INVALID; }
    for (int k = 0; k < 4; k++) counts[k] = ctx->jpeg_counts[k].load();
    return IPX_OK;
}

}  // extern "C"
