// ipx_jpeg_dec_cmyk.hip -- image.Decode for four-component JPEGs (Adobe CMYK and YCCK), opt-in by IPX_JPEG_CMYK=1.
//
// Go's image/jpeg decodes components 0..2 of such a file into an *image.YCbCr (4:4:4 for the sampling vector 11 11 11 11, 4:2:0 for
// 22 11 11 22 -- processSOF takes no other) and component 3 into blackPix at component 0's resolution; after EOI applyBlack turns the
// four planes into an *image.CMYK by the APP14 transform byte:
//   transform != 0 (YCCK)   imageutil.DrawYCbCr of the three planes into an RGBA buffer, then Pix[4i+3] = 255 - K: R, G, B are stored as
//                           they are (the inversion Adobe files carry and the one CMYK asks for cancel)
//   transform == 0 (CMYK)   Pix[4i+t] = 255 - plane_t[sy * stride + sx] for t = 0..3, (sx, sy) the pixel's coordinates, halved for a
//                           component whose (h, v) differs from component 0's (M and Y of the 22 vector)
// (restated from reader.go as recalled, not read: DESIGN.md section 4.6.)
//
// The split: every scan of a four-component file is walked on the host pool's threads (jpeg_host_decode4, ipx_jpeg_dec_prog.cpp), baseline
// and progressive alike, into two coefficient sets in layouts the IDCT kernel already reads -- a three-component image and a Gray image.
// launch_jpeg_idct runs once on each (Go's idct.go as pinned for every other file), and jpeg_cmyk_assemble_kernel below turns the four
// MCU-padded planes into tightly packed *image.CMYK frames, the layout ipx_plan_run_dev_deep(IPX_DEEP_CMYK) takes.
#include <algorithm>

#include "ipx_decode_common.h"
#pragma clang fp contract(off)
#include "ipx_device.h"

namespace ipx {
namespace {

struct CmykAsmArgs {
    const uint8_t *y, *cb, *cr, *k;     // the planes as launch_jpeg_idct leaves them; K has Y's geometry
    int ystride, cstride;
    size_t y_fs, c_fs;
    uint8_t *pix;                        // frames of w * 4 bytes per row
    int stride;
    size_t fs;
    int w, h;
    int half;                            // 1: the chroma planes are 4:2:0 (sampling vector 22 11 11 22)
    const uint8_t *kind;                 // per file: 0 no frame, 1 transform 0 (CMYK), 2 any other transform (YCCK)
};

// A lane takes four adjacent pixels of kAsmRows consecutive rows.  Per row: a dword of Y and of K (the planes' rows are multiples of 8
// bytes long and x is a multiple of 4: aligned, and never past the row), a dword (4:4:4) or two bytes (4:2:0: the pixels x .. x + 3
// share chroma x / 2 and x / 2 + 1) of Cb and Cr, and one 16-byte store where the frame's rows are 16-byte aligned and all four pixels
// exist; pixel by pixel otherwise (w not a multiple of 4: rows are not aligned, and the last lane of a row must not reach into the
// next).  All loads of the rows go out before the first pixel is computed (rows beyond the image load the last row again and store
// nothing); a workgroup of one row was 0.95 ms per 256 1080p frames, most of it workgroup turnover.  7 to 8 bytes moved per pixel.
constexpr int kAsmRows = 4;
template <bool YCCK>
__global__ __launch_bounds__(256) void jpeg_cmyk_assemble_kernel(CmykAsmArgs a)
{
    const int img = blockIdx.z;
    if (a.kind[img] != (YCCK ? 2 : 1)) return;            // uniform over the workgroup
    const int y0 = (int)blockIdx.y * kAsmRows, x = (int)(blockIdx.x * 256 + threadIdx.x) * 4;
    if (x >= a.w) return;
    const uint8_t *py = a.y + (size_t)img * a.y_fs + x, *pk = a.k + (size_t)img * a.y_fs + x;
    const uint8_t *pcb = a.cb + (size_t)img * a.c_fs + (a.half ? x >> 1 : x), *pcr = a.cr + (size_t)img * a.c_fs + (a.half ? x >> 1 : x);
    uint32_t yv[kAsmRows], kv[kAsmRows], cbv[kAsmRows], crv[kAsmRows];     // cbv / crv: the four pixels' chroma samples, one per byte
#pragma unroll
    for (int r = 0; r < kAsmRows; r++) {
        const int y = min(y0 + r, a.h - 1);
        yv[r] = *(const uint32_t *)(py + (size_t)y * a.ystride); kv[r] = *(const uint32_t *)(pk + (size_t)y * a.ystride);
        if (a.half) {
            const size_t ci = (size_t)(y >> 1) * a.cstride;
            cbv[r] = *(const uint16_t *)(pcb + ci); crv[r] = *(const uint16_t *)(pcr + ci);
        } else {
            const size_t ci = (size_t)y * a.cstride;
            cbv[r] = *(const uint32_t *)(pcb + ci); crv[r] = *(const uint32_t *)(pcr + ci);
        }
    }
#pragma unroll
    for (int r = 0; r < kAsmRows; r++) {
        const int y = y0 + r;
        if (y >= a.h) break;
        uint32_t cb4 = cbv[r], cr4 = crv[r];
        if (a.half) { cb4 = (cb4 & 0xffu) * 0x101u | (cb4 >> 8) * 0x1010000u; cr4 = (cr4 & 0xffu) * 0x101u | (cr4 >> 8) * 0x1010000u; }
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t ys = (yv[r] >> (8 * i)) & 0xffu, bs = (cb4 >> (8 * i)) & 0xffu, rs = (cr4 >> (8 * i)) & 0xffu, ks = (kv[r] >> (8 * i)) & 0xffu;
            if (YCCK) o[i] = (ycbcr_to_rgb8(ys, bs, rs) & 0xffffffu) | (255u - ks) << 24;
            else o[i] = (255u - ys) | (255u - bs) << 8 | (255u - rs) << 16 | (255u - ks) << 24;
        }
        uint8_t *dp = a.pix + (size_t)img * a.fs + (size_t)y * a.stride + (size_t)x * 4;
        if ((a.stride & 15) == 0 && x + 4 <= a.w) { *(uint4 *)dp = make_uint4(o[0], o[1], o[2], o[3]); continue; }
#pragma unroll
        for (int i = 0; i < 4; i++) if (x + i < a.w) ((uint32_t *)dp)[i] = o[i];
    }
}

hipError_t launch_cmyk_assemble(const CmykAsmArgs &a, int n, bool ycck, hipStream_t s)
{
    const dim3 grid((unsigned)(((a.w + 3) / 4 + 255) / 256), (unsigned)((a.h + kAsmRows - 1) / kAsmRows), (unsigned)n);
    if (ycck) hipLaunchKernelGGL(jpeg_cmyk_assemble_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(jpeg_cmyk_assemble_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

int hip_status(hipError_t e, const char *what)
{
    if (e != hipSuccess) set_error("%s: %s", what, hipGetErrorString(e));
    return e == hipSuccess ? IPX_OK : IPX_ERR_HIP;
}
#define CMYK_HIP(call) do { const int rc_ = hip_status((call), "jpeg cmyk decode"); if (rc_) return rc_; } while (0)

struct Events { hipEvent_t ev[2] = {nullptr, nullptr}; ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); } };

}  // namespace
}  // namespace ipx

bool jpeg_cmyk_enabled() { return env_int("IPX_JPEG_CMYK", 0) == 1; }

// component 0's sampling factor (1 or 2: the vector) of a file whose frame header announces four components in a vector Go takes; 0 for
// every other file (the legs' test of what they take out of a call)
int jpeg_cmyk_peek(const uint8_t *d, size_t len)
{
    JpegDecInfo info;
    JpegDecTables tab;
    return d && len < ((size_t)1 << 30) && jpeg_parse(d, len, &info, &tab, true) == IPX_OK && info.ncomp == 4 ? info.h0 : 0;
}

// The driver: the four-component files of the call that share the size asked for (or the first decodable one's) and one sampling vector
// are decoded; everything else gets its status.  frames->pix stays NULL when no file was decodable.
int jpeg_decode_cmyk_files(ipx_ctx *ctx, hipStream_t s, const ipx_bytes *jpegs, int n, int *w, int *h, int want_h0, ipx_cmyk_batch *frames,
                           int *status, ipx_jpeg_planes **owner)
{
    static const char *const kPrep = "jpeg cmyk decode: host preparation failed";
    const bool on = jpeg_cmyk_enabled();
    std::vector<JpegDecInfo> info(n);
    int rc = parallel_light(n, [&](int i) {
        JpegDecTables tab;                                 // (the Huffman tables of these files are the host decoder's)
        status[i] = !jpegs[i].data ? IPX_ERR_INVALID : (jpegs[i].len >= ((size_t)1 << 30) ? IPX_ERR_UNSUPPORTED : jpeg_parse(jpegs[i].data, jpegs[i].len, &info[i], &tab, on));
        if (status[i] == IPX_OK && info[i].ncomp != 4) status[i] = IPX_ERR_UNSUPPORTED;        // *image.YCbCr / *image.Gray: ipx_jpeg_decode_batch's
    }, kPrep);
    if (rc) return rc;
    int ref = -1;
    for (int i = 0; i < n; i++) {
        if (status[i] != IPX_OK) continue;
        if (ref < 0 && (*w <= 0 || (info[i].w == *w && info[i].h == *h)) && (want_h0 <= 0 || info[i].h0 == want_h0)) ref = i;
        if (ref < 0 || info[i].w != info[ref].w || info[i].h != info[ref].h || info[i].h0 != info[ref].h0) status[i] = IPX_ERR_UNSUPPORTED;
    }
    if (ref < 0) return IPX_OK;
    const JpegDecInfo R = info[ref];
    *w = R.w; *h = R.h;
    if (!frame_span_ok(R.w, R.h, (long long)R.w * 4, 4)) {
        for (int i = 0; i < n; i++) if (status[i] == IPX_OK) status[i] = IPX_ERR_UNSUPPORTED;
        return IPX_OK;
    }
    std::vector<int> todo;
    for (int i = 0; i < n; i++) if (status[i] == IPX_OK) todo.push_back(i);
    ctx->jpeg_cmyk_files += (long long)todo.size();

    // the two launches of the IDCT kernel: a three-component image of the file's sampling, and a Gray image of component 0's block grid
    JpegDecArgs a3{}, ak{};
    JpegPlanes p3{}, pk{};
    a3.n = n; a3.h0 = R.h0; a3.v0 = R.v0; a3.w = R.w; a3.h = R.h;
    a3.mxx = (R.w + 8 * R.h0 - 1) / (8 * R.h0); a3.myy = (R.h + 8 * R.v0 - 1) / (8 * R.v0);
    a3.ybl = R.h0 * R.v0; a3.bpm = a3.ybl + 2; a3.nblk = a3.mxx * a3.myy * a3.bpm;
    ak.n = n; ak.h0 = ak.v0 = 1; ak.w = R.w; ak.h = R.h;
    ak.mxx = R.h0 * a3.mxx; ak.myy = R.v0 * a3.myy; ak.ybl = ak.bpm = 1; ak.nblk = ak.mxx * ak.myy;
    p3.ystride = 8 * R.h0 * a3.mxx; p3.cstride = 8 * a3.mxx;
    p3.y_fs = align256((size_t)p3.ystride * 8 * R.v0 * a3.myy); p3.c_fs = align256((size_t)p3.cstride * 8 * a3.myy);
    pk.ystride = p3.ystride; pk.y_fs = p3.y_fs;
    const size_t nb3 = (size_t)a3.nblk, nbk = (size_t)ak.nblk, nblk = nb3 + nbk;
    ipx_cmyk_batch out{};
    out.stride = R.w * 4; out.frame_stride = align256((size_t)out.stride * R.h);

    OwnedBlocks<ipx_jpeg_planes> own(ctx, s);
    // in reverse order of need: the wait for the stream, the pinned blocks, the scratch, then the host vectors the copies read
    std::vector<JpegDecTables> tab3(n), tabk(n);
    std::vector<uint8_t> valid(n, 0), kind(n, 0);
    AsyncFree mem{s, {}};
    PinnedBlocks pinned(ctx, s);
    StreamSync sync{s};
    memset(tab3.data(), 0, sizeof(JpegDecTables) * n); memset(tabk.data(), 0, sizeof(JpegDecTables) * n);
    uint8_t *d_valid = nullptr, *d_kind = nullptr;
    JpegDecTables *d_tab3 = nullptr, *d_tabk = nullptr;
    CMYK_HIP(own.alloc(&out.pix, out.frame_stride * n));
    CMYK_HIP(mem.get(&p3.y, p3.y_fs * n));
    CMYK_HIP(mem.get(&p3.cb, p3.c_fs * n));
    CMYK_HIP(mem.get(&p3.cr, p3.c_fs * n));
    CMYK_HIP(mem.get(&pk.y, pk.y_fs * n));
    CMYK_HIP(mem.get(&a3.coefs, (size_t)n * nb3 * 128));
    CMYK_HIP(mem.get(&a3.dcs, (size_t)n * nb3 * 2 + 16));
    CMYK_HIP(mem.get(&ak.coefs, (size_t)n * nbk * 128));
    CMYK_HIP(mem.get(&ak.dcs, (size_t)n * nbk * 2 + 16));
    CMYK_HIP(mem.get(&d_valid, (size_t)n));
    CMYK_HIP(mem.get(&d_kind, (size_t)n));
    CMYK_HIP(mem.get(&d_tab3, sizeof(JpegDecTables) * n));
    CMYK_HIP(mem.get(&d_tabk, sizeof(JpegDecTables) * n));
    a3.tab = d_tab3; ak.tab = d_tabk; p3.valid = pk.valid = d_valid;

    // the scans, in groups on the pool's threads into one half of a pinned block while the copies of the group before leave the other
    const size_t slot_words = nblk * 65;                   // per file: the coefficients of both sets, then their DC terms
    const int group = std::max(1, std::min((int)todo.size(), env_int("IPX_JPEG_HOST_GROUP", 16)));
    int16_t *hpin = (int16_t *)pinned.get((size_t)2 * group * slot_words * sizeof(int16_t));
    if (!hpin) return IPX_ERR_NOMEM;
    Events ev;
    for (int g0 = 0, gi = 0; g0 < (int)todo.size(); g0 += group, gi++) {
        const int half = gi & 1, cnt = std::min(group, (int)todo.size() - g0);
        int16_t *base = hpin + (size_t)half * group * slot_words;
        if (gi >= 2) CMYK_HIP(hipEventSynchronize(ev.ev[half]));
        rc = parallel_heavy(cnt, [&](int j) {
            const int i = todo[g0 + j];
            int16_t *slot = base + (size_t)j * slot_words;
            bool prog = false;
            int transform = 0;
            JpegDecInfo full;
            uint16_t q[4][64];
            const int st = jpeg_host_decode4(jpegs[i].data, jpegs[i].len, &full, slot, slot + nblk * 64, nblk, q, &prog, &transform);
            if (st != IPX_OK) { status[i] = st; return; }
            memcpy(tab3[i].qnat, q, sizeof tab3[i].qnat);
            memcpy(tabk[i].qnat[0], q[3], sizeof q[3]);
            valid[i] = prog ? 3 : 1;
            kind[i] = transform == 0 ? 1 : 2;
        }, kPrep);
        if (rc) return rc;
        for (int j = 0; j < cnt; j++) {
            const int i = todo[g0 + j];
            if (!valid[i]) continue;
            const int16_t *slot = base + (size_t)j * slot_words, *dcs = slot + nblk * 64;
            CMYK_HIP(hipMemcpyAsync(a3.coefs + (size_t)i * nb3 * 64, slot, nb3 * 128, hipMemcpyHostToDevice, s));
            CMYK_HIP(hipMemcpyAsync(ak.coefs + (size_t)i * nbk * 64, slot + nb3 * 64, nbk * 128, hipMemcpyHostToDevice, s));
            CMYK_HIP(hipMemcpyAsync(a3.dcs + (size_t)i * nb3, dcs, nb3 * 2, hipMemcpyHostToDevice, s));
            CMYK_HIP(hipMemcpyAsync(ak.dcs + (size_t)i * nbk, dcs + nb3, nbk * 2, hipMemcpyHostToDevice, s));
        }
        if (!ev.ev[half]) CMYK_HIP(hipEventCreateWithFlags(&ev.ev[half], hipEventDisableTiming));
        CMYK_HIP(hipEventRecord(ev.ev[half], s));
    }
    if (!any_ok(status, n)) return IPX_OK;
    CMYK_HIP(hipMemcpyAsync(d_valid, valid.data(), (size_t)n, hipMemcpyHostToDevice, s));
    CMYK_HIP(hipMemcpyAsync(d_kind, kind.data(), (size_t)n, hipMemcpyHostToDevice, s));
    CMYK_HIP(hipMemcpyAsync(d_tab3, tab3.data(), sizeof(JpegDecTables) * n, hipMemcpyHostToDevice, s));
    CMYK_HIP(hipMemcpyAsync(d_tabk, tabk.data(), sizeof(JpegDecTables) * n, hipMemcpyHostToDevice, s));
    CMYK_HIP(launch_jpeg_idct(a3, p3, s));
    CMYK_HIP(launch_jpeg_idct(ak, pk, s));
    CmykAsmArgs g{};
    g.y = p3.y; g.cb = p3.cb; g.cr = p3.cr; g.k = pk.y; g.ystride = p3.ystride; g.cstride = p3.cstride; g.y_fs = p3.y_fs; g.c_fs = p3.c_fs;
    g.pix = out.pix; g.stride = out.stride; g.fs = out.frame_stride; g.w = R.w; g.h = R.h; g.half = R.h0 == 2; g.kind = d_kind;
    for (int k = 1; k <= 2; k++)
        if (std::find(kind.begin(), kind.end(), (uint8_t)k) != kind.end()) CMYK_HIP(launch_cmyk_assemble(g, n, k == 2, s));
    CMYK_HIP(hipStreamSynchronize(s));
    *frames = out;
    *owner = own.release();
    return IPX_OK;
}

extern "C" {

int ipx_jpeg_decode_batch_cmyk(ipx_ctx *ctx, void *stream, const ipx_bytes *jpegs, int n, int *w, int *h, ipx_cmyk_batch *frames, int *status,
                               ipx_jpeg_planes **owner) try
{
    IPX_ENTER(ctx);
    if (!jpegs || n < 0 || !w || !h || !frames || !status || !owner) { set_error("ipx_jpeg_decode_batch_cmyk: bad argument"); return IPX_ERR_INVALID; }
    *owner = nullptr;
    memset(frames, 0, sizeof *frames);
    if (n == 0) return IPX_OK;
    if (n > 65535) { set_error("ipx_jpeg_decode_batch_cmyk: at most 65535 files per call"); return IPX_ERR_UNSUPPORTED; }
    return jpeg_decode_cmyk_files(ctx, stream ? (hipStream_t)stream : ctx->stream, jpegs, n, w, h, 0, frames, status, owner);
}
IPX_CATCH_STATUS

int ipx_jpeg_cmyk_files(ipx_ctx *ctx, long long *files)
{
    clear_error();
    if (!ctx || !files) { set_error("ipx_jpeg_cmyk_files: bad argument"); return IPX_ERR_INVALID; }
    *files = ctx->jpeg_cmyk_files.load();
    return IPX_OK;
}

}  // extern "C"
