// ipx_internal.h -- shared declarations of libipx (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/ipx.h"
#include "ipx_jpeg_enc_mixed_plan.h"
#include "ipx_jpeg_mixed_plan.h"

namespace ipx {

// ---- error plumbing: every ABI entry returns a status, text goes to a thread-local buffer ----
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();
// Nothing may unwind through the C ABI (a cgo or ctypes caller would be terminated): every extern "C" entry that can allocate is a
// function-try-block closed by IPX_CATCH_STATUS, which maps std::bad_alloc / std::system_error to IPX_ERR_NOMEM and anything else to
// IPX_ERR_INVALID, with the text in ipx_last_error().  Call status_of_exception() only inside a catch block.
int status_of_exception() noexcept;
#define IPX_CATCH_STATUS catch (...) { return ipx::status_of_exception(); }

#define IPX_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ipx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,  \
                           __LINE__);                                                        \
            return IPX_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

// ---- frame geometry the kernels can address --------------------------------------------------------------------------
// Frames are addressed through buffer descriptors (32-bit num_records) and int byte offsets; an idle lane's offset is kOOB =
// 0x7fffffff, which has to lie beyond every frame.  So a frame's span (h-1)*stride + w*bpp must stay below 2 GiB, and a side
// below 65536 (grid dimensions; also jpeg.Encode's own limit).  A 32 MiB PNG upload (domain/task.go:55) can decode past that:
// such frames get IPX_ERR_UNSUPPORTED and stay on the reference's CPU path -- never wrapped offsets.
constexpr long long kMaxFrameSpan = 0x7fff0000LL;
constexpr int kMaxFrameSide = 65535;
inline bool frame_span_ok(long long w, long long h, long long stride, int bpp)
{
    if (w > kMaxFrameSide || h > kMaxFrameSide) return false;
    return w <= 0 || h <= 0 || (h - 1) * stride + w * bpp <= kMaxFrameSpan;
}

// ---- image.Rectangle arithmetic (image/geom.go semantics) ------------------------------------
struct Rect {
    int x0, y0, x1, y1;
    int dx() const { return x1 - x0; }
    int dy() const { return y1 - y0; }
    bool empty() const { return x0 >= x1 || y0 >= y1; }
    Rect shifted(int ox, int oy) const { return Rect{x0 + ox, y0 + oy, x1 + ox, y1 + oy}; }
    Rect intersect(const Rect &s) const;
};
inline Rect to_rect(const ipx_rect &r) { return Rect{r.x0, r.y0, r.x1, r.y1}; }

// image/draw.clip for DrawMask: narrows r to dst, to the source placed by sp and, when mask_w >= 0,
// to the mask placed by mp; advances sp / mp by the amount r.Min moved.  has_src false = Uniform.
bool draw_clip(Rect &r, int dw, int dh, bool has_src, int sw, int sh, int &spx, int &spy,
               bool has_mask, int mw, int mh, int &mpx, int &mpy);

// ---- the Go image types a batch of source frames can have ---------------------------------------------------------------------
// The one enumeration of source types (BatchSrc in ipx_runtime_internal.h).  The deep types keep the order of IPX_DEEP_*.
enum SrcType { kSrcRGBA, kSrcNRGBA, kSrcGray, kSrcPaletted, kSrcYCbCr, kSrcNRGBA64, kSrcRGBA64, kSrcGray16, kSrcCMYK, kSrcTypes };
// bytes per pixel of plane 0 (Pix, the index plane, Y)
inline int src_bpp(int type) { static const int b[kSrcTypes] = {4, 4, 1, 1, 1, 8, 8, 2, 4}; return b[type]; }
// the ABI's own numberings -> SrcType; -1 for a value that names no source of pixels
inline int src_of_deep(int k) { return k >= IPX_DEEP_NRGBA64 && k <= IPX_DEEP_CMYK ? kSrcNRGBA64 + k : -1; }
inline int src_of_png(int k)
{
    static const int t[] = {kSrcGray, kSrcNRGBA, kSrcRGBA, kSrcPaletted, kSrcGray16, kSrcRGBA64, kSrcNRGBA64};      // IPX_PNG_*
    return k >= 0 && k < 7 ? t[k] : -1;
}
inline int src_of_job(int k)
{
    static const int t[] = {kSrcRGBA, -1, kSrcNRGBA, kSrcGray, kSrcNRGBA64, kSrcRGBA64, kSrcGray16, kSrcCMYK};      // IPX_JOB_*
    return k >= 0 && k < 8 ? t[k] : -1;
}
// size of the chroma planes of a w x h *image.YCbCr (image.NewYCbCr)
inline void chroma_size(int ratio, int w, int h, int *cw, int *ch)
{
    *cw = ratio == IPX_YCBCR_422 || ratio == IPX_YCBCR_420 ? (w + 1) / 2 : ratio == IPX_YCBCR_411 || ratio == IPX_YCBCR_410 ? (w + 3) / 4 : w;
    *ch = ratio == IPX_YCBCR_420 || ratio == IPX_YCBCR_440 || ratio == IPX_YCBCR_410 ? (h + 1) / 2 : h;
}
// a ratio the *image.YCbCr entries take (IPX_GRAY has entries of its own)
inline bool ycbcr_ratio_ok(int ratio) { return (ratio >= IPX_YCBCR_444 && ratio <= IPX_YCBCR_440) || ratio == IPX_YCBCR_411 || ratio == IPX_YCBCR_410; }
// the shifts of COffset: Cb, Cr of pixel (x, y) sit at (x >> hs, y >> vs)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int ycbcr_hshift(int ratio) { return ratio == IPX_YCBCR_422 || ratio == IPX_YCBCR_420 ? 1 : ratio == IPX_YCBCR_411 || ratio == IPX_YCBCR_410 ? 2 : 0; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int ycbcr_vshift(int ratio) { return ratio == IPX_YCBCR_420 || ratio == IPX_YCBCR_440 || ratio == IPX_YCBCR_410 ? 1 : 0; }
// the ratio of a three-component frame whose luma factors are (h0, v0) with 1x1 chroma (makeImg)
inline int ycbcr_ratio_of(int h0, int v0)
{
    return h0 == 4 ? (v0 == 1 ? IPX_YCBCR_411 : IPX_YCBCR_410) : h0 == 1 ? (v0 == 1 ? IPX_YCBCR_444 : IPX_YCBCR_440) : (v0 == 1 ? IPX_YCBCR_422 : IPX_YCBCR_420);
}

// ---- kernel launchers (ipx_kernels.hip) --------------------------------------------------------
// how the pixels of a source image in HBM are laid out (the tap kinds built on them: ipx_ks.h)
enum { IPX_SRC_RGBA = 0, IPX_SRC_NRGBA = 1, IPX_SRC_YCBCR = 2,
       IPX_SRC_TAP64 = 3 /* At(x, y).RGBA() as four little-endian uint16 per pixel: the deep source types after deep_expand_kernel */ };
hipError_t launch_opaque_scan(const uint8_t *src, int sw, int sh, int sstride, int *flag,
                              hipStream_t s);
hipError_t launch_opaque_scan_tap64(const uint8_t *src, int sw, int sh, int sstride, int *flag, hipStream_t s);
hipError_t launch_draw(uint8_t *dst, int dstride, const uint8_t *src, int sstride, int w, int h,
                       int op, hipStream_t s);
hipError_t launch_draw_nrgba(uint8_t *dst, int dstride, const uint8_t *src, int sstride, int w, int h, int op,
                             hipStream_t s, int nframes = 1, size_t dst_fs = 0, size_t src_fs = 0);
// deep source types (ipx.h IPX_DEEP_*): Go's Pix -> frames of 16-bit taps (dst rows w * 8 bytes apart), and taps -> RGBA8 (drawRGBA / drawCMYK)
hipError_t launch_deep_expand(uint8_t *dst, size_t dst_fs, const uint8_t *src, int sstride, size_t src_fs, int kind, int w, int h, int nframes, hipStream_t s);
hipError_t launch_draw_tap64(uint8_t *dst, int dstride, const uint8_t *src, int sstride, int w, int h, int op, hipStream_t s,
                             int nframes = 1, size_t dst_fs = 0, size_t src_fs = 0);
hipError_t launch_draw_ycbcr(uint8_t *dst, int dstride, const uint8_t *y, int ystride, const uint8_t *cb,
                             const uint8_t *cr, int cstride, int ratio, int spx, int spy, int w, int h, hipStream_t s,
                             int nframes = 1, size_t dst_fs = 0, size_t y_fs = 0, size_t c_fs = 0);

struct DevGlyph {           // one clipped DrawMask call, masks resident in HBM
    const uint8_t *mask;    // points at mask(mpx, mpy) after clipping
    int mstride;
    int x0, y0, x1, y1;     // clipped destination rectangle
};
constexpr int kMaxGlyphs = 256;
hipError_t launch_stream_copy(void *dst, const void *src, size_t bytes, hipStream_t s);   // the box's streaming ceiling (bench.py)
hipError_t launch_composite(uint8_t *dst, int dstride, size_t frame_stride, int nframes,
                            const DevGlyph *glyphs_dev, int n, Rect bbox, uint32_t sr, uint32_t sg,
                            uint32_t sb, uint32_t sa, hipStream_t s);
// one text of a text set (ipx_textset): its clipped glyphs glyphs[first .. first + n) of the set's one table, their bounding box (empty:
// nothing to draw) and the colour as launch_composite takes it (c * 0x101)
struct DevText {
    int first, n;
    Rect bbox;
    uint16_t col[4];
};
hipError_t launch_composite_texts(uint8_t *dst, int dstride, size_t frame_stride, int nframes, const DevText *texts_dev,
                                  const DevGlyph *glyphs_dev, const int *map_dev, int first, int bw, int bh, hipStream_t s);

hipError_t launch_gray_expand(uint8_t *dst, size_t dst_fs, const uint8_t *src, int sstride, size_t src_fs, int w, int h, int n, hipStream_t s);
hipError_t launch_palette_expand(uint8_t *dst, size_t dst_fs, const uint8_t *src, int sstride, size_t src_fs, const uint8_t *palettes, int w,
                                 int h, int n, hipStream_t s);

// Per kernel instantiation and process: the dynamic-LDS limit is raised once (it only has to be at least what a launch asks for) and the
// occupancy is cached per LDS size.  These are properties of the loaded function, not of the calling thread; done per thread, every
// short-lived worker thread repeated hipFuncSetAttribute / hipOccupancy... in the middle of other threads' launches.
struct KernelLaunchCache {
    std::mutex mu;
    size_t lds_max = 0;
    std::map<size_t, int> resident;
    bool said = false;
    hipError_t prepare(const void *fn, int threads, size_t lds, int *res)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (lds > lds_max) {
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            lds_max = lds;
        }
        if (res) {
            auto it = resident.find(lds);
            if (it == resident.end()) {
                int n = 0;
                hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds);
                if (e != hipSuccess) return e;
                it = resident.emplace(lds, n > 1 ? n : 1).first;
            }
            *res = it->second;
        }
        return hipSuccess;
    }
    bool first_report() { std::lock_guard<std::mutex> lk(mu); const bool f = !said; said = true; return f; }
};


// ---- jpeg.Encode: transform on the GPU (ipx_jpeg.hip), tables / headers / entropy coder on the host ----
struct JpegTables {
    uint8_t quant[2][64];     // zig-zag order, as DQT carries them (e.quant of writer.go)
    uint16_t div8[2][64];     // 8 * quant, natural order: the divisor of writeBlock's div()
    uint32_t recip[2][64];    // ceil(2^32 / div8): floor(n / div8) == mulhi(n, recip) for n < 2^20
};
void jpeg_tables(int quality, JpegTables *t);
struct JpegArgs {
    const uint8_t *src; size_t frame_stride; int stride, w, h;
    int aligned16;            // base, row stride and frame stride are multiples of 16
    int16_t *coefs; int mcus_per_frame;
    // optional (all three or none): the AC part of every block's Huffman-coded length, and the quantised DC terms as a dense array --
    // computed while the block sits in LDS, so that no separate pass has to read the coefficients back to size the scan
    const uint32_t *huff;     // jpeg_huff_packed: four tables of 256 (len << 16 | code)
    uint32_t *aclen;          // [frame][block] bits of the AC symbols (ZRL, EOB included)
    int16_t *dcq;             // [frame][block]
    uint32_t recip[2][64];
    uint16_t div8[2][64];
};
hipError_t launch_jpeg_fdct(const JpegArgs &a, int n, hipStream_t s);
// the transform of n frames of any sizes in one launch (ipx_jpeg_enc_mixed_plan.h): of `a` the tables and the three dense arrays are read
// (huff, aclen, dcq: required), the frame's own fields come from its record; wgs = JpegEncTotals::fdct_wgs
hipError_t launch_jpeg_fdct_mixed(const JpegArgs &a, const JpegEncFrame *frames, int n, unsigned long long wgs, hipStream_t s);


// ---- image.Decode for baseline JPEGs (ipx_jpeg_dec_host.cpp parses, ipx_jpeg_dec.hip decodes) ------------
struct JpegDecInfo {
    int w, h, h0, v0, ratio, ri, ncomp;
    int host_scans;            // 1: not one baseline scan the GPU's Huffman kernels take (progressive, several scans, table ids above 1):
                               // jpeg_host_decode walks the scans on the host, the coefficients go up, the GPU does the rest
    int progressive;           // SOF2 (reconstructProgressiveImage's rule for blocks outside the image applies)
    int gpu_scans;             // host_scans files only, under IPX_JPEG_PROG_GPU=1: the marker pre-pass was clean (jpeg_prog_prepass), the
                               // scans are walked by jpeg_prog_kernel instead of jpeg_host_decode
    uint8_t td[3], ta[3];      // kernel table slots of the three components: 0,1 = DC tables, 2,3 = AC tables
    size_t scan_off, scan_len; // entropy-coded data within the file
};
struct JpegDecTables {         // per image, as the kernels read them
    uint16_t lut[4][256];      // first level: length << 8 | symbol for codes of at most 8 bits, else 0
    int32_t maxcode[4][18];    // by code length; -1 = no code of that length
    int32_t valoff[4][18];     // symbol index = valoff[len] + code
    uint8_t vals[4][256];
    uint16_t qnat[3][64];      // quantiser per component, natural order
    uint32_t bound[4][8];      // for lengths 9..16: first 16-bit left-aligned value NOT covered by codes of at most that length
};
// one independently decodable piece of a scan: the whole scan, or one restart interval of it (DC predictions and the bit
// reader start afresh after every RSTn, so intervals decode in parallel)
struct JpegDecImage {
    unsigned long long scan_off; uint32_t scan_len, img, first_mcu, n_mcu;
    uint8_t td[3], ta[3], valid, pad;   // pad: bytes to skip at the start (pieces are read in aligned 16-byte chunks)
    uint8_t strict_end, rsv[3];         // a restart interval must end exactly at its RSTn marker (Go would resynchronise: not ours to guess)
    unsigned long long uoff;            // where the piece's unstuffed copy lives (launch_jpeg_pieces), 16-byte aligned, regions do not overlap
    uint32_t tab_img, rsv2;             // the image whose Huffman tables this piece decodes with (the first of the batch with identical tables)
};
struct JpegDecArgs {
    const uint8_t *blob; const JpegDecImage *img; const JpegDecTables *tab;
    int16_t *coefs; int *status;
    int16_t *dcs;                    // [n][nblk] the DC coefficient of every block (coefs[...][0] stays zero)
    int n, mxx, myy, h0, v0, nblk;   // n = images
    int w, h;                        // the batch's frame size (progressive images reconstruct only blocks that hold image pixels)
    int bpm, ybl;                    // blocks per MCU and how many of them are luma (Gray: 1, 1; 4:1:1: 6, 4 in one row; 4:1:0: 10, 8 as 2 rows of 4)
    int nitems;                      // pieces to decode (>= images)
    int shared_tables, first_valid;   // every valid image carries the Huffman tables of image first_valid
    const JpegMixGeom *geom;          // a mixed-size class (ipx_jpeg_mixed_plan.h): one record per image replaces mxx, myy, nblk, w, h and the
                                      // planes' strides, which are then unset; NULL: the uniform kernels, which never read it
    unsigned mix_wgs;                 // geom != NULL: workgroups of the one-dimensional IDCT launch
};
// the per-image status word of the decoder kernels: 0, or a negative key whose low three bits are -IPX_ERR_* and whose upper bits order
// the reporting pieces so that atomicMin keeps the verdict of the piece a sequential decoder would have reached first
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int jpeg_status_key(uint32_t first_mcu, int status) { return -(int)(((0x3ffffffu - (first_mcu & 0x3ffffffu)) << 3) | (uint32_t)(-status)); }
// a DC value beyond int16: Go keeps int32 and decodes such a (damaged) file, this pipeline cannot represent it -> UNSUPPORTED, with the
// lowest priority: any real decoding error elsewhere in the file, which Go fails on as well, wins
constexpr uint32_t kJpegStatusLast = 0x3ffffffu;
inline int jpeg_status_of(int key) { return key >= 0 ? 0 : -(int)((uint32_t)(-key) & 7u); }
struct JpegPlanes { uint8_t *y, *cb, *cr; int ystride, cstride; size_t y_fs, c_fs; const uint8_t *valid; /* per image: bit 0 decodable, bit 1 progressive, bits 2..4 component 0..2 coded by non-interleaved sequential scans only (jpeg_host_decode) */ };
// Huffman decoding parallel inside a scan (ipx_jpeg_dec_par.hip): per image and per 1 KiB sub-sequence of its scan
struct JpegParImage { unsigned long long scan_off; uint32_t scan_len, img, nsub; size_t sub_off; uint8_t td[3], ta[3], pad[2]; };
struct JpegParArgs {
    const uint8_t *blob; const JpegDecTables *tab; const JpegParImage *img;
    uint8_t *ublob;                        // the scans without stuffing, same offsets as blob, zero filled
    int nimg, max_nsub, bpm, ybl, nblk;
    int stage_rows;                        // 1: the workgroup's 64 sub-sequences are staged in LDS (rows of sub + 4 bytes: small batches); 0: read through L1 / L2; 2: diagnostic, see CoefSink::drop
    int sub;                               // bytes of scan per sub-sequence: 128, 256, 512 or 1024 (jpeg_par_sub_bytes(): the largest)
    uint32_t *stuffed;                     // [nimg][max_nsub] stuffed zeros before each sub-sequence's chunk (after the scan)
    uint32_t *scan_end, *ulen;             // per image: first marker in the stuffed scan; bytes of the unstuffed scan
    unsigned long long *entry, *exit_a, *exit_b;
    unsigned long long *ck_state; uint32_t *ck_ends;   // per sub-sequence, jpeg_par_checkpoints() each: state and block ends at the checkpoints
    uint32_t *ends, *total_ends;           // block ends per sub-sequence (after the scan: first block index); per image total
    uint32_t *changed;
    int16_t *coefs; int *status;
    int16_t *dcs;                          // [image][nblk]: DC differences from the write pass, DC values after par_dc_kernel
    const JpegMixGeom *geom;               // as JpegDecArgs::geom, indexed by JpegParImage::img: the block count and the slot base per image
};
int jpeg_par_sub_bytes();
int jpeg_par_checkpoints();
hipError_t launch_par_count(const JpegParArgs &a, hipStream_t s);
hipError_t launch_par_unstuff(const JpegParArgs &a, hipStream_t s);
hipError_t launch_par_sync(const JpegParArgs &a, int round, hipStream_t s);
hipError_t launch_par_write(const JpegParArgs &a, hipStream_t s);
hipError_t launch_par_dc(const JpegParArgs &a, hipStream_t s);
// s411 (IPX_JPEG_411=1): three-component frames with luma factors (4,1) and (4,2) and 1x1 chroma are taken too (4:1:1, 4:1:0)
int jpeg_parse(const uint8_t *d, size_t len, JpegDecInfo *info, JpegDecTables *tab, bool cmyk = false, bool s411 = false);
int jpeg_host_decode(const uint8_t *d, size_t len, JpegDecInfo *info, int16_t *coefs, int16_t *dcs, size_t nblk, uint16_t qnat[3][64],
                     bool *progressive, bool s411 = false, int *alone = nullptr);
// *alone (sequential files of several components): bit c set when component c was coded by non-interleaved scans only.  Such a scan
// carries no data for the blocks (bx, by) of the component's own grid with bx * 8 >= w or by * 8 >= h, and Go, which reconstructs a
// sequential block when it decodes it, never writes them: they stay zero in the planes (JpegPlanes::valid bits 2..4).
// Four-component files (IPX_JPEG_CMYK=1; ipx_jpeg_dec_cmyk.hip): every scan on the host, into TWO coefficient sets the IDCT kernel reads as
// they are -- components 0..2 as a three-component image of the file's sampling (mxx * myy * (ybl + 2) blocks in MCU order), then
// component 3 as a Gray image of component 0's block grid, raster by block ((h0 * mxx) * (v0 * myy) blocks).  nblk is the sum; coefs, dcs
// and the progressive flag as for jpeg_host_decode; qnat[3] is component 3's quantiser; *transform the Adobe APP14 transform byte (a
// file without a valid APP14 segment is IPX_ERR_UNSUPPORTED: Go's "unknown color model").
int jpeg_host_decode4(const uint8_t *d, size_t len, JpegDecInfo *info, int16_t *coefs, int16_t *dcs, size_t nblk, uint16_t qnat[4][64],
                      bool *progressive, int *transform);
// ---- progressive scans walked on the GPU (IPX_JPEG_PROG_GPU=1): the scan program of a file (jpeg_prog_prepass in ipx_jpeg_dec_prog.cpp)
// and the kernel that runs it (ipx_jpeg_dec_scans.hip) ----
constexpr int IPX_JPEG_PROG_MAX_SCANS = 64;
// one DHT definition in the device format: the 9-bit first level and the per-length bounds of the host decoder's Huff
struct JpegProgHuff {
    uint16_t look[512];                            // length << 8 | symbol, 0: no code of at most 9 bits
    int32_t mincode[17], maxcode[17], valptr[17];  // by code length 1..16; maxcode -1: no code of that length
    uint8_t vals[256];
    int32_t ncodes;
};
static_assert(sizeof(JpegProgHuff) % 16 == 0, "copied to LDS in 16-byte units");
struct JpegProgScan {
    uint32_t off, len;           // the READABLE entropy data within the file: up to the first 0xff that 0x00 does not follow
    uint8_t ns, ss, se, ah, al;
    uint8_t comp[3];             // component index per slot
    uint16_t dc_def[3], ac_def[3];   // the table definitions in effect (indices into the file's definitions, of which there are at most
                                     // IPX_JPEG_PROG_MAX_SCANS * 3: one per table a scan decodes with); 0xffff: not used by this scan
    uint32_t rsv;
};
struct JpegProgFile { unsigned long long blob_off; uint32_t img, nscans, scan0, def0; };   // scan0 / def0: first entry in the batch's arrays
struct JpegProgPlan {            // what the pre-pass leaves for one file
    std::vector<JpegProgScan> scans;
    std::vector<JpegProgHuff> defs;
};
struct JpegProgArgs {
    const uint8_t *blob; const JpegProgFile *files; const JpegProgScan *scans; const JpegProgHuff *defs;
    int16_t *coefs, *dcs; int *status;
    int nfiles, mxx, myy, h0, v0, nblk, w, h, bpm, ybl;
};
// the status word of a file whose walk met a coefficient that int16 truncates to zero: the host decoder's non-zero mask and the
// coefficients disagree from there on, so the driver asks jpeg_host_decode for this (damaged) file's verdict
constexpr uint32_t kJpegProgHostVerdict = 0x3fffffeu;
// 1: SOF2, and Decoder::run's marker loop with the entropy data skipped reaches EOI with every SOS header valid, every table a scan
// decodes with defined, no restart interval and at most IPX_JPEG_PROG_MAX_SCANS scans; then *plan and qnat (the FINAL tables) are filled
bool jpeg_prog_prepass(const uint8_t *d, size_t len, const JpegDecInfo &info, JpegProgPlan *plan, uint16_t qnat[3][64]);
hipError_t launch_jpeg_prog(const JpegProgArgs &a, hipStream_t s);
int jpeg_prog_lds_bytes();

// The host plan of a batch decode (jpeg_plan_batch in ipx_jpeg_dec_host.cpp; no device call): the files parsed, the batch's geometry
// chosen, the baseline scans cut into pieces (grouped by table class) and parallel images, all placed in one blob.
struct JpegPlanOptions {
    int want_w, want_h;        // the size asked for; want_w <= 0: the first parsed file's
    bool use_par;              // IPX_JPEG_PAR: long scans without restart markers go to the parallel decoder
    int forced_sub, max_sub;   // IPX_JPEG_PAR_SUB: 128 .. 1024 fixes the sub-sequence size, else the batch chooses; jpeg_par_sub_bytes()
    bool prog_gpu = false;     // IPX_JPEG_PROG_GPU=1: progressive files with a clean pre-pass are walked on the GPU
    bool s411 = false;         // IPX_JPEG_411=1: 4:1:1 and 4:1:0 files are taken (never by the GPU scan walk)
    bool mixed = false;        // every parsed file of the call is taken whatever its size (want_w, want_h unused); the caller passes files
                               // of ONE sampling class (jpeg_plan_place)
};
struct JpegBatchPlan {
    std::vector<JpegDecInfo> info;
    std::vector<JpegDecTables> tabs;
    std::vector<uint8_t> valid;       // per file: bit 0 decodable (final only once the host-decoded files are through), bit 1 progressive
    std::vector<size_t> blob_off;     // where a GPU-decoded file's scan lies in the blob
    std::vector<int> hslot;           // host-decoded files (info.host_scans without gpu_scans) numbered in file order, -1 for the others
    std::vector<int> gfiles;          // files whose scans jpeg_prog_kernel walks (info.gpu_scans), their whole bytes in the blob at blob_off
    std::vector<JpegProgPlan> prog;   // per file; filled for gfiles only
    std::vector<uint8_t> route;       // per file: the IPX_JPEG_ROUTE_* its decoder is reached by; 0xff: refused before (ipx_jpeg_decode_counts)
    std::vector<JpegDecImage> items;  // pieces by table class, every class but the last padded to whole groups of 64 (padding: valid == 0)
    std::vector<JpegParImage> par;
    std::vector<std::vector<uint32_t>> marks;   // per file: the RSTn markers of a baseline scan, as offsets into it (jpeg_plan_parse)
    int ref = -1, par_sub = 0, nhost = 0;   // ref: the file that sets the batch's geometry; -1: nothing decodable
    size_t blob_bytes = 0, piece_ubytes = 0;
    double parse_ms = 0;              // for the IPX_DEBUG timing line
};
// status[i]: the parser's verdict, UNSUPPORTED outside the batch's geometry.  Returns the status of an exception on a preparation thread.
int jpeg_plan_batch(const ipx_bytes *files, int n, const JpegPlanOptions &opt, int *status, JpegBatchPlan *plan);
// its two halves: every file parsed (info, tabs, marks, prog; status[i] the parser's verdict), then the geometry chosen and the scans
// placed.  A mixed-size call parses once and places once per sampling class, on that class's files moved into a plan of their own.
int jpeg_plan_parse(const ipx_bytes *files, int n, const JpegPlanOptions &opt, int *status, JpegBatchPlan *plan);
void jpeg_plan_place(const ipx_bytes *files, int n, const JpegPlanOptions &opt, int *status, JpegBatchPlan *plan);
bool jpeg_same_tables(const JpegDecTables &x, const JpegDecTables &y);     // the Huffman tables (not the quantisers)
hipError_t launch_jpeg_huff(const JpegDecArgs &a, hipStream_t s);
// the same pieces through the word-wise reader of the parallel decoder: unstuff each piece into ublob (+ its length into ulen), then one
// decode pass -- the state at the start of a piece is known, so nothing is speculative.  The 64 pieces of a workgroup share one set
// of tables (img[64 * k].tab_img): the host groups the pieces by table set and pads each group to a multiple of 64.
hipError_t launch_jpeg_pieces(const JpegDecArgs &a, uint8_t *ublob, uint32_t *ulen, hipStream_t s);
hipError_t launch_jpeg_idct(const JpegDecArgs &a, const JpegPlanes &pl, hipStream_t s);

void jpeg_write_stream(const int16_t *coefs, int w, int h, const JpegTables &t, std::vector<uint8_t> *out);
void jpeg_write_header(int w, int h, const JpegTables &t, std::vector<uint8_t> *out);
void jpeg_huff_packed(uint32_t out[1024]);
// the entropy coder on the GPU (ipx_jpeg_entropy.hip)
hipError_t launch_jpeg_len(const int16_t *coefs, int nblk, int n, const uint32_t *tables, uint32_t *len, hipStream_t s);
// len[b] += bits of block b's DC symbol (difference to the previous block of its component), from the dense DC array of the transform kernel
hipError_t launch_jpeg_dclen(const int16_t *dcq, int nblk, int n, const uint32_t *tables, uint32_t *len, hipStream_t s);
hipError_t launch_jpeg_bits(const int16_t *coefs, int nblk, int n, const uint32_t *tables, const uint32_t *off,
                            const unsigned long long *total_bits, const unsigned long long *ubase, uint8_t *ustream, hipStream_t s);
hipError_t launch_scan(uint32_t *v, int per_frame, int n, uint32_t *total, hipStream_t s);
// the same scan with the frame's sum in 64 bits (the offsets still wrap at 2^32: the caller refuses a frame whose sum reaches that)
hipError_t launch_scan64(uint32_t *v, int per_frame, int n, unsigned long long *total, hipStream_t s);
int jpeg_chunk_bytes();
hipError_t launch_jpeg_ffcount(const uint8_t *ustream, const unsigned long long *ubase, const uint32_t *ubytes, int max_chunks, int n,
                               uint32_t *ffcount, hipStream_t s);
hipError_t launch_jpeg_stuff(const uint8_t *ustream, const unsigned long long *ubase, const uint32_t *ubytes, int max_chunks, int n,
                             const uint32_t *ffoff, const uint8_t *header, int hdr_len, const unsigned long long *obase, uint8_t *ostream,
                             hipStream_t s);
// The same stages for n frames of any sizes, one launch each (ipx_jpeg_enc_mixed_plan.h): a frame's geometry, bases and first workgroups
// come from its record, len / dcq / ffcount are the dense arrays the records index, total_bits and fftotal are [n].  header: one
// jpeg_write_header output for the call; the stuffing pass writes each frame's own height and width over its bytes at kJpegSofDims.
hipError_t launch_jpeg_dclen_mixed(const JpegEncFrame *frames, int n, unsigned long long wgs, const int16_t *dcq, const uint32_t *tables,
                                   uint32_t *len, hipStream_t s);
hipError_t launch_jpeg_bits_mixed(const JpegEncFrame *frames, int n, unsigned long long wgs, const uint32_t *tables, const uint32_t *off,
                                  const unsigned long long *total_bits, uint8_t *ustream, hipStream_t s);
hipError_t launch_scan_mixed_len(const JpegEncFrame *frames, int n, uint32_t *len, unsigned long long *total_bits, hipStream_t s);
hipError_t launch_scan_mixed_ff(const JpegEncFrame *frames, int n, uint32_t *ffcount, uint32_t *fftotal, hipStream_t s);
hipError_t launch_jpeg_ffcount_mixed(const JpegEncFrame *frames, int n, unsigned long long wgs, const uint8_t *ustream, uint32_t *ffcount,
                                     hipStream_t s);
hipError_t launch_jpeg_stuff_mixed(const JpegEncFrame *frames, int n, unsigned long long wgs, const uint8_t *ustream, const uint32_t *ffoff,
                                   const uint8_t *header, int hdr_len, uint8_t *ostream, hipStream_t s);
}  // namespace ipx
