/*
 * ipx.h -- C ABI of libipx, the MI355X (gfx950) pixel worker for ImageProcessor.
 *
 * This is the drop-in boundary for ONE path of the reference: the per-pixel work of
 * internal/worker -> internal/usecase/processor.  The reference has no
 * FFI today (dockerfile:12 builds with CGO_ENABLED=0); the seam is three private Go helpers
 * plus the operator method set.  Every entry point below names the reference code it replaces.
 * Plain pointers and sizes only; all functions are callable from any OS thread (goroutines
 * migrate), return an ipx_status (0 = ok, negative = error) and never abort or throw.
 * INTEGRATION.md holds the cgo binding that goes with this header.
 *
 * Pixel format everywhere: 8-bit premultiplied RGBA, as Go's image.RGBA (Pix, Stride, Rect
 * with Min = (0,0)).  Strides are in bytes.
 */
#ifndef IPX_H
#define IPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPX_ABI_VERSION 1

typedef struct ipx_ctx ipx_ctx;           /* one per worker process and GPU            */
typedef struct ipx_glyphset ipx_glyphset; /* rasterised watermark text resident in HBM */
typedef struct ipx_plan ipx_plan;         /* fused resize+thumbnail+watermark geometry */

typedef enum {
    IPX_OK = 0,
    IPX_ERR_INVALID = -1,     /* bad argument (the Go side returns an error, image_processor.go:66-75) */
    IPX_ERR_NOMEM = -2,       /* host or device allocation failed                       */
    IPX_ERR_HIP = -3,         /* a HIP call failed; text in ipx_last_error()            */
    IPX_ERR_UNSUPPORTED = -4, /* valid in the reference but outside this library's path */
    IPX_ERR_NODEVICE = -5     /* no gfx950 device visible                               */
} ipx_status;

/* draw.Op of image/draw and x/image/draw (resize.go:123 passes xdraw.Over, watermark.go:92 draw.Src) */
enum { IPX_OP_OVER = 0, IPX_OP_SRC = 1 };

/* image.Rectangle: [x0,x1) x [y0,y1) */
typedef struct { int32_t x0, y0, x1, y1; } ipx_rect;

/* One draw.DrawMask call of freetype.Context.DrawString (watermark.go:151): an *image.Alpha
 * mask with bounds (0,0)-(mw,mh), the destination rectangle dr and the mask point mp that is
 * aligned with dr.Min.  Clipping against the frame and the mask is done by the library exactly
 * as image/draw does.  Glyphs are applied in array order; overlapping boxes are NOT merged. */
typedef struct {
    const uint8_t *mask;
    int32_t mw, mh, mstride;
    ipx_rect dr;
    int32_t mpx, mpy;
} ipx_glyph;

typedef struct {
    int32_t device;        /* HIP device ordinal; -1 = LOCAL_RANK / 0                          */
    int32_t lanes;         /* staging lanes (a stream + device scratch each); 0 = 5: a host batch pipelines its chunks over four
                              (the reference's WORKER_CONCURRENCY is 3, .env.example:38, worker.go:90; a compressed-in /
                              compressed-out batch measured best in four parts) and one stays free, so that a single-frame call is
                              served while a batch runs */
    size_t lane_bytes;     /* initial pinned+device staging per lane; grows on demand; 0 = 64 MiB */
} ipx_config;

/* ---- lifetime ----------------------------------------------------------------------------- */

/* Replaces processor.NewImageProcessor (image_processor.go:29) as the owner of per-process state. */
int ipx_create(const ipx_config *cfg, ipx_ctx **out);
void ipx_destroy(ipx_ctx *ctx);
/* Thread-local text of the last failure on the calling thread ("" if none). */
const char *ipx_last_error(void);
int ipx_abi_version(void);
/* Number of gfx950 devices visible; a negative ipx_status on failure. */
int ipx_device_count(void);

/* Whether a frame of w x h pixels with this row stride can go to the GPU path at all: the kernels address a frame through 32-bit
 * buffer descriptors, so (h-1)*stride + w*bytes_per_pixel must stay below 2 GiB and each side below 65536.  IPX_OK, or
 * IPX_ERR_UNSUPPORTED -- the answer every plan / per-operation entry gives for such a frame; the worker keeps its CPU path for it
 * (a 32 MiB PNG upload, domain/task.go:55, can decode past 23170 x 23170).  Host only. */
int ipx_frame_supported(int w, int h, long long stride, int bytes_per_pixel);

/* ---- geometry and parameter rules (host only, no GPU needed) ------------------------------- */

/* resize.go:61-75: aspect-fit in float64 with truncation, or (w,h) as given. */
int ipx_resize_dims(int ow, int oh, int w, int h, int keep_aspect, int *nw, int *nh);
/* thumbnail.go:48-65 (short side = size) and :114-127 (centre square crop). */
int ipx_thumb_geometry(int ow, int oh, int size, int crop_to_fit, ipx_rect *crop, int *nw, int *nh);
/* watermark.go:116-118: int(fixed.Int26_6(fontSize*64*1.2).Ceil()). */
int ipx_text_height_px(double font_size);
/* watermark.go:121-148: baseline point (whole pixels, as freetype.Pt) for a position string;
 * unknown strings fall to bottom-right like the reference's default arm. */
int ipx_watermark_anchor(const char *position, int w, int h, int width_px, int height_px,
                         int *px, int *py);
/* watermark.go:159-190 + :93-97: "r,g,b[,a]" -> color.RGBA bytes (NOT premultiplied, as the
 * reference builds it).  Returns IPX_OK, or 1 when the string is malformed, in which case rgba
 * holds the reference's fallback (black with alpha uint8(255*opacity)). */
int ipx_parse_color(const char *s, double opacity, uint8_t rgba[4]);

/* ---- memory the Go side may hand to asynchronous calls --------------------------------------- */

/* hipHostMalloc'd staging (cgo: wrap with unsafe.Slice; C owns it, Go must not retain it past free). */
void *ipx_host_alloc(ipx_ctx *ctx, size_t bytes);
int ipx_host_free(ipx_ctx *ctx, void *p);
void *ipx_dev_alloc(ipx_ctx *ctx, size_t bytes);
int ipx_dev_free(ipx_ctx *ctx, void *p);
/* The three copies are complete when they return (the device-to-device one runs on the context's stream and waits for it). */
int ipx_memcpy_h2d(ipx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int ipx_memcpy_d2h(ipx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int ipx_memcpy_d2d(ipx_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
/* A plain streaming copy (every workgroup copies a contiguous region of its own, 16 bytes per lane; dst, src and bytes multiples of 16),
 * asynchronous on `stream`.  Not
 * part of the path: bench.py times it on the box it runs on, because the streaming ceiling the band kernels are held against differs
 * from box to box and with where buffers land. */
int ipx_stream_copy(ipx_ctx *ctx, void *stream, void *dst_dev, const void *src_dev, size_t bytes);
/* What the host link gives pinned memory on this box: out_gbps = {up alone, down alone, up while down runs, down while up runs}, best of
 * `reps` transfers of up_bytes / down_bytes (down_bytes a multiple of 16).  Copies go in 32 MiB pieces on one stream per direction; the
 * both-at-once pair is the better of two ways down -- a copy engine, or a kernel storing into the pinned block (how the host entries
 * deliver their outputs).  Not part of the path: bench.py holds its PCIe-inclusive legs against it (`frac_of_link`). */
int ipx_link_probe(ipx_ctx *ctx, size_t up_bytes, size_t down_bytes, int reps, double out_gbps[4]);
/* Blocks until the device is idle (every stream). */
int ipx_device_sync(ipx_ctx *ctx);
/* Blocks until everything queued on `stream` (a hipStream_t, NULL = the context's stream) is done. */
int ipx_stream_sync(ipx_ctx *ctx, void *stream);

/* A stream of the caller's own on the context's device (a hipStream_t, non-blocking) for the asynchronous device-pointer entries:
 * two of them let a worker queue the next batch while the previous one runs (bench.py --mixed does exactly that).  Destroying a
 * stream waits for what is queued on it. */
void *ipx_stream_create(ipx_ctx *ctx);
int ipx_stream_destroy(ipx_ctx *ctx, void *stream);

/* ---- per-operation seam, host pointers, synchronous ------------------------------------------
 * Each call stages through a pinned lane, runs the HIP kernel and copies the result back. */

/* xdraw.BiLinear.Scale(dst, dr, src, sr, op, nil) for *image.RGBA <- *image.RGBA -- BiLinear is x/image's tent Kernel run through its
 * two-pass float64 kernel scaler (newDistrib, scaleX_RGBA, scaleY_RGBA_{Src,Over}), NOT the 2x2-tap ApproxBiLinear:
 * resizeImage (resize.go:121-125) and both Scale calls of cropAndResize (thumbnail.go:128-131; equal sizes are not simplified to a Copy).
 * dst is read as well as written when op = IPX_OP_OVER.  sr must lie inside the source
 * (IPX_ERR_UNSUPPORTED otherwise: the reference would leave its typed fast path). */
int ipx_scale_bilinear_rgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr,
                             const uint8_t *src, int sw, int sh, int sstride, ipx_rect sr, int op);
/* draw.Draw / draw.DrawMask with a nil mask, *image.RGBA <- *image.RGBA: the full-frame copy of
 * addTextWatermark (watermark.go:90-92). */
int ipx_draw_rgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r,
                   const uint8_t *src, int sw, int sh, int sstride, int spx, int spy, int op);
/* freetype.Context.DrawString's compositing (watermark.go:151): draw.DrawMask(dst, dr,
 * image.Uniform{col}, ZP, mask, mp, draw.Over) per glyph, in order, in place on dst.
 * col is the color.RGBA of watermark.go:93-97 (parseColor). */
int ipx_composite_glyphs_rgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride,
                               const ipx_glyph *glyphs, int n, const uint8_t col[4]);

/* ---- source-type variants of the same helpers ---------------------------------
 * image.Decode hands the reference *image.NRGBA for PNGs with alpha and *image.YCbCr for JPEGs
 * (image_processor.go:47); resizeImage / cropAndResize / draw.Draw take them as they are.  These
 * entries do the same on the GPU: per-tap conversion inside the kernel scaler exactly as x/image/draw
 * does it (scaleX_NRGBA, scaleX_YCbCr4xx), and image/draw's drawNRGBA{Src,Over} /
 * imageutil.DrawYCbCr for copies (the watermark's draw.Draw). */
int ipx_scale_bilinear_nrgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr,
                              const uint8_t *src, int sw, int sh, int sstride, ipx_rect sr, int op);
int ipx_draw_nrgba8(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r,
                    const uint8_t *src, int sw, int sh, int sstride, int spx, int spy, int op);

/* *image.YCbCr with Rect.Min = (0,0); ratio 0..3 numbered as image.YCbCrSubsampleRatio */
enum { IPX_YCBCR_444 = 0, IPX_YCBCR_422 = 1, IPX_YCBCR_420 = 2, IPX_YCBCR_440 = 3,
       IPX_GRAY = 4 /* *image.Gray: only the y plane is set (one-component JPEGs) */,
       /* YCbCrSubsampleRatio411 and ...410: one chroma sample per 4 x 1 and 4 x 2 luma samples (Cb, Cr at (x / 4, y) and (x / 4, y / 2);
        * planes (w + 3) / 4 wide).  NOT Go's own enum values (there 411 = 4 and 410 = 5; 4 is IPX_GRAY here): translate, do not cast.
        * The pixel entries below take them on caller-supplied planes as they are; the JPEG decoder hands them out under IPX_JPEG_411=1. */
       IPX_YCBCR_411 = 5, IPX_YCBCR_410 = 6 };
typedef struct {
    const uint8_t *y, *cb, *cr;
    int32_t ystride, cstride, w, h, ratio;
} ipx_ycbcr;
/* A YCbCr image is opaque, so the reference's Over becomes Src: there is no op argument. */
int ipx_scale_bilinear_ycbcr(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr,
                             const ipx_ycbcr *src, ipx_rect sr);
int ipx_draw_ycbcr(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r,
                   const ipx_ycbcr *src, int spx, int spy);

/* ---- same operations on frames already resident in HBM, asynchronous on `stream` -------------
 * `stream` is a hipStream_t (NULL = the context's own stream).  Pointers are device pointers.
 *
 * Layout.  Row strides may exceed the rows, and a frame may be a window of a larger one (dst / src point at the window's first pixel).
 *   dst, dstride   REQUIRED multiples of 4: the kernels store whole pixels at their natural alignment.  Anything else is
 *                  IPX_ERR_INVALID, decided on the host before any launch; nothing is written.
 *   src, sstride   any value.  When dst, dstride, src and sstride are all multiples of 16 and the width drawn is a multiple of 4,
 *                  ipx_dev_draw_rgba8 with IPX_OP_SRC copies 16 bytes per lane; everything else, including a source off a 4-byte
 *                  boundary, is read a pixel at a time: the same bytes, slower.  (Each pixel is then one dword load from an
 *                  address that is no multiple of 4: this rests on the device serving unaligned global dword loads, which
 *                  tests/test_layouts_gpu.py pins by the bytes.  A load can only return wrong bytes, which a test sees; a store
 *                  could write outside the frame, which is why destinations are refused instead.)
 * Bytes of the destination outside the rectangle drawn into, padding included, are never written. */

int ipx_dev_scale_bilinear_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int dw, int dh,
                                 int dstride, ipx_rect dr, const uint8_t *src, int sw, int sh,
                                 int sstride, ipx_rect sr, int op);
int ipx_dev_draw_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int dw, int dh, int dstride,
                       ipx_rect r, const uint8_t *src, int sw, int sh, int sstride, int spx,
                       int spy, int op);
/* Uploads the glyph masks once (host pointers in `glyphs`); clipping happens per frame size. */
int ipx_glyphset_create(ipx_ctx *ctx, const ipx_glyph *glyphs, int n, const uint8_t col[4],
                        ipx_glyphset **out);
void ipx_glyphset_destroy(ipx_ctx *ctx, ipx_glyphset *gs);
int ipx_dev_composite_glyphs_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int dw, int dh,
                                   int dstride, const ipx_glyphset *gs);

/* ---- one text per frame ------------------------------------------------------------------------
 * The upload form takes the watermark text from the user (watermark_text, internal/http-server/handler/image/image.go:249-251), so
 * the text is a property of each upload like the frame size.  A text set holds n texts -- each one file's DrawString (its DrawMask
 * calls) and parseColor -- clipped against w x h exactly as a glyph set is clipped per frame size (image/draw's clipping of dr against
 * the frame and the mask, mp moved with it), all masks in one block and all descriptors in one table in HBM, uploaded on `stream`
 * (NULL: the context's stream; the call returns when the uploads are done; the stream has to outlive the set).  A text of more than 256
 * glyphs refuses the whole set with IPX_ERR_UNSUPPORTED, as ipx_glyphset_create does; a bad mask (mstride < mw, a null mask with
 * area) is IPX_ERR_INVALID; n_glyphs == 0 is a valid text that draws nothing.
 * ipx_dev_composite_texts_rgba8: n_frames frames of w x h (the set's size) at dst + z * frame_stride; frame z takes text map[z], or
 * text first + z when map is NULL -- ONE launch however many different texts there are; a frame whose text has nothing left inside the
 * frame costs no loads and no stores.  dst, dstride and frame_stride REQUIRED multiples of 4 (the layout rule above: IPX_ERR_INVALID
 * before any launch); no byte outside the frames, and no pixel the text does not change, is written.  `map` is host memory (n_frames
 * entries, each below the set's n, checked before the launch); with a map the call waits for the stream before it returns. */
typedef struct { const ipx_glyph *glyphs; int32_t n_glyphs; uint8_t col[4]; } ipx_text;   /* one file's DrawString + parseColor */
typedef struct ipx_textset ipx_textset;
int ipx_textset_create(ipx_ctx *ctx, void *stream, const ipx_text *texts, int n, int w, int h, ipx_textset **out);
void ipx_textset_destroy(ipx_ctx *ctx, ipx_textset *ts);
int ipx_dev_composite_texts_rgba8(ipx_ctx *ctx, void *stream, uint8_t *dst, int w, int h, int dstride, size_t frame_stride,
                                  int n_frames, const ipx_textset *ts, int first, const int32_t *map /* host, may be NULL */);

/* ---- the batched worker path -------------------------------------------------------------------
 * Replaces (*ImageProcessor).Process (image_processor.go:39-102) between image.Decode (:47) and
 * the encoders (resize.go:78-91, thumbnail.go:68-81, watermark.go:66-79) for a batch of decoded
 * frames of one size: every operator is applied to the ORIGINAL frame (image_processor.go:64-65),
 * so one pass over each source frame produces all requested outputs. */

typedef struct {
    int32_t sw, sh;                 /* frame size                                          */
    int32_t do_resize;              /* operator present in task.Operations (domain/task.go) */
    int32_t resize_w, resize_h, keep_aspect; /* resize.go:26-59                             */
    int32_t do_thumbnail;
    int32_t thumb_size, crop_to_fit;         /* thumbnail.go:25-47; size 0 = 200 (task.go:56) */
    int32_t do_watermark;
    const ipx_glyphset *glyphs;     /* rasterised text; may be NULL (copy only)             */
} ipx_plan_params;

typedef struct {
    int32_t resize_w, resize_h;     /* actual output sizes after the aspect rules           */
    int32_t thumb_w, thumb_h;
    ipx_rect thumb_crop;
    int32_t wm_w, wm_h;
    size_t resize_bytes, thumb_bytes, wm_bytes; /* tightly packed bytes per frame             */
    size_t algorithmic_bytes;       /* source read once + every output written once, per frame */
} ipx_plan_info;

int ipx_plan_create(ipx_ctx *ctx, const ipx_plan_params *p, ipx_plan **out);
void ipx_plan_destroy(ipx_ctx *ctx, ipx_plan *plan);
int ipx_plan_query(const ipx_plan *plan, ipx_plan_info *info);

/* n frames resident in HBM at src + i*src_frame_stride (row stride sstride); outputs tightly
 * packed rows at out + i*out_frame_stride.  An output pointer may be NULL to skip it even when
 * the plan has the operator.  Asynchronous on `stream`.
 *
 * Layout of the ipx_plan_run_dev* entries (tests/test_layouts_gpu.py holds every line):
 *   outputs        each output pointer and its frame stride are REQUIRED multiples of 4 (rows are tight, so every row then is): the
 *                  kernels store whole pixels -- the one-pass kernel four at a time into the watermark frames -- through buffer
 *                  descriptors built at that address.  Anything else is IPX_ERR_INVALID, decided on the host before any launch;
 *                  nothing is written.  No more than 4 is needed: frame strides larger than the frames, and frames at 4, 8 or 12
 *                  bytes past a 16-byte boundary, run on the same kernels, and no byte between or around the frames is written.
 *   RGBA8, NRGBA8  src, sstride and src_frame_stride multiples of 4: the one-pass kernel (ks_fused_kernel), any width (rows whose
 *                  width is no multiple of 4 have a variant of their own).  Otherwise the batch is served by one kernel per
 *                  output, which reads a pixel at a time (an unaligned dword load each, as for the ipx_dev_* sources above): the
 *                  same bytes, slower.
 *   Gray, Y        pointer, row stride and frame stride multiples of 4 AND a width that is a multiple of 4: the one-pass kernel;
 *                  otherwise one kernel per output (byte loads), slower.
 *   Cb, Cr         as Y, but multiples of 2 are enough for 4:2:2 and 4:2:0 (4:4:4 and 4:4:0: 4; 4:1:1 and 4:1:0: any, their chroma
 *                  is read a byte per four pixels).
 *   index planes   any layout; multiples of 4 (and a width that is one) take the expansion's vector path.  The expanded frames are
 *                  the library's own, so the one-pass kernel runs whatever the index planes' layout.
 *   palettes       REQUIRED 4-byte aligned (IPX_ERR_INVALID otherwise).
 *   deep types     src, sstride and src_frame_stride REQUIRED multiples of 2 (CMYK: 4), IPX_ERR_INVALID otherwise; the expanded taps
 *                  are the library's own: the one-pass kernel when the width is a multiple of 4, one kernel per output otherwise.
 * A plan whose resize enlarges by more than about two (a source row feeding more than four output rows) has no one-pass kernel at all.
 * The host variants (ipx_plan_run_host*) take any layout of sources and outputs: frames are copied row by row where they are not
 * tight; pinned outputs whose pointers and frame strides are all multiples of 16 are stored by the kernels directly, others are
 * copied a frame at a time, and bytes between the frames are never written either way. */
int ipx_plan_run_dev(ipx_ctx *ctx, void *stream, const ipx_plan *plan, int n, const uint8_t *src,
                     int sstride, size_t src_frame_stride, uint8_t *resize_out,
                     size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride,
                     uint8_t *wm_out, size_t wm_frame_stride);

/* Host-to-host variant for the worker: frames and outputs in pinned memory from ipx_host_alloc
 * (or any host memory, slower); copies and kernels are pipelined over the context's lanes so
 * H2D, kernels and D2H of consecutive chunks overlap.  Synchronous. */
int ipx_plan_run_host(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *src, int sstride,
                      size_t src_frame_stride, uint8_t *resize_out, size_t resize_frame_stride,
                      uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out,
                      size_t wm_frame_stride);

/* A batch of decoded JPEG frames (what image.Decode returns, image_processor.go:47) for the same plan:
 * planes of frame i at y + i*y_frame_stride and cb / cr + i*c_frame_stride.  Per operator the reference
 * converts differently (16-bit per tap inside resize; RGBA8 first for the crop thumbnail and the
 * watermark); the results are those of the reference's helpers on the *image.YCbCr itself.  The host
 * variant uploads 1.5 bytes per pixel for 4:2:0 instead of 4. */
typedef struct {
    const uint8_t *y, *cb, *cr;
    int32_t ystride, cstride;
    size_t y_frame_stride, c_frame_stride;
    int32_t ratio;                  /* IPX_YCBCR_* */
} ipx_ycbcr_batch;
int ipx_plan_run_dev_ycbcr(ipx_ctx *ctx, void *stream, const ipx_plan *plan, int n, const ipx_ycbcr_batch *src,
                           uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                           size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
/* A batch of *image.NRGBA frames (PNGs with alpha): like the YCbCr batch, per operator as the reference's helpers treat the
 * type -- resize and the non-crop thumbnail weight 16-bit premultiplied taps (scaleX_NRGBA), the crop thumbnail scales its 8-bit
 * crop copy and the watermark premultiplies to RGBA8 (drawNRGBASrc).  One pass (ks_fused_kernel) for frames whose pointer, row stride
 * and frame stride are multiples of 4 -- at any width: rows that are no multiple of 4 pixels wide have a variant of the kernel --,
 * one kernel per output otherwise; the same bytes either way (the layout rules above ipx_plan_run_dev). */
int ipx_plan_run_dev_nrgba(ipx_ctx *ctx, void *stream, const ipx_plan *plan, int n, const uint8_t *src, int sstride,
                           size_t src_frame_stride, uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                           size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
/* A batch of *image.Gray frames (one-component JPEGs, grey PNGs): image/draw's drawGray and x/image's
 * scaleX_Gray both read a source pixel as (y, y, y, 0xff).  A YCbCr pixel with Cb = Cr = 128 converts to exactly that in both of
 * the reference's conversions, so the batch takes the planar pass with a constant chroma row (1 byte per pixel read); shapes that kernel
 * does not take are expanded to RGBA8 in HBM and take the RGBA pass.  The outputs are bit for bit the reference's either way. */
int ipx_plan_run_dev_gray(ipx_ctx *ctx, void *stream, const ipx_plan *plan, int n, const uint8_t *gray, int stride,
                          size_t frame_stride, uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                          size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
/* A batch of *image.Paletted frames (what image.Decode returns for GIF uploads and palette PNGs, image_processor.go:47): one index
 * byte per pixel plus, per frame, 256 palette entries of 4 bytes (R, G, B, A), non-premultiplied, unused entries zero; palettes of
 * frame i at palettes + i*1024, in device memory, 4-byte aligned.  No routine of x/image or image/draw specialises on this type: the
 * generic ones (scaleX_Image, drawRGBA) read Palette[i].RGBA() per tap.  For every entry the GIF and PNG decoders produce --
 * opaque color.RGBA, the zero colour for a GIF's transparent index, color.NRGBA for a PNG's tRNS -- that is exactly the
 * premultiplication scaleX_NRGBA / drawNRGBA* apply to (R, G, B, A), so the frames are expanded to NRGBA8 in HBM and take
 * ipx_plan_run_dev_nrgba; outputs are bit for bit the generic routines' (tests/test_sources_gpu.py against an oracle of those). */
int ipx_plan_run_dev_paletted(ipx_ctx *ctx, void *stream, const ipx_plan *plan, int n, const uint8_t *index, int stride,
                              size_t frame_stride, const uint8_t *palettes, uint8_t *resize_out, size_t resize_frame_stride,
                              uint8_t *thumb_out, size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
/* The same three source types from host memory (frames Go's png / gif / jpeg decoders left there), chunked over the lanes like
 * ipx_plan_run_host; `palettes` is host memory here. */
int ipx_plan_run_host_nrgba(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                            uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride,
                            uint8_t *wm_out, size_t wm_frame_stride);
int ipx_plan_run_host_gray(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *gray, int stride, size_t frame_stride,
                           uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out, size_t thumb_frame_stride,
                           uint8_t *wm_out, size_t wm_frame_stride);
int ipx_plan_run_host_paletted(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *index, int stride, size_t frame_stride,
                               const uint8_t *palettes, uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                               size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
/* The remaining image types image.Decode returns (image_processor.go:47) -- *image.NRGBA64, *image.RGBA64, *image.Gray16 from 16-bit
 * PNGs, *image.CMYK from four-component JPEGs ("deep" sources; SURVEY.md 8(f) N2 tail).  resizeImage (resize.go:121-125) takes them
 * through x/image's generic scaleX_Image, which reads every tap as src.At(x, y).RGBA() at full 16-bit precision; the
 * crop copy (thumbnail.go:128-130) and draw.Draw (watermark.go:92) go through image/draw's drawRGBA (drawCMYK for CMYK) and keep the
 * top byte of the same value.  `src` is Go's Pix for the type: big-endian 16-bit channels R G B A (8 bytes per pixel; NRGBA64 not
 * premultiplied, RGBA64 premultiplied), big-endian Y (2 bytes), or C M Y K bytes (4); rows `sstride` bytes apart, 2-byte aligned
 * (CMYK: 4).  One pass expands the frames to those 16-bit taps in HBM (8 bytes per pixel); the fused converted-tile kernel then reads
 * them as they are.  Bit for bit the generic routines' outputs (tests/test_deep_gpu.py against the oracle's restatement). */
enum { IPX_DEEP_NRGBA64 = 0, IPX_DEEP_RGBA64 = 1, IPX_DEEP_GRAY16 = 2, IPX_DEEP_CMYK = 3 };
/* the per-operation seam for these types (host pointers, one frame; like ipx_scale_bilinear_nrgba8 / ipx_draw_nrgba8): Scale with any
 * rectangles and either op -- Over turns into Src when (*NRGBA64).Opaque / (*RGBA64).Opaque holds, Gray16 and CMYK are opaque -- and
 * draw.Draw (drawRGBA; drawCMYK for CMYK) */
int ipx_scale_bilinear_deep(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect dr, const uint8_t *src, int sw, int sh,
                            int sstride, int kind, ipx_rect sr, int op);
int ipx_draw_deep(ipx_ctx *ctx, uint8_t *dst, int dw, int dh, int dstride, ipx_rect r, const uint8_t *src, int sw, int sh, int sstride,
                  int kind, int spx, int spy, int op);
int ipx_plan_run_dev_deep(ipx_ctx *ctx, void *stream, const ipx_plan *plan, int n, int kind, const uint8_t *src, int sstride,
                          size_t src_frame_stride, uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                          size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
int ipx_plan_run_host_deep(ipx_ctx *ctx, const ipx_plan *plan, int n, int kind, const uint8_t *src, int sstride,
                           size_t src_frame_stride, uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                           size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);
int ipx_plan_run_host_ycbcr(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_ycbcr_batch *src,
                            uint8_t *resize_out, size_t resize_frame_stride, uint8_t *thumb_out,
                            size_t thumb_frame_stride, uint8_t *wm_out, size_t wm_frame_stride);

/* Average duration in milliseconds of the last `ipx_plan_run_dev` launches on `stream` is a
 * measurement concern of the caller: bracket calls with ipx_event_* below (HIP events on the
 * stream the kernels run on). */
void *ipx_event_create(ipx_ctx *ctx);
int ipx_event_record(ipx_ctx *ctx, void *event, void *stream);
int ipx_event_elapsed_ms(ipx_ctx *ctx, void *start, void *stop, float *ms); /* syncs on stop */
void ipx_event_destroy(ipx_ctx *ctx, void *event);

/* ---- operator seam: the reference's own method set on decoded frames ---------------------------
 * Resizer / Thumbnailer / Watermarker .Process(ctx, img, format, params) (resize.go:26,
 * thumbnail.go:25, watermark.go:40) and ImageProcessor.Process (image_processor.go:39) with the
 * codecs cut off: the input is the decoded frame (image_processor.go:47 stays on the Go side) and
 * each result is the *image.RGBA the reference would hand to its encoder, plus the format string
 * and object key it would use.  Parameter parsing, defaults and error texts follow the reference. */

/* one entry of Go's map[string]interface{}; the type tag reproduces the reference's type switches
 * (after the JSON round trip of a task every number is float64, domain/task.go:17-20) */
typedef enum {
    IPX_PT_FLOAT64 = 1, IPX_PT_INT = 2, IPX_PT_INT64 = 3, IPX_PT_INT32 = 4, IPX_PT_BOOL = 5, IPX_PT_STRING = 6
} ipx_param_type;
typedef struct {
    const char *key;
    int32_t type;      /* ipx_param_type */
    double f64;        /* FLOAT64 */
    int64_t i64;       /* INT / INT64 / INT32 / BOOL */
    const char *str;   /* STRING */
} ipx_param;

/* *image.RGBA with Rect.Min = (0,0).  Outputs are allocated by the library (ipx_image_free). */
typedef struct { uint8_t *pix; int32_t w, h, stride; } ipx_image;
void ipx_image_free(ipx_image *img);

/* The text rasteriser sits on the host side of the boundary (the reference uses golang/freetype
 * with the Go Regular face, watermark.go:29-38,98-118,151).  measure() returns
 * int(textWidth.Ceil()) of watermark.go:109-117; glyphs() returns, for the baseline point (px, py)
 * and a frame of w x h (c.SetClip(result.Bounds()), watermark.go:101), the DrawMask calls
 * DrawString would make (valid until release()).  A NULL rasteriser makes Watermarker.Process fail
 * with "font not loaded" like a nil font (watermark.go:87-89).  ipx_font_rasterizer() below fills
 * one in from a parsed TrueType font; a caller may also supply its own. */
typedef struct {
    void *user;
    int (*measure)(void *user, const char *text, double font_size, int *width_px);
    int (*glyphs)(void *user, const char *text, double font_size, int px, int py, int w, int h,
                  const ipx_glyph **out, int *n);
    void (*release)(void *user);
} ipx_text_rasterizer;

/* ---- glyph mask producer: truetype.Parse + freetype.Context.DrawString ------
 * A restatement of github.com/golang/freetype @ e2365dfdc4a0 (go.mod:42) without hinting, which is
 * all the reference uses: cmap formats 4 / 12, simple and compound glyphs, kern format 0, the
 * quadratic-spline cell rasteriser (even-odd), 4 horizontal sub-pixel positions.  Host code: the
 * masks are a few hundred bytes each and cached; the composite is the GPU's part. */
typedef struct ipx_font ipx_font;
/* truetype.Parse (watermark.go:31).  Failure = the reference's nil font; text in ipx_last_error(). */
int ipx_font_create(const uint8_t *ttf, size_t len, ipx_font **out);
void ipx_font_destroy(ipx_font *font);
/* (f *Font).Index */
int ipx_font_glyph_index(const ipx_font *font, uint32_t rune);
/* face.GlyphAdvance of truetype.NewFace(font, {Size, DPI: 72}) (watermark.go:105-111), 26.6 fixed */
int ipx_font_glyph_advance(const ipx_font *font, uint32_t rune, double font_size, int32_t *advance26_6);
/* (f *Font).Kern at the freetype.Context's scale (what DrawString adds between runes), 26.6 fixed */
int ipx_font_kern(const ipx_font *font, uint32_t rune0, uint32_t rune1, double font_size, int32_t *kern26_6);
/* watermark.go:108-117: textWidth = sum of advances (no kerning) and int(textWidth.Ceil()) */
int ipx_font_text_width(const ipx_font *font, const char *text, double font_size, int32_t *width26_6,
                        int *width_px);
/* c.DrawString(text, freetype.Pt(px, py)) with c.SetClip((0,0)-(clip_w,clip_h)) (watermark.go:98-104,151):
 * the DrawMask calls in rune order.  *out stays valid until the next call on the calling thread or
 * ipx_font_release_thread().  end_x26_6 (may be NULL) receives the returned point's X. */
int ipx_font_draw_string(ipx_font *font, const char *text, double font_size, int px, int py, int clip_w,
                         int clip_h, const ipx_glyph **out, int *n, int32_t *end_x26_6);
void ipx_font_release_thread(void);
/* Fills an ipx_text_rasterizer whose callbacks are the three entries above. */
int ipx_font_rasterizer(ipx_font *font, ipx_text_rasterizer *out);

/* out_format receives "jpeg" / "png" / "gif" as the reference's encoder switch would name it
 * (resize.go:78-91, thumbnail.go:68-81, watermark.go:66-79: a GIF watermark becomes JPEG). */
int ipx_resizer_process(ipx_ctx *ctx, const ipx_image *img, const char *format,
                        const ipx_param *params, int nparams, ipx_image *out, char out_format[8]);
int ipx_thumbnailer_process(ipx_ctx *ctx, const ipx_image *img, const char *format,
                            const ipx_param *params, int nparams, ipx_image *out, char out_format[8]);
int ipx_watermarker_process(ipx_ctx *ctx, const ipx_image *img, const char *format,
                            const ipx_param *params, int nparams, const ipx_text_rasterizer *font,
                            ipx_image *out, char out_format[8]);

/* domain.OperationParams / domain.ProcessingTask (domain/task.go:3-20) */
typedef struct { const char *type; const ipx_param *params; int32_t nparams; } ipx_operation;
typedef struct {
    const char *id, *image_id;
    const ipx_operation *ops; int32_t nops;
    const char *format;            /* task.Format; "" = the decoded format (image_processor.go:55-58) */
} ipx_task;
typedef struct {
    char operation[16];            /* key of ProcessingResult.ProcessedPaths                    */
    char path[320];                /* generatePath (image_processor.go:129-162)                 */
    char content_type[32];         /* getContentType (image_processor.go:164-182)               */
    char format[8];
    ipx_image image;
} ipx_processed;
/* (*ImageProcessor).Process (image_processor.go:39-102) from the decoded frame on: every operator
 * is applied to the ORIGINAL frame (:64-65), in one fused GPU pass when each type occurs at most
 * once.  `out` has room for task->nops entries; *n_out of them are filled.  On an operator failure
 * the status is negative, *n_out counts the operators that had succeeded before it, and
 * ipx_last_error() holds "operation <type> failed: ..." as the reference formats it (:66-75). */
int ipx_processor_process(ipx_ctx *ctx, const ipx_task *task, const ipx_image *decoded,
                          const char *decoded_format, const ipx_text_rasterizer *font,
                          ipx_processed *out, int *n_out);

/* ---- jpeg.Encode (encoder side) ------------------------------------------------
 * Every operator of the reference ends in jpeg.Encode(buf, img, &jpeg.Options{Quality: 85}) on its
 * *image.RGBA (resize.go:80, thumbnail.go:70, watermark.go:68,73,76).  Go's writer is restated on the GPU end to end: colour
 * conversion, 2x2 chroma box, jfdctint and the quantiser leave int16 coefficients (zig-zag order, 6 x 64 per 16x16 MCU in scan order
 * Y0 Y1 Y2 Y3 Cb Cr); the Huffman coder sizes every block while it still sits in LDS, places the bits, stuffs 0xff bytes and
 * prepends SOI / DQT / SOF0 / DHT / SOS in further kernels (ipx_jpeg_encode_batch_dev and the ipx_plan_run_*_jpeg entries), so only
 * finished streams cross the link.  ipx_jpeg_entropy_encode is the same coder on the host, for coefficients a caller has downloaded.
 * The byte stream is the one Go's encoder writes (no JFIF segment, both DQT tables, 4:2:0, Annex K Huffman tables).
 * Limit of the GPU entropy coder: the bit offsets inside a frame's scan are 32-bit, so a batch holding a frame whose entropy-coded scan
 * reaches 2^32 - 1 bits (512 MiB; some 200 M pixels of noise at quality 100) is refused as a whole by ipx_jpeg_encode_batch_dev and the
 * ipx_plan_run_*_jpeg entries with IPX_ERR_UNSUPPORTED, "jpeg: scan too long for the GPU entropy coder", before anything is
 * written; the worker keeps its CPU path for it.  ipx_jpeg_encode_rgba8 and ipx_jpeg_entropy_encode (host coder) have no such limit. */
size_t ipx_jpeg_coef_count(int w, int h);                 /* int16 elements per frame                 */
int ipx_jpeg_quant_tables(int quality, uint8_t out[128]); /* the two DQT tables, zig-zag order         */
/* n frames resident in HBM -> coefficients in HBM (n * ipx_jpeg_coef_count int16).  Asynchronous. */
int ipx_dev_jpeg_fdct_rgba8(ipx_ctx *ctx, void *stream, const uint8_t *src, int w, int h, int stride,
                            size_t frame_stride, int n, int quality, int16_t *coefs);
/* Host half: coefficients (host memory) -> the complete stream.  *out is malloc'd: ipx_buffer_free. */
int ipx_jpeg_entropy_encode(const int16_t *coefs, int w, int h, int quality, uint8_t **out, size_t *len);
/* jpeg.Encode for one frame in host memory (upload, transform, download, entropy coding). */
int ipx_jpeg_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, int quality,
                          uint8_t **out, size_t *len);
/* n frames resident in HBM -> n streams in ONE block of host memory: transform, entropy coding (sizing,
 * placement and 0xff stuffing) and headers all happen on the GPU and only the finished streams cross the
 * link.  *blob is pinned memory owned by the library (ipx_host_free); stream i is blob[offs[i] ..
 * offs[i] + lens[i]).  cgo: wrap each with unsafe.Slice, write it out, then free the block. */
int ipx_jpeg_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride,
                              size_t frame_stride, int n, int quality, uint8_t **blob, size_t *offs,
                              size_t *lens);
void ipx_buffer_free(void *p);

/* The worker's whole GPU leg for a batch of decoded frames in host memory (image_processor.go:64-77 without
 * image.Decode): upload, every requested operator in one pass, jpeg.Encode of each output on the GPU, and
 * only the finished streams come back.  resize_out / thumb_out / wm_out (n entries each, or NULL to skip)
 * receive pointers into pinned blocks owned by *result; release them with ipx_jpeg_result_free once the
 * streams are written out (fileRepo.SaveProcessed, image_processor.go:76).  Chunks run on the context's
 * lanes, one host thread per lane, so uploads, kernels and downloads of different chunks overlap. */
typedef struct { const uint8_t *data; size_t len; } ipx_bytes;
typedef struct ipx_jpeg_result ipx_jpeg_result;
int ipx_plan_run_host_jpeg(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *src, int sstride,
                           size_t src_frame_stride, int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out,
                           ipx_bytes *wm_out, ipx_jpeg_result **result);
/* The same for a batch of decoded JPEGs (*image.YCbCr planes): 1.5 bytes per pixel go up for 4:2:0 instead of 4. */
int ipx_plan_run_host_ycbcr_jpeg(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_ycbcr_batch *src,
                                 int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out,
                                 ipx_jpeg_result **result);
void ipx_jpeg_result_free(ipx_ctx *ctx, ipx_jpeg_result *result);

/* ---- gif.Encode (GIF half) ---------------------------------------------------------
 * resize.go:78-91 and thumbnail.go:68-81 end a GIF task in gif.Encode(buf, img, nil) on the operator's *image.RGBA: no palette to
 * reuse, so image/gif draws the frame onto palette.Plan9 with draw.FloydSteinberg (image/draw drawPaletted) and LZW-codes the indices
 * (compress/lzw, LSB, literal width 8) into one image block.  Both run on the GPU: the dither as a wavefront of rows in flight, LZW one
 * wave per frame with the dictionary in LDS, and only finished streams cross the link.  The bytes are the ones Go's writer produces for a
 * single frame (GIF89a, global Plan 9 table, no extensions, LZW minimum code size 8, trailer 0x3B).  Frames 65536 pixels or more in
 * either dimension are refused (IPX_ERR_INVALID), as gif.Encode refuses them.  DESIGN.md section 4.7. */
/* one frame in host memory -> *out, malloc'd (ipx_buffer_free) */
int ipx_gif_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, uint8_t **out, size_t *len);
/* n frames resident in HBM -> n streams in ONE pinned block, the ownership rules of ipx_jpeg_encode_batch_dev: *blob is freed with
 * ipx_host_free; stream i is blob[offs[i] .. offs[i] + lens[i]). */
int ipx_gif_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                             size_t *offs, size_t *lens);
/* the dither alone: n frames in HBM -> n dense w x h index frames (Plan 9 indices) at index + i * w * h, in HBM.  Asynchronous on
 * `stream` (NULL: the context's stream). */
int ipx_dev_gif_dither_rgba8(ipx_ctx *ctx, void *stream, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n,
                             uint8_t *index);
/* The GIF task's whole GPU leg for a batch of decoded GIF frames in host memory (the arguments of ipx_plan_run_host_paletted):
 * upload, every requested operator, then gif.Encode of the resize and thumbnail outputs and jpeg.Encode at `quality` of the watermark
 * output (watermark.go:66-79: a GIF watermark becomes a JPEG).  The streams land in pinned blocks owned by *result, released with
 * ipx_jpeg_result_free as for ipx_plan_run_host_jpeg. */
int ipx_plan_run_host_paletted_gif(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *index, int stride, size_t frame_stride,
                                   const uint8_t *palettes, int quality, ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out,
                                   ipx_jpeg_result **result);

/* ---- png.Encode (PNG half) ---------------------------------------------------------
 * resize.go:83, thumbnail.go:73 and watermark.go:71 end a PNG task in png.Encode(buf, img) on the operator's *image.RGBA.  Go's
 * visible decisions are kept exactly: colour type 2 (RGB 8) when every alpha byte is 0xff, else 6 (RGBA 8) with the writer's
 * un-premultiply; per row the filter Go's heuristic picks (smallest sum of abs8; Up, Paeth, None, Sub, Average on ties); IHDR, IDAT
 * chunks, IEND and nothing else.  The zlib stream is this project's own (segments of whole rows deflated independently on the GPU,
 * one IDAT chunk each, the Adler-32 in a last 4-byte IDAT chunk): any inflater decodes it to the rows png.Encode would have
 * compressed, but the compressed bytes are not Go's.  A width or height below 1 is refused (IPX_ERR_INVALID), as Go refuses it;
 * frames beyond ipx_frame_supported get IPX_ERR_UNSUPPORTED.  DESIGN.md section 4.9. */
/* one frame in host memory -> *out, malloc'd (ipx_buffer_free) */
int ipx_png_encode_rgba8(ipx_ctx *ctx, const uint8_t *pix, int w, int h, int stride, uint8_t **out, size_t *len);
/* n frames resident in HBM (e.g. after any ipx_plan_run_dev_*) -> n streams in ONE pinned block, the ownership rules of
 * ipx_gif_encode_batch_dev: *blob is freed with ipx_host_free; stream i is blob[offs[i] .. offs[i] + lens[i]). */
int ipx_png_encode_batch_dev(ipx_ctx *ctx, const uint8_t *src, int w, int h, int stride, size_t frame_stride, int n, uint8_t **blob,
                             size_t *offs, size_t *lens);
/* The same for n frames of ANY sizes, each described on its own: RGBA8 in HBM, pix and stride multiples of 4.  One launch per stage
 * for the whole call however many sizes it holds (the kernels read a per-frame table), and stream i is byte for byte what
 * ipx_png_encode_batch_dev writes for frame i alone: nothing of it depends on its neighbours or its place.  The rules are that
 * entry's: one pinned block (ipx_host_free), streams that start 16-byte aligned, a width or height below 1 IPX_ERR_INVALID, a frame
 * beyond ipx_frame_supported IPX_ERR_UNSUPPORTED, more than 65535 frames IPX_ERR_UNSUPPORTED; one bad frame refuses the call before
 * any launch.  DESIGN.md section 4.9. */
typedef struct { const uint8_t *pix; int32_t w, h, stride; } ipx_rgba_frame;
int ipx_png_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, uint8_t **blob, size_t *offs, size_t *lens);
/* jpeg.Encode of n frames of ANY sizes and strides, each described on its own: RGBA8 in HBM.  One launch per stage for the whole call
 * however many sizes it holds (the kernels read a per-frame record) and three waits for the device in all, as
 * ipx_jpeg_encode_batch_dev has for one size; stream i is byte for byte what that entry writes for frame i in a call of its own at the
 * same quality.  One pinned block (ipx_host_free), streams that start 16-byte aligned; n == 0 is IPX_OK with *blob = NULL.  One bad
 * frame refuses the call before any launch: a NULL pix, a width or height below 1, a stride below 4 * w or a side of 65536 or more
 * IPX_ERR_INVALID, a frame beyond ipx_frame_supported IPX_ERR_UNSUPPORTED; more than 65535 frames IPX_ERR_UNSUPPORTED.  A frame whose
 * scan reaches the GPU entropy coder's limit (above) refuses the call with IPX_ERR_UNSUPPORTED and is named in the message.  The
 * blocks are always sized in the transform kernel: IPX_JPEG_FUSED_LEN and IPX_JPEG_HOST_ENTROPY do not apply.  Thread-safe like
 * ipx_jpeg_encode_batch_dev.  DESIGN.md section 4.6. */
int ipx_jpeg_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, int quality, uint8_t **blob, size_t *offs, size_t *lens);
/* gif.Encode of n frames of ANY sizes and strides, each described on its own: RGBA8 in HBM.  Stream i is byte for byte what
 * ipx_gif_encode_batch_dev writes for frame i in a call of its own: nothing in it depends on its neighbours, on its place in the call
 * or on how many rows were in flight.  The kernels read a per-frame record: one dither launch per number of rows in flight (at most
 * 16, one workgroup per frame, a frame's rows in flight from its own height), one LZW launch (one wave per frame, the longest first)
 * and one packing launch, and the host waits for the device twice -- the lengths, the download -- as ipx_gif_encode_batch_dev does,
 * whatever sizes the call holds.  One pinned block (ipx_host_free), streams that start 16-byte aligned; n == 0 is IPX_OK with *blob =
 * NULL.  One bad frame refuses the call before any launch: a NULL pix, a width or height below 1 or a stride below 4 * w
 * IPX_ERR_INVALID, a side of 65536 or more IPX_ERR_INVALID with gif.Encode's message, a frame beyond ipx_frame_supported
 * IPX_ERR_UNSUPPORTED; more than 65535 frames IPX_ERR_UNSUPPORTED.  Thread-safe like ipx_gif_encode_batch_dev.  DESIGN.md section 4.7. */
int ipx_gif_encode_mixed_dev(ipx_ctx *ctx, const ipx_rgba_frame *frames, int n, uint8_t **blob, size_t *offs, size_t *lens);
/* The PNG task's whole GPU leg (ipx_plan_run_host's inputs): upload, every requested operator, then png.Encode of all three outputs
 * (a PNG watermark stays PNG).  The streams land in pinned blocks owned by *result, released with ipx_jpeg_result_free. */
int ipx_plan_run_host_png(ipx_ctx *ctx, const ipx_plan *plan, int n, const uint8_t *src, int sstride, size_t src_frame_stride,
                          ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, ipx_jpeg_result **result);

/* ---- image.Decode for JPEGs (decoder side) -------------------------------------------
 * image_processor.go:47 decodes every upload; for JPEG files that is Go's image/jpeg.  A batch of
 * files of one size and one kind (three components at 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0, or one component; with IPX_JPEG_411=1 in the
 * environment -- read on every call; unset or anything else: as before -- also 4:1:1 and 4:1:0, luma factors (4,1) and (4,2) with 1x1
 * chroma, planes->ratio IPX_YCBCR_411 / IPX_YCBCR_410; their progressive and multi-scan files keep the host route) is decoded here.  Baseline files:
 * the compressed bytes go up, Huffman decoding runs in parallel inside each scan (or per restart interval), the integer IDCT of idct.go runs
 * block-parallel.  Progressive (SOF2), multi-scan and extended-sequential files: their scans are decoded by the host threads that parse
 * the batch (the scans refine each other), the coefficients go up, IDCT onwards is the same GPU path.  With IPX_JPEG_PROG_GPU=1 in the
 * environment (read on every call; unset or anything else: as before) a progressive file whose marker pre-pass is wholly clean -- it
 * reaches EOI, every SOS header is valid, every Huffman table a scan decodes with is defined, no restart interval, at most 64 scans -- goes
 * up as compressed bytes instead and one GPU wave per file walks its scans in file order; every other file keeps the host route, and the
 * planes and statuses are the same on both.  Either way the *image.YCbCr planes
 * (MCU-padded strides, as image.NewYCbCr lays them out) stay in
 * HBM, ready for ipx_plan_run_dev_ycbcr (ratio IPX_GRAY: only y is set; ipx_plan_run_dev_gray).  status[i]: IPX_OK, IPX_ERR_INVALID (malformed:
 * Go's decoder fails on the file too, including a file that ends without EOI) or
 * IPX_ERR_UNSUPPORTED (CMYK / RGB, other samplings, a size or sampling
 * different from the batch's, damaged restart intervals Go would resynchronise over, coefficients beyond int16): the worker decodes those
 * with Go as before.  planes->y == NULL when no
 * image was decodable.  Free the planes with ipx_jpeg_planes_free: they are stream-ordered allocations of `stream` (NULL: the
 * context's default stream), which has to outlive them. */
typedef struct ipx_jpeg_planes ipx_jpeg_planes;
/* Compressed in, compressed out: the uploads as they arrive from the object store (image_processor.go:41-47), the
 * objects as they go back (:76).  image.Decode, every operator of the plan and jpeg.Encode run on the GPU; the
 * link carries ~0.3 MB up and ~0.5 MB down per 1080p image.  status[i] as for ipx_jpeg_decode_batch (the
 * plan's frame size is the batch's size); outputs of undecodable files are {NULL, 0}.  Under IPX_JPEG_CMYK=1 the four-component
 * files of the call (see ipx_jpeg_decode_batch_cmyk) are taken out of it, decoded to *image.CMYK frames and run as sub-batches of one
 * sampling vector each; streams and statuses land at the files' own indices, the rest of the call runs as without the switch. */
int ipx_plan_run_jpeg_jpeg(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_bytes *files, int quality,
                           ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status,
                           ipx_jpeg_result **result);
int ipx_jpeg_decode_batch(ipx_ctx *ctx, void *stream, const ipx_bytes *jpegs, int n, int *w, int *h,
                          ipx_ycbcr_batch *planes, int *status, ipx_jpeg_planes **owner);
void ipx_jpeg_planes_free(ipx_ctx *ctx, ipx_jpeg_planes *owner);
/* Which decoder a JPEG file's scans reach: the parallel Huffman kernels (one baseline scan), the host threads, or the GPU scan walk. */
enum { IPX_JPEG_ROUTE_PAR = 0, IPX_JPEG_ROUTE_HOST_SCANS = 1, IPX_JPEG_ROUTE_GPU_SCANS = 2 };
/* host only, no context: the route this file would take now (IPX_JPEG_PROG_GPU is read; under IPX_JPEG_CMYK=1 a four-component file of a
 * sampling vector Go takes answers IPX_OK and the host route; under IPX_JPEG_411=1 a 4:1:1 or 4:1:0 file answers IPX_OK with the parallel
 * route for one baseline scan and the host route otherwise, never the GPU scan walk); returns the parse status, *route is meaningful when that is IPX_OK */
int ipx_jpeg_scan_route(const uint8_t *file, size_t len, int *route);
/* since ipx_create: the files that reached the decoder of route [0..2] in any decode entry of this context (whatever status they ended
 * with; files refused by the marker parser or for their geometry reach none), and [3] the files the GPU scan walk ended with a status
 * other than IPX_OK */
int ipx_jpeg_decode_counts(ipx_ctx *ctx, long long counts[4]);
/* n JPEG files of any sizes and samplings in ONE decode pass per sampling class.  The files are grouped by class -- one (h0, v0,
 * components): 4:4:4, 4:2:2, 4:2:0, 4:4:0 or Gray -- and every class is decoded by one set of launches whatever sizes it holds: the
 * kernels read each image's geometry from a per-image record in HBM instead of the launch arguments.  One
 * baseline scan goes to the parallel Huffman passes, restart intervals to the piece kernels, progressive and multi-scan files to the
 * host threads.  frames[i] describes file i's own *image.YCbCr or *image.Gray in HBM: its size, its ratio (IPX_YCBCR_*, IPX_GRAY),
 * the planes (256-byte aligned) and the MCU-padded strides of image.NewYCbCr; cb and cr are NULL and cstride 0 for IPX_GRAY; every
 * field is zero for a non-OK file.  status[i] is exactly what ipx_jpeg_decode_batch gives that file in a call of its own with
 * *w = *h = 0: no file is IPX_ERR_UNSUPPORTED because of a neighbour's size or sampling.  Whatever the switches say, in this entry
 * the GPU scan walk (IPX_JPEG_PROG_GPU=1) is not used -- such files take the host route, with the same planes and statuses -- and
 * 4:1:1, 4:1:0 (IPX_JPEG_411=1) and four-component files (IPX_JPEG_CMYK=1) are IPX_ERR_UNSUPPORTED.  The three route counters of
 * ipx_jpeg_decode_counts count these files too.  *owner (NULL when nothing decoded) is freed with ipx_jpeg_planes_free.  n == 0 is
 * IPX_OK; more than 65535 files is IPX_ERR_UNSUPPORTED. */
typedef struct { int32_t w, h, ratio; uint8_t *y, *cb, *cr; int32_t ystride, cstride; } ipx_jpeg_frame;
int ipx_jpeg_decode_mixed(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, ipx_jpeg_frame *frames, int *status,
                          ipx_jpeg_planes **owner);
/* Four-component JPEGs (Adobe CMYK and YCCK: print-workflow and Photoshop files), with IPX_JPEG_CMYK=1 in the environment (read on every
 * call; unset or anything else: every such file is IPX_ERR_UNSUPPORTED in every entry, as before).  Go takes two sampling vectors,
 * (h, v) = 11 11 11 11 and 22 11 11 22, and needs a valid Adobe APP14 segment; a file of the call's size (*w, *h: 0, or the size the
 * batch must have) and of the first such file's vector is decoded -- every scan on the host threads, baseline and progressive alike, the
 * IDCT and applyBlack on the GPU -- into an *image.CMYK frame: frame i at pix + i * frame_stride, rows `stride` = 4 * w bytes apart, ready
 * for ipx_plan_run_dev_deep(..., IPX_DEEP_CMYK, ...).  status[i]: IPX_OK, IPX_ERR_INVALID (malformed) or IPX_ERR_UNSUPPORTED (any other
 * vector, no APP14 segment, another size or vector than the batch's, and every three- or one-component file: those are
 * ipx_jpeg_decode_batch's).  pix == NULL when no file was decodable; the frames of non-OK files are undefined.  Free the frames with
 * ipx_jpeg_planes_free.  DESIGN.md section 4.6. */
typedef struct { uint8_t *pix; int32_t stride; size_t frame_stride; } ipx_cmyk_batch;
int ipx_jpeg_decode_batch_cmyk(ipx_ctx *ctx, void *stream, const ipx_bytes *jpegs, int n, int *w, int *h,
                               ipx_cmyk_batch *frames, int *status, ipx_jpeg_planes **owner);
/* files that reached the four-component decoder (of this entry or of a compressed-in leg) since ipx_create, whatever came of them */
int ipx_jpeg_cmyk_files(ipx_ctx *ctx, long long *files);

/* ---- image.Decode for GIFs (decoder side) ---------------------------------------------
 * For a GIF upload image.Decode is gif.Decode: the FIRST image of the file as an *image.Paletted.  The host reads the container
 * (header, tables, extensions, descriptor) and strips the sub-block framing; the LZW data go up, one lane per file walks the codes
 * (every validity rule of compress/lzw's reader, O(1) work per code) and the workgroups of a second kernel expand the codes' strings in
 * parallel straight into row order (interlace undone).  Frames stay in HBM, ready for ipx_plan_run_dev_paletted: frame i (file i) at
 * index + i * frame_stride, rows `stride` bytes apart, its 256 x (R, G, B, A) palette at palettes + i * 1024 (the layout
 * ipx_plan_run_dev_paletted takes).  *w, *h: 0, or the size the batch must have; on return the batch's size (the first image's, not
 * the logical screen's).  status[i]: IPX_OK, IPX_ERR_INVALID (Go's decoder fails on the file too) or IPX_ERR_UNSUPPORTED (a first
 * image not at (0, 0), an empty one, one of another size than the batch's or beyond ipx_frame_supported: the worker decodes those
 * with Go as before).  The frames of non-OK files are undefined; index == NULL when no file was decodable.  Free the frames with
 * ipx_gif_frames_free: stream-ordered allocations of `stream` (NULL: the context's default stream).  DESIGN.md section 4.8. */
typedef struct { uint8_t *index; int32_t stride; size_t frame_stride; uint8_t *palettes; } ipx_paletted_batch;
typedef struct ipx_gif_frames ipx_gif_frames;
int ipx_gif_decode_batch(ipx_ctx *ctx, void *stream, const ipx_bytes *gifs, int n, int *w, int *h, ipx_paletted_batch *frames,
                         int *status, ipx_gif_frames **owner);
void ipx_gif_frames_free(ipx_ctx *ctx, ipx_gif_frames *owner);
/* The same for n files of ANY sizes in one decode pass: one upload, one walk launch (the parallel walk plus the redo walk under
 * IPX_GIF_PAR=1) and one expand launch per scratch group (IPX_GIF_DEC_SCRATCH_MB), the files of a launch ordered longest data first.
 * frames[i] describes file i's frame: index 256-byte aligned with tight rows (stride = w), palette its 1024 bytes; all zero for a
 * non-OK file.  status[i] is exactly what ipx_gif_decode_batch gives that file in a call of its own with *w = *h = 0: no file is
 * IPX_ERR_UNSUPPORTED because of a neighbour.  IPX_GIF_PAR and ipx_gif_decode_counts mean what they mean there and count these files.
 * n == 0 is IPX_OK; more than 65535 files is IPX_ERR_UNSUPPORTED.  *owner is NULL when nothing decoded; it is freed with
 * ipx_gif_frames_free.  DESIGN.md section 4.8. */
typedef struct { int32_t w, h; uint8_t *index; int32_t stride; uint8_t *palette; } ipx_gif_frame;
int ipx_gif_decode_mixed(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, ipx_gif_frame *frames, int *status, ipx_gif_frames **owner);
/* The parallel code walk, with IPX_GIF_PAR=1 in the environment (read on every call that decodes GIF files; unset or anything else: the
 * serial walk alone, as before).  In every entry that decodes GIF files -- this one, ipx_plan_run_gif_gif and its _texts twin, the
 * pool's IPX_JOB_GIF, the micro-batcher -- the 64 lanes of the file's wave then read 64 consecutive codes at once: between two clear
 * codes the code at ordinal t is min(12, bitlen(eof + t)) bits wide whatever the codes' values, so its bit offset is a closed form of t
 * and the literal width; the strings' lengths follow by pointer jumping, the output offsets by a prefix sum.
 * That kernel accepts a file only at an EOF code that meets the reader's rules and decides no error: an invalid code or pixel value, a
 * string past the frame, data that end without an EOF code or an EOF code that comes early or breaks the sub-block rule hand the file,
 * by a per-file redo bit and without a host round trip, to the serial walk, so frames, palettes and statuses are byte for byte those
 * without the switch.
 * ipx_gif_decode_counts, since ipx_create: [0] files that entered the parallel walk, [1] files it finished itself, [2] files handed
 * to the serial walk by the redo bit ([0] = [1] + [2]), [3] code records written by the parallel lanes, over the files of [1] only.
 * All four stay 0 while the switch is unset. */
int ipx_gif_decode_counts(ipx_ctx *ctx, long long counts[4]);
/* The GIF task compressed in, compressed out: the uploads as the object store returns them, gif.Decode, every operator of the plan
 * (the plan's frame size is the batch's size), gif.Encode of the resize and thumbnail outputs and jpeg.Encode at `quality` of the
 * watermark output (watermark.go:66-79), all on the GPU; only compressed bytes cross the link.  status[i] as for
 * ipx_gif_decode_batch; outputs of non-OK files are {NULL, 0}.  Streams as for ipx_plan_run_host_paletted_gif (ipx_jpeg_result_free). */
int ipx_plan_run_gif_gif(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_bytes *files, int quality, ipx_bytes *resize_out,
                         ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);

/* ---- image.Decode for PNGs (decoder side) ---------------------------------------------
 * For a PNG upload image.Decode is png.Decode.  The host walks the chunk headers only (signature, IHDR, PLTE, tRNS, IDAT, IEND); the
 * whole files go up, and on the GPU the CRC of every chunk is checked in parallel pieces, the IDAT payloads are gathered into one zlib
 * stream per file, one wave per file inflates it with its Huffman tables, input and 32 KiB window in LDS, and a diagonal wavefront of
 * rows unfilters it and writes the frame layout of the type Go returns (IPX_PNG_*).  Adam7-interlaced files are taken only when
 * IPX_PNG_ADAM7=1 is set in the environment (read on every call; unset or anything else: IPX_ERR_UNSUPPORTED as before): then a wave per
 * pass unfilters the pass and puts its pixels where they belong, and the file decodes to the frame of its non-interlaced twin.
 *   IPX_PNG_GRAY     *image.Gray     1 byte per pixel     gray 1/2/4/8 without tRNS             -> ipx_plan_run_dev_gray
 *   IPX_PNG_NRGBA    *image.NRGBA    4                    gray 8 + tRNS, gray-alpha 8, RGB 8 + tRNS, RGBA 8 -> ipx_plan_run_dev_nrgba
 *   IPX_PNG_RGBA     *image.RGBA     4 (A = 0xff)         RGB 8 without tRNS                    -> ipx_plan_run_dev
 *   IPX_PNG_PALETTED *image.Paletted 1 + 256 x 4 palette  palette 1/2/4/8                       -> ipx_plan_run_dev_paletted
 *   IPX_PNG_GRAY16   *image.Gray16   2 (big-endian)       gray 16 without tRNS                  -> ipx_plan_run_dev_deep, IPX_DEEP_GRAY16
 *   IPX_PNG_RGBA64   *image.RGBA64   8 (A = 0xffff)       RGB 16 without tRNS                   -> _deep, IPX_DEEP_RGBA64
 *   IPX_PNG_NRGBA64  *image.NRGBA64  8                    gray 16 + tRNS, gray-alpha 16, RGB 16 + tRNS, RGBA 16 -> _deep, IPX_DEEP_NRGBA64
 * Frame i (file i) at pix + i * frame_stride, rows `stride` (w * bytes per pixel) bytes apart; for IPX_PNG_PALETTED the palettes at
 * palettes + i * 1024 (256 x (R, G, B, A), non-premultiplied: tRNS entries as color.NRGBA, entries past PLTE opaque black, as Go pads
 * them), else palettes == NULL.  *w, *h: 0, or the size the batch must have; *kind: -1, or the kind it must have; on return the batch's
 * size and kind (the first decodable file's).  status[i]: IPX_OK, IPX_ERR_INVALID (Go's decoder fails on the file too) or
 * IPX_ERR_UNSUPPORTED (Adam7 unless IPX_PNG_ADAM7=1, another chunk order, bytes after the zlib stream, sub-byte gray with tRNS, another size or kind than the
 * batch's, frames beyond ipx_frame_supported, ...: the worker decodes those with Go as before; the full list is in DESIGN.md section
 * 4.10).  The frames of non-OK files are undefined; pix == NULL when no file was decodable.  Free the frames with ipx_png_frames_free:
 * stream-ordered allocations of `stream` (NULL: the context's default stream). */
enum { IPX_PNG_GRAY = 0, IPX_PNG_NRGBA = 1, IPX_PNG_RGBA = 2, IPX_PNG_PALETTED = 3, IPX_PNG_GRAY16 = 4, IPX_PNG_RGBA64 = 5,
       IPX_PNG_NRGBA64 = 6 };
typedef struct { uint8_t *pix; int32_t stride; size_t frame_stride; uint8_t *palettes; } ipx_png_batch;
typedef struct ipx_png_frames ipx_png_frames;
int ipx_png_decode_batch(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, int *w, int *h, int *kind, ipx_png_batch *frames,
                         int *status, ipx_png_frames **owner);
void ipx_png_frames_free(ipx_ctx *ctx, ipx_png_frames *owner);
/* n files of any sizes and kinds in ONE decode pass: every file that parses is decoded in the same launches (one CRC pass, one
 * inflate, the unfilter) whatever its neighbours are.  frames[i] describes file i's frame in HBM: its size, its kind (IPX_PNG_*), pix
 * (256-byte aligned, rows tight, stride = w * bytes per pixel) and, for IPX_PNG_PALETTED, its 1024-byte palette (else NULL).
 * status[i] is what ipx_png_decode_batch gives the file in a batch of its own size and kind: no file is IPX_ERR_UNSUPPORTED because
 * of a neighbour.  frames[i] of a non-OK file is all zero.  IPX_PNG_ADAM7 and IPX_PNG_PAR mean what they mean there.  *owner (NULL
 * when nothing decoded) is freed with ipx_png_frames_free.  n == 0 is IPX_OK; more than 65535 files is IPX_ERR_UNSUPPORTED. */
typedef struct { int32_t w, h, kind; uint8_t *pix; int32_t stride; uint8_t *palette; } ipx_png_frame;
int ipx_png_decode_mixed(ipx_ctx *ctx, void *stream, const ipx_bytes *files, int n, ipx_png_frame *frames, int *status,
                         ipx_png_frames **owner);
/* The parallel inflate, with IPX_PNG_PAR=1 in the environment (read on every call that decodes PNG files; unset or anything else: the
 * serial inflate alone, as before).  In every entry that decodes PNG files -- this one, ipx_plan_run_png_png and its _texts twin, the
 * pool's IPX_JOB_PNG, the micro-batcher -- a Huffman block's body is then parsed by the 64 lanes of the file's wave side by side
 * (speculative starts at sub-sequence boundaries, rounds until the lanes fall into step).  That kernel decides
 * no error: a stream that breaks any rule, fails its Adler-32 or has bytes behind it is handed, by a per-file redo bit and without a host
 * round trip, to the serial decoder, so frames, palettes and statuses are byte for byte those without the switch.
 * ipx_png_decode_counts, since ipx_create: [0] files that entered the parallel kernel, [1] files it finished itself, [2] files handed
 * to the serial decoder by the redo bit ([0] = [1] + [2]), [3] tokens (literals, matches and end-of-block symbols, one each) decoded by
 * the parallel lanes and [4] tokens decoded by the wave-uniform loop inside that kernel (a sub-sequence whose output alone exceeds one
 * 16 KiB flush unit), both over the files of [1] only.  All five stay 0 while the switch is unset. */
int ipx_png_decode_counts(ipx_ctx *ctx, long long counts[5]);
/* The PNG task compressed in, compressed out: the uploads as the object store returns them, png.Decode, every operator of the plan
 * (the plan's frame size is the batch's size) and png.Encode of all three outputs (a PNG watermark stays PNG), all on the GPU; only
 * compressed bytes cross the link.  Files of any kind may be mixed: they are grouped by kind on the host, decoded in large groups
 * (IPX_HOST_CHUNK_PNG_DEC files, bounded by memory) and fed to the operators and the encoder in chunks of IPX_HOST_CHUNK_PNG.
 * status[i] as for ipx_png_decode_batch (Adam7 files: IPX_ERR_UNSUPPORTED unless IPX_PNG_ADAM7=1; the pool's IPX_JOB_PNG and the
 * micro-batcher go through this entry and answer alike); outputs of non-OK files are {NULL, 0}.  Streams as for ipx_plan_run_host_png
 * (ipx_jpeg_result_free). */
int ipx_plan_run_png_png(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_bytes *files, ipx_bytes *resize_out, ipx_bytes *thumb_out,
                         ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);

/* ---- the three compressed-in / compressed-out legs with a text per file ----------------------------------
 * As ipx_plan_run_jpeg_jpeg / _png_png / _gif_gif, with texts[i] drawn on files[i]'s watermark frame: the plan copies the frame
 * (it must have been created with glyphs == NULL; a plan that carries a glyph set is refused with IPX_ERR_INVALID) and one launch per
 * chunk of the leg draws every file's own text behind it (ipx_dev_composite_texts_rgba8), however many different texts the chunk
 * holds.  The texts are checked first (the rules of ipx_textset_create) and uploaded once per call (the JPEG leg: once per part).  A
 * plan without the watermark operator, or a null wm_out, checks the texts and draws nothing.  The resize and thumbnail streams are
 * those of the plain legs. */
int ipx_plan_run_jpeg_jpeg_texts(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                                 ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);
int ipx_plan_run_png_png_texts(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_bytes *files, const ipx_text *texts,
                               ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);
int ipx_plan_run_gif_gif_texts(ipx_ctx *ctx, const ipx_plan *plan, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                               ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);

/* ---- one process, several GPUs, asynchronous jobs ----------------------------------------------------------
 * The reference worker is ONE process whose goroutines pull independent messages (worker.go:88-96, 112-149); it scales by
 * running more consumers, nothing is exchanged (kafka/consumer.go:23).  A pool is that shape behind the C ABI: one context per
 * listed device (a device may be listed more than once), `lanes_per_device` feeder threads per context with a stream each, and ONE
 * queue of chunks ordered by cost, largest first, that every feeder pulls from when it is free -- a mixed-size batch balances itself
 * (work stealing falls out of pull scheduling), a uniform batch spreads evenly.  No data-path collective, no xGMI traffic.
 * Jobs are asynchronous: ipx_job_submit returns a ticket at once, so a goroutine does not hold an OS thread for the length of a batch.
 * cgo rule: frames, outputs, files and the status array of a job must stay valid (and, for Go, be C-allocated: ipx_pool_host_alloc)
 * until ipx_job_wait has returned; the operator description and its glyph masks are copied at submit. */
typedef struct ipx_pool ipx_pool;
typedef struct {
    int32_t lanes_per_device;   /* feeder threads (one stream each) per listed device; 0 = 4 (the reference's WORKER_CONCURRENCY is 3; four chunks in flight keep the host link busy) */
    size_t lane_bytes;          /* frames per chunk are sized to about this many bytes; 0 = 256 MiB */
} ipx_pool_config;
int ipx_pool_create(const int *devices, int n_devices, const ipx_pool_config *cfg, ipx_pool **out);
void ipx_pool_destroy(ipx_pool *pool);                        /* finishes what is queued, frees what was not released */
int ipx_pool_slots(const ipx_pool *pool);
long long ipx_pool_frames_done(const ipx_pool *pool, int slot); /* frames (files) slot `slot` has processed so far */
/* ipx_png_decode_counts of slot `slot`'s own context (the pool's IPX_JOB_PNG and the micro-batcher decode there): since ipx_pool_create */
int ipx_pool_png_decode_counts(const ipx_pool *pool, int slot, long long counts[5]);
/* ipx_gif_decode_counts of slot `slot`'s own context (the pool's IPX_JOB_GIF and the micro-batcher decode there): since ipx_pool_create */
int ipx_pool_gif_decode_counts(const ipx_pool *pool, int slot, long long counts[4]);
/* hipHostMalloc'd memory, allocated and first touched on a thread bound to the CPUs next to slot `slot`'s GPU (sysfs local_cpulist):
 * staging on the GPU's NUMA node.  Free with ipx_pool_host_free. */
void *ipx_pool_host_alloc(ipx_pool *pool, int slot, size_t bytes);
int ipx_pool_host_free(ipx_pool *pool, int slot, void *p);

/* The operators of a job, device independent (ipx_plan_params names a glyph set of ONE context): the same fields, with the
 * rasterised text as host masks.  Plans and uploaded glyph sets are cached per device by content. */
typedef struct {
    int32_t sw, sh;
    int32_t do_resize, resize_w, resize_h, keep_aspect;
    int32_t do_thumbnail, thumb_size, crop_to_fit;
    int32_t do_watermark;
    const ipx_glyph *glyphs;    /* may be NULL (copy only) */
    int32_t n_glyphs;
    uint8_t col[4];             /* parseColor's color.RGBA (watermark.go:93-97) */
} ipx_pool_ops;

/* A plan (and its uploaded glyph set) from the context's cache, keyed by content: what the per-operator entries and the pool use,
 * so that describing the operators per call costs no hipMalloc / hipFree in the steady state (each of those waits for every stream
 * of the device).  *cached = 1: the context owns the plan, and it stays valid at least until the caller hands it back; 0: every plan
 * of the full cache was in use and this one is the caller's for this call.  Either way hand it back with ipx_plan_release.  The
 * cache holds IPX_PLAN_CACHE_MAX (256) plans and replaces the least recently used one nobody holds. */
int ipx_plan_acquire(ipx_ctx *ctx, const ipx_pool_ops *ops, ipx_plan **plan, int *cached);
void ipx_plan_release(ipx_ctx *ctx, ipx_plan *plan, int cached);

/* The PNG task compressed in, compressed out for uploads of ANY sizes and kinds in one call.  ops gives the operator parameters;
 * ops->sw and ops->sh must be 0 (each file's own size is used) and ops->glyphs NULL (a positioned glyph list is anchored for one frame
 * size, watermark.go:121-148), else IPX_ERR_INVALID with nothing written.  texts: NULL (the watermark output is the plain copy), or n
 * texts, texts[i] positioned by the caller for file i's size (the rules of ipx_textset_create: more than 256 glyphs in any text refuses
 * the call).  The files are ordered by (width, height, kind) and decoded in groups of IPX_HOST_CHUNK_PNG_DEC files and ~4 GiB of
 * frames, each group in ONE decode pass; a group is cut into chunks of at most IPX_PNG_MIXED_CHUNK_MB (1024) of output frames and
 * encoder scratch; within a chunk the operators run once per run of one size and kind, with a plan of that size from the context's
 * cache (ipx_plan_acquire), and every present output is encoded by ONE mixed-size png.Encode over all frames of the chunk.
 * status[i] and the three streams of file i are exactly what ipx_plan_run_png_png (or _texts) returns for that file in a call of its
 * own with a plan of its size; files of a size for which no plan can be made get the status ipx_plan_create returned, alone.  A NULL
 * output array skips that output; an operator ops does not ask for gives {NULL, 0}; n == 0 is IPX_OK.  Streams as for
 * ipx_plan_run_png_png (ipx_jpeg_result_free).  DESIGN.md section 4.10. */
int ipx_run_png_png_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts,
                          ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);

/* The JPEG task compressed in, compressed out for uploads of ANY sizes and samplings in one call; the contract is
 * ipx_run_png_png_mixed's.  ops gives the operator parameters; ops->sw and ops->sh are ignored (each file's own size is used).
 * texts: NULL, or n texts, texts[i] positioned by the caller for file i's size and drawn as ipx_plan_run_jpeg_jpeg_texts draws it
 * (then ops->glyphs must be NULL, else IPX_ERR_INVALID with nothing written; the rules of ipx_textset_create: more than 256 glyphs in
 * any text refuses the call); without texts, a glyph list in ops is clipped against every size's frame as a plan of that size clips it.
 * The files are parsed once and decoded as ipx_jpeg_decode_mixed decodes them -- so here too the GPU scan walk (IPX_JPEG_PROG_GPU=1) is
 * not used, and 4:1:1, 4:1:0 and four-component files are IPX_ERR_UNSUPPORTED whatever IPX_JPEG_411 and IPX_JPEG_CMYK say.  The OK
 * files are ordered by (width, height, sampling class) and cut into decode groups of IPX_JPEG_MIXED_GROUP (256) files and ~4 GiB of
 * planes and coefficient scratch, each group ONE decode pass per sampling class; a group is cut into chunks of at most
 * IPX_JPEG_MIXED_CHUNK_MB (8192: the 256 files of a 1080p group in one chunk) of output frames and encoder scratch; within a chunk the operators run once per run of one size and
 * class, with a plan of that size from the context's cache (ipx_plan_acquire).  Every chunk is encoded once, with three waits for the
 * device: a chunk whose every present output has one size for every file (a resize without keep_aspect, a cropped thumbnail) as
 * ipx_jpeg_encode_batch_dev encodes one size, any other chunk by one mixed-size jpeg.Encode over every present output of its files
 * that are still IPX_OK (what ipx_jpeg_encode_mixed_dev runs).  status[i] and the three streams of file i are byte for byte what ipx_plan_run_jpeg_jpeg (or _texts) returns
 * for that file in a call of its own with a plan of its size and the same quality -- outside the three switches named above; files of a
 * size for which no plan can be made get the status ipx_plan_create returned, alone.  A NULL output array skips that output; an
 * operator ops does not ask for gives {NULL, 0}; n == 0 is IPX_OK; more than 65535 files is IPX_ERR_UNSUPPORTED.  Streams as for
 * ipx_plan_run_jpeg_jpeg (ipx_jpeg_result_free).  DESIGN.md sections 4.6 and 7. */
int ipx_run_jpeg_jpeg_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                            ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);

/* The GIF task compressed in, compressed out for uploads of ANY sizes in one call; the contract is ipx_run_jpeg_jpeg_mixed's.
 * ops->sw and ops->sh are ignored (each file's own size is used).  texts: NULL, or n texts as for that entry; texts together with
 * ops->glyphs is IPX_ERR_INVALID with nothing written.  The order of the refusals: a bad argument, more than 65535 files
 * (IPX_ERR_UNSUPPORTED), then the texts' own rules.  The files are parsed once and decoded as ipx_gif_decode_mixed decodes them.  The OK
 * files are ordered by size and cut into decode groups of IPX_GIF_MIXED_GROUP (256) files and ~4 GiB, each group ONE decode pass; a
 * group is cut into chunks of at most IPX_GIF_MIXED_CHUNK_MB (4096) of output frames and encoder scratch; within a chunk the
 * operators run once per run of one size with a plan of that size from the context's cache.  A file the walk failed is left out of
 * its run and out of every encode.  Every chunk is encoded once: ONE mixed-size gif.Encode (what ipx_gif_encode_mixed_dev runs) over
 * every resize and thumbnail frame of its files that are still IPX_OK, then jpeg.Encode at `quality` of the watermark frames
 * (watermark.go:66-79: a GIF watermark becomes a JPEG) -- as ipx_jpeg_encode_batch_dev encodes one size when every file of the chunk
 * is IPX_OK and has that output at one size, else by one mixed-size jpeg.Encode.  status[i] and the three streams of file i are byte for
 * byte what ipx_plan_run_gif_gif (or _texts) returns for that file in a call of its own, with a plan of its size and the same quality,
 * but for two cases, both per file: a size no plan can be made for gets ipx_plan_create's status, alone; a file whose resize or
 * thumbnail output would be 65536 or more on a side gets IPX_ERR_INVALID, alone (the uniform leg refuses the whole call).  A NULL
 * output array skips that output; an operator ops does not ask for gives {NULL, 0}; n == 0 is IPX_OK.  Streams as for
 * ipx_plan_run_gif_gif (ipx_jpeg_result_free).  DESIGN.md sections 4.8 and 7. */
int ipx_run_gif_gif_mixed(ipx_ctx *ctx, const ipx_pool_ops *ops, int n, const ipx_bytes *files, const ipx_text *texts, int quality,
                          ipx_bytes *resize_out, ipx_bytes *thumb_out, ipx_bytes *wm_out, int *status, ipx_jpeg_result **result);

enum { IPX_JOB_RGBA8 = 0,       /* decoded frames in, the operators' RGBA8 outputs back (what ipx_plan_run_host does) */
       IPX_JOB_JPEG = 1,        /* uploaded JPEG files in, three JPEG streams per file back (what ipx_plan_run_jpeg_jpeg does) */
       /* decoded frames of the other packed image types, Pix as Go holds it (src / sstride / src_frame_stride describe it), RGBA8
        * outputs back: what ipx_plan_run_host_nrgba / _gray / _deep do */
       IPX_JOB_NRGBA8 = 2, IPX_JOB_GRAY8 = 3,
       IPX_JOB_NRGBA64 = 4, IPX_JOB_RGBA64 = 5, IPX_JOB_GRAY16 = 6, IPX_JOB_CMYK = 7,
       /* uploaded PNG / GIF files in, three streams per file back (what ipx_plan_run_png_png / ipx_plan_run_gif_gif do): file jobs,
        * shaped like IPX_JOB_JPEG */
       IPX_JOB_PNG = 8, IPX_JOB_GIF = 9 };
typedef struct {
    int32_t kind;
    ipx_pool_ops ops;
    int32_t n;                  /* frames / files, all of size ops.sw x ops.sh */
    /* pixel jobs (every kind but the file jobs IPX_JOB_JPEG / _PNG / _GIF): frame i at src + i*src_frame_stride; an output pointer may be NULL to skip it */
    const uint8_t *src; int32_t sstride; size_t src_frame_stride;
    uint8_t *resize_out; size_t resize_frame_stride;
    uint8_t *thumb_out; size_t thumb_frame_stride;
    uint8_t *wm_out; size_t wm_frame_stride;
    /* file jobs (IPX_JOB_JPEG, IPX_JOB_PNG, IPX_JOB_GIF): n files of the job's format; n entries per output array (or NULL), pointing
     * into pinned blocks the pool owns until ipx_job_release; status[i] as the format's leg (ipx_plan_run_jpeg_jpeg / _png_png /
     * _gif_gif) reports it (files Go has to decode itself get IPX_ERR_UNSUPPORTED), preset to IPX_OK at submit; outputs of non-OK
     * files are {NULL, 0}.  The three output arrays keep their names for every format and hold streams of the job's format, as the
     * reference's operators end in the encoder of the upload's own format: a JPEG job three JPEG streams; a PNG job three PNG
     * streams; a GIF job a GIF (resize), a GIF (thumbnail) and a JPEG for the watermark (watermark.go:66-79).  `quality` is
     * jpeg.Options.Quality: a JPEG job's three outputs, a GIF job's watermark, ignored by a PNG job. */
    const ipx_bytes *files; int32_t quality;
    ipx_bytes *resize_jpeg, *thumb_jpeg, *wm_jpeg;
    int32_t *status;
    /* file jobs only: NULL, or n texts, texts[i] drawn on files[i]'s watermark frame (the job's chunks run the legs' _texts entries
     * with texts + i0).  Then ops.glyphs must be NULL (IPX_ERR_INVALID otherwise, as for a pixel job with texts: a text per decoded
     * frame is not offered); a text of more than 256 glyphs refuses the job (IPX_ERR_UNSUPPORTED).  Deep-copied at submit, like the
     * glyphs of ops.  NULL: the job as it always was. */
    const ipx_text *texts;
} ipx_job;
typedef uint64_t ipx_ticket;
int ipx_job_submit(ipx_pool *pool, const ipx_job *job, ipx_ticket *ticket);     /* returns at once */
int ipx_job_poll(ipx_pool *pool, ipx_ticket ticket, int *done);                 /* *done = 1 when ipx_job_wait would not block */
int ipx_job_wait(ipx_pool *pool, ipx_ticket ticket, int *frames_done);          /* blocks; the job's status (first failing chunk's) */
int ipx_job_release(ipx_pool *pool, ipx_ticket ticket);                         /* forgets the job, frees a file job's output blocks */
/* Synchronous convenience for pixel jobs: submit them all (mixed sizes welcome: the queue runs the largest first), wait, release. */
int ipx_pool_run_host(ipx_pool *pool, const ipx_job *jobs, int n_jobs);

/* ---- micro-batching of single uploads ---------------------------------------------------------------------------------------
 * The reference pulls ONE message per goroutine (internal/worker/worker.go:112-149) from a channel of concurrency * 2 (:88); what
 * turns those single files into GPU batches has to sit between the goroutines and the pool, and it sits here, below the ABI, so that
 * its policy is the library's (and tested) rather than every binding's.  ipx_batcher_submit takes ONE uploaded file -- JPEG, PNG or GIF, told apart by
 * the full signature as image.Decode does (the 8 bytes 89 50 4E 47 0D 0A 1A 0A; the 6 bytes GIF87a or GIF89a; anything else goes the
 * JPEG way and gets its status from that decoder) -- with the operators of its task (ops->sw x ops->sh = the frame size from the
 * file's header, image.DecodeConfig) and returns a ticket at once; files are grouped by format, frame size, JPEG shape (components
 * and luma sampling of the frame header: a JPEG batch is one shape; PNG files of every colour type and depth share a group, the leg
 * sorts them itself) and operator content (parameters, colour, every glyph's rectangle and mask bytes); a group goes to the pool as
 * one IPX_JOB_JPEG / IPX_JOB_PNG / IPX_JOB_GIF when it holds max_batch files or when its first file has waited max_wait_us.  The
 * streams of a result are those of the job's format (ipx_job).  For a GIF image.DecodeConfig reports the logical screen while the
 * leg goes by the first image: a file whose first image has another size gets IPX_ERR_UNSUPPORTED, alone.  ipx_batcher_wait blocks until
 * the ticket's group is done and fills the file's own result: status IPX_OK and three streams (NULL for operators the task did not ask
 * for), or IPX_ERR_UNSUPPORTED / IPX_ERR_INVALID for a file the GPU path does not decode -- its neighbours are not affected, the worker
 * runs its own image.Decode path for that message.  The streams live in blocks shared by the group: ipx_batcher_release hands a file's
 * share back (call it after fileRepo.SaveProcessed, image_processor.go:76), the blocks go with the group's last file.  At-least-once
 * delivery is unchanged: a goroutine commits its message only after its own ticket came back and its objects were saved.
 * cgo rule: the file bytes must stay valid (C-allocated for Go) until ipx_batcher_wait or ipx_batcher_release has returned for the
 * ticket; the operator description and its glyph masks are copied at submit.  Every entry is thread-safe.
 * IPX_BATCH_TEXTS=1 in the environment (read once, at ipx_batcher_create; unset or anything else: everything above, unchanged): the
 * grouping key stops before the colour and the glyphs -- format, frame size, JPEG shape and operator parameters stay in it -- so files
 * that differ only in their watermark text share a batch; each file keeps its own deep-copied text and the group goes out as one file
 * job with ops.glyphs = NULL and ipx_job.texts set.  A file whose text has more than 256 glyphs is then refused at ipx_batcher_submit
 * (IPX_ERR_UNSUPPORTED), alone, and never joins a group. */
typedef struct ipx_batcher ipx_batcher;
typedef struct {
    int32_t max_batch;      /* files per job; 0 = 256 (a part of ipx_plan_run_jpeg_jpeg) */
    int32_t max_wait_us;    /* how long the first file of a group may wait for company WHILE other jobs of this batcher run; 0 = 2000 */
    int32_t quality;        /* jpeg.Options.Quality of the JPEG outputs (a GIF's watermark among them); 0 = 85 (domain.DefaultJPEGQuality, task.go:57) */
} ipx_batcher_config;
typedef uint64_t ipx_batch_ticket;
typedef struct {
    int32_t status;               /* of this file: IPX_OK, or why the worker has to decode it itself */
    ipx_bytes resize, thumb, wm;  /* valid until ipx_batcher_release(ticket) */
} ipx_batch_result;
typedef struct {
    long long files, batches, flushed_by_size, flushed_by_timer, largest_batch, pending_files;
    long long flushed_when_idle;   /* groups that left at once because nothing of this batcher was running (a job finishing releases what
                                    * gathered while it ran): a lone file does not wait max_wait_us for company that is not coming */
} ipx_batcher_stats;
int ipx_batcher_create(ipx_pool *pool, const ipx_batcher_config *cfg, ipx_batcher **out);
void ipx_batcher_destroy(ipx_batcher *b);     /* flushes what is pending, waits for it, frees what was not released */
int ipx_batcher_submit(ipx_batcher *b, const ipx_bytes *file, const ipx_pool_ops *ops, ipx_batch_ticket *ticket);
int ipx_batcher_wait(ipx_batcher *b, ipx_batch_ticket ticket, ipx_batch_result *res);
int ipx_batcher_release(ipx_batcher *b, ipx_batch_ticket ticket);
int ipx_batcher_get_stats(ipx_batcher *b, ipx_batcher_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* IPX_H */
