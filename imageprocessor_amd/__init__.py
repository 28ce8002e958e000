"""imageprocessor_amd -- MI355X-native pixel worker for ImageProcessor's resize / thumbnail /
watermark path.  This module is a thin numpy/ctypes front end of the C ABI in include/ipx.h;
all pixel work runs in the hand-written HIP kernels of csrc/ (there is no CPU fallback)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Config, Glyph, PlanInfo, PlanParams, Rect

OP_OVER = 0
DEEP_NRGBA64, DEEP_RGBA64, DEEP_GRAY16, DEEP_CMYK = 0, 1, 2, 3   # ipx.h IPX_DEEP_*
PNG_GRAY, PNG_NRGBA, PNG_RGBA, PNG_PALETTED, PNG_GRAY16, PNG_RGBA64, PNG_NRGBA64 = range(7)   # ipx.h IPX_PNG_*
OP_SRC = 1
# ipx.h IPX_YCBCR_* / IPX_GRAY: 0..3 are image.YCbCrSubsampleRatio's own values, 411 and 410 are not (Go: 4 and 5)
YCBCR_444, YCBCR_422, YCBCR_420, YCBCR_440, GRAY, YCBCR_411, YCBCR_410 = range(7)


class IpxError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("ipx status %d: %s" % (status, text))
        self.status = status
        self.text = text


def lib():
    return _lib.load()


def _check(rc):
    if rc < 0:
        raise IpxError(rc, lib().ipx_last_error().decode(errors="replace"))
    return rc


def _rect(r):
    return r if isinstance(r, Rect) else Rect(*[int(v) for v in r])


def _bytes_array(files):
    """ipx_bytes[max(n, 1)] over the byte strings in `files`; the array keeps them alive"""
    keep = [bytes(f) for f in files]
    arr = (_lib.Bytes * max(len(keep), 1))()
    for i, f in enumerate(keep):
        arr[i].data = C.cast(C.c_char_p(f), C.c_void_p)
        arr[i].len = len(f)
    arr._keep = keep
    return arr


def _rows(a):
    """-> (uint8 array, row stride in bytes): `a` itself when its rows are contiguous and strides[0] covers a row -- a window of a
    larger array, which is what an image's SubImage is --, a packed copy otherwise"""
    a = np.asarray(a, dtype=np.uint8)
    row = int(np.prod(a.shape[1:]))
    if a.ndim < 2 or not a[:1].flags.c_contiguous or (a.shape[0] > 1 and a.strides[0] < row):
        a = np.ascontiguousarray(a)
    return a, (a.strides[0] if a.shape[0] > 1 else row)


def _frame(a):
    """an RGBA8 source frame -> (array, row stride)"""
    a, stride = _rows(a)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("RGBA8 frame must be H x W x 4")
    return a, stride


def _dst(dst, shape=None):
    """a destination frame is written in place: H x W x 4 uint8 with contiguous rows -> its row stride"""
    assert isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.ndim == 3 and dst.shape[2] == 4 and dst.flags.writeable
    assert shape is None or dst.shape == shape
    d, stride = _rows(dst)
    assert d is dst, "the destination's rows must be contiguous and strides[0] at least a row"
    return stride


# ---- host-only rules (no GPU needed) ------------------------------------------------------------

def resize_dims(ow, oh, w, h, keep_aspect):
    nw, nh = C.c_int(), C.c_int()
    _check(lib().ipx_resize_dims(ow, oh, w, h, int(bool(keep_aspect)), C.byref(nw), C.byref(nh)))
    return nw.value, nh.value


def thumb_geometry(ow, oh, size, crop_to_fit):
    r, nw, nh = Rect(), C.c_int(), C.c_int()
    _check(lib().ipx_thumb_geometry(ow, oh, size, int(bool(crop_to_fit)), C.byref(r), C.byref(nw),
                                    C.byref(nh)))
    return (r.x0, r.y0, r.x1, r.y1), nw.value, nh.value


def text_height_px(font_size):
    return lib().ipx_text_height_px(float(font_size))


def watermark_anchor(position, w, h, width_px, height_px):
    px, py = C.c_int(), C.c_int()
    _check(lib().ipx_watermark_anchor(position.encode(), w, h, width_px, height_px, C.byref(px),
                                      C.byref(py)))
    return px.value, py.value


def parse_color(s, opacity):
    out = (C.c_uint8 * 4)()
    rc = _check(lib().ipx_parse_color(s.encode(), float(opacity), out))
    return tuple(out), rc == 1


def device_count():
    return lib().ipx_device_count()


def _glyph_array(glyphs):
    keep = []
    arr = (Glyph * max(1, len(glyphs)))()
    for i, g in enumerate(glyphs):
        m, mstride = _rows(g["mask"])
        if m.ndim != 2:
            raise ValueError("glyph mask must be mh x mw")
        keep.append(m)
        mp = g.get("mp", (0, 0))
        arr[i] = Glyph(m.ctypes.data, m.shape[1], m.shape[0], mstride, _rect(g["dr"]), int(mp[0]),
                       int(mp[1]))
    return arr, keep


def _text_array(texts):
    """texts: one (glyphs, col) pair per file or frame -> (ipx_text array, what it points into)"""
    keep = []
    arr = (_lib.Text * max(1, len(texts)))()
    for i, (glyphs, col) in enumerate(texts):
        glyphs = list(glyphs)
        ga, gk = _glyph_array(glyphs)
        keep.append((ga, gk))
        arr[i].glyphs = ga if glyphs else None
        arr[i].n_glyphs = len(glyphs)
        for c in range(4):
            arr[i].col[c] = int(col[c])
    return arr, keep


def _texts_for(texts, n):
    """texts: None, or one (glyphs, col) per file -> (ipx_text array | None, what it points into)"""
    if texts is None:
        return None, None
    texts = list(texts)
    if len(texts) != n:
        raise ValueError("one text per file")
    return _text_array(texts)


def _pool_ops(ops, glyph_list=False):
    """ops: a PoolOps, taken as it is, or dict(resize=(w, h, keep_aspect) | None, thumbnail=(size, crop_to_fit) | None, watermark=bool)
    -> (PoolOps with sw = sh = 0, what it points into).  glyph_list: watermark=(glyphs, col) puts that glyph list into the PoolOps;
    where it is False such a pair means no more than True."""
    if not isinstance(ops, dict):
        return ops, None
    o, keep = _lib.PoolOps(), None
    if ops.get("resize"):
        o.do_resize, o.resize_w, o.resize_h, o.keep_aspect = 1, ops["resize"][0], ops["resize"][1], int(bool(ops["resize"][2]))
    if ops.get("thumbnail"):
        o.do_thumbnail, o.thumb_size, o.crop_to_fit = 1, ops["thumbnail"][0], int(bool(ops["thumbnail"][1]))
    wm = ops.get("watermark")
    o.do_watermark = int(bool(wm))
    if glyph_list and isinstance(wm, (tuple, list)):
        glyphs, col = list(wm[0]), wm[1]
        keep = _glyph_array(glyphs)
        o.glyphs, o.n_glyphs = keep[0], len(glyphs)
        for c in range(4):
            o.col[c] = int(col[c])
    return o, keep


def _streams(arrs, n, copy):
    """{operator: the ipx_bytes array a compressed-out entry filled} -> {operator: [bytes | None] * n}: None for a slot the entry left
    unpublished; copy=False: the stream's length instead of its bytes"""
    return {k: [(C.string_at(a[j].data, a[j].len) if copy else a[j].len) if a[j].data else None for j in range(n)] for k, a in arrs.items()}


# ---- GPU objects -------------------------------------------------------------------------------------

class DevBuffer:
    """hipMalloc'd bytes owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        self.ptr = lib().ipx_dev_alloc(ctx.handle, max(1, self.nbytes))
        if not self.ptr:
            raise IpxError(-2, lib().ipx_last_error().decode())

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        _check(lib().ipx_memcpy_h2d(self.ctx.handle, self.ptr + offset, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype=np.uint8, offset=0):
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        _check(lib().ipx_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr + offset, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().ipx_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GlyphSet:
    """Rasterised watermark text (A8 masks + DrawMask rectangles) resident in HBM."""

    def __init__(self, ctx, glyphs, col):
        self.ctx = ctx
        arr, keep = _glyph_array(list(glyphs))
        c = (C.c_uint8 * 4)(*[int(v) for v in col])
        h = C.c_void_p()
        _check(lib().ipx_glyphset_create(ctx.handle, arr, len(glyphs), c, C.byref(h)))
        self.handle = h.value

    def close(self):
        if self.handle:
            lib().ipx_glyphset_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TextSet:
    """One text per frame of a batch, clipped for w x h frames and resident in HBM (ipx_textset_*).  texts: (glyphs, col) pairs."""

    def __init__(self, ctx, texts, w, h, stream=None):
        self.ctx = ctx
        texts = list(texts)
        arr, keep = _text_array(texts)
        hd = C.c_void_p()
        _check(lib().ipx_textset_create(ctx.handle, stream, arr, len(texts), int(w), int(h), C.byref(hd)))
        self.handle, self.n, self.w, self.h = hd.value, len(texts), int(w), int(h)

    def close(self):
        if self.handle:
            lib().ipx_textset_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """Fused resize + thumbnail + watermark for frames of one size (ipx_plan_*)."""

    def __init__(self, ctx, sw, sh, resize=(1024, 768, True), thumbnail=(200, True), watermark=None):
        """resize=(w, h, keep_aspect) | None; thumbnail=(size, crop_to_fit) | None;
        watermark=None (operator absent) | False/GlyphSet-less copy (True) | GlyphSet."""
        self.ctx = ctx
        self._sw, self._sh = sw, sh
        p = PlanParams()
        p.sw, p.sh = sw, sh
        if resize:
            p.do_resize, p.resize_w, p.resize_h, p.keep_aspect = 1, resize[0], resize[1], int(bool(resize[2]))
        if thumbnail:
            p.do_thumbnail, p.thumb_size, p.crop_to_fit = 1, thumbnail[0], int(bool(thumbnail[1]))
        self._gs = None
        if watermark is not None and watermark is not False:
            p.do_watermark = 1
            if isinstance(watermark, GlyphSet):
                self._gs = watermark
                p.glyphs = watermark.handle
        h = C.c_void_p()
        _check(lib().ipx_plan_create(ctx.handle, C.byref(p), C.byref(h)))
        self.handle = h.value
        self.info = PlanInfo()
        _check(lib().ipx_plan_query(self.handle, C.byref(self.info)))

    def _run(self, entry, head, n, src, ptrs, strides=(None, None, None)):
        """One pixel-out entry.  head: () for frames in host memory, (stream,) for frames in HBM; src: the entry's source arguments;
        ptrs: the addresses of the resize, thumbnail and watermark outputs (None: not wanted); strides: their frame strides
        (None: tightly packed)."""
        i = self.info
        fs = [d if s is None else s for s, d in zip(strides, (i.resize_bytes, i.thumb_bytes, i.wm_bytes))]
        _check(entry(self.ctx.handle, *head, self.handle, n, *src, ptrs[0], fs[0], ptrs[1], fs[1], ptrs[2], fs[2]))

    def _run_host(self, entry, n, src, want, out=None):
        """A host entry: arrays for the wanted outputs the plan has (those in `out` are used as they are), the call, the dict."""
        i = self.info
        out = dict(out) if out else {}
        for k, nbytes, h, w in (("resize", i.resize_bytes, i.resize_h, i.resize_w), ("thumbnail", i.thumb_bytes, i.thumb_h, i.thumb_w),
                                ("watermark", i.wm_bytes, i.wm_h, i.wm_w)):
            if k in want and nbytes and k not in out:
                out[k] = np.empty((n, h, w, 4), np.uint8)
        self._run(entry, (), n, src, [out[k].ctypes.data if k in out else None for k in ("resize", "thumbnail", "watermark")])
        return out

    def run_dev(self, n, src_ptr, resize_ptr=None, thumb_ptr=None, wm_ptr=None, stream=None,
                sstride=None, src_frame_stride=None, resize_frame_stride=None,
                thumb_frame_stride=None, wm_frame_stride=None):
        sstride = self._sw * 4 if sstride is None else sstride
        self._run(lib().ipx_plan_run_dev, (stream,), n,
                  (src_ptr, sstride, sstride * self._sh if src_frame_stride is None else src_frame_stride),
                  (resize_ptr, thumb_ptr, wm_ptr), (resize_frame_stride, thumb_frame_stride, wm_frame_stride))

    def run_host(self, frames, want=("resize", "thumbnail", "watermark"), out=None):
        """frames: n x H x W x 4 uint8 (host).  Returns dict of output batches (`out` may supply
        preallocated, e.g. pinned, arrays)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        return self._run_host(lib().ipx_plan_run_host, frames.shape[0], (frames.ctypes.data, self._sw * 4, self._sw * self._sh * 4), want, out)

    def run_host_nrgba(self, frames, want=("resize", "thumbnail", "watermark")):
        """frames: n x H x W x 4 uint8, non-premultiplied (*image.NRGBA, host) -> dict of output batches"""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        return self._run_host(lib().ipx_plan_run_host_nrgba, frames.shape[0], (frames.ctypes.data, self._sw * 4, self._sw * self._sh * 4), want)

    def run_host_deep(self, pix, kind, want=("resize", "thumbnail", "watermark")):
        """pix: n x H x (W * bpp) uint8, Go's Pix rows of *image.NRGBA64 / RGBA64 / Gray16 / CMYK frames (kind: DEEP_*, host)"""
        pix = np.ascontiguousarray(pix, dtype=np.uint8)
        return self._run_host(lib().ipx_plan_run_host_deep, pix.shape[0], (kind, pix.ctypes.data, pix.shape[2], pix.shape[1] * pix.shape[2]), want)

    def run_host_gray(self, frames, want=("resize", "thumbnail", "watermark")):
        """frames: n x H x W uint8 (*image.Gray, host) -> dict of output batches"""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        return self._run_host(lib().ipx_plan_run_host_gray, frames.shape[0], (frames.ctypes.data, self._sw, self._sw * self._sh), want)

    def run_host_paletted(self, index, palettes, want=("resize", "thumbnail", "watermark")):
        """index: n x H x W uint8, palettes: n x 256 x 4 uint8 (R, G, B, A) non-premultiplied (*image.Paletted, host)"""
        index = np.ascontiguousarray(index, dtype=np.uint8)
        palettes = np.ascontiguousarray(palettes, dtype=np.uint8)
        n = index.shape[0]
        assert palettes.shape == (n, 256, 4)
        return self._run_host(lib().ipx_plan_run_host_paletted, n, (index.ctypes.data, self._sw, self._sw * self._sh, palettes.ctypes.data), want)

    def _run_streams(self, entry, n, want, copy, args, status=None):
        """One compressed-out entry: output arrays for the wanted outputs the plan has, the call (args go between the plan and the
        arrays), then per output the streams (their lengths when copy=False; None for a slot the entry left unpublished); the
        result is freed."""
        i = self.info
        arrs = {k: (_lib.Bytes * max(n, 1))() for k, present in (("resize", i.resize_bytes), ("thumbnail", i.thumb_bytes),
                                                                  ("watermark", i.wm_bytes)) if k in want and present}
        res = C.c_void_p()
        extra = () if status is None else (status,)
        _check(entry(self.ctx.handle, self.handle, n, *args, arrs.get("resize"), arrs.get("thumbnail"), arrs.get("watermark"), *extra,
                     C.byref(res)))
        out = _streams(arrs, n, copy)
        lib().ipx_jpeg_result_free(self.ctx.handle, res)
        return out

    def _run_files(self, entry, files, want, copy, args=()):
        """A file-in entry: ({operator: [bytes | None] * n}, status list)."""
        n = len(files)
        status = (C.c_int * max(n, 1))()
        out = self._run_streams(entry, n, want, copy, (_bytes_array(files),) + args, status)
        return out, list(status)[:n]

    def run_host_jpeg(self, frames, quality=85, want=("resize", "thumbnail", "watermark"), copy=True):
        """frames: n x H x W x 4 uint8 (host, ideally pinned) -> {operator: [jpeg bytes] * n}: operators and jpeg.Encode on
        the GPU, only the streams come back.  copy=False: lengths only (the streams are released unread; for timing)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        return self._run_streams(lib().ipx_plan_run_host_jpeg, frames.shape[0], want, copy,
                                 (frames.ctypes.data, self._sw * 4, self._sw * self._sh * 4, int(quality)))

    def run_host_paletted_gif(self, index, palettes, quality=85, want=("resize", "thumbnail", "watermark"), copy=True):
        """Decoded GIF frames (index: n x H x W uint8, palettes: n x 256 x 4 uint8, host) -> {operator: [bytes] * n}: operators,
        gif.Encode of resize / thumbnail and jpeg.Encode (at `quality`) of the watermark on the GPU; only the streams come back."""
        index = np.ascontiguousarray(index, dtype=np.uint8)
        palettes = np.ascontiguousarray(palettes, dtype=np.uint8)
        n = index.shape[0]
        assert index.shape[1:] == (self._sh, self._sw) and palettes.shape == (n, 256, 4)
        return self._run_streams(lib().ipx_plan_run_host_paletted_gif, n, want, copy,
                                 (index.ctypes.data, self._sw, self._sw * self._sh, palettes.ctypes.data, int(quality)))

    def run_host_png(self, frames, want=("resize", "thumbnail", "watermark"), copy=True):
        """frames: n x H x W x 4 uint8 (host) -> {operator: [png bytes] * n}: operators and png.Encode of every output on the GPU, only
        the streams come back.  copy=False: lengths only (the streams are released unread; for timing)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        assert frames.shape[1:] == (self._sh, self._sw, 4)
        return self._run_streams(lib().ipx_plan_run_host_png, frames.shape[0], want, copy,
                                 (frames.ctypes.data, self._sw * 4, self._sw * self._sh * 4))

    def run_host_ycbcr_jpeg(self, y, cb, cr, ratio, quality=85, want=("resize", "thumbnail", "watermark"), copy=True):
        """Decoded JPEG planes (host) -> {operator: [jpeg bytes] * n}; see run_host_jpeg."""
        y, cb, cr = (np.ascontiguousarray(a, dtype=np.uint8) for a in (y, cb, cr))
        n, h, w = y.shape
        assert (w, h) == (self._sw, self._sh) and cb.shape == cr.shape and cb.shape[0] == n
        b = _lib.YCbCrBatch(y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, cb.shape[2], h * w, cb.shape[1] * cb.shape[2], int(ratio))
        return self._run_streams(lib().ipx_plan_run_host_ycbcr_jpeg, n, want, copy, (C.byref(b), int(quality)))

    def _run_files_texts(self, entry, files, texts, want, copy, args=()):
        """A file-in entry with texts[i] = (glyphs, col) drawn on file i's watermark (the plan must be copy-only: watermark=True)."""
        n = len(files)
        arr, keep = _texts_for(texts, n)
        status = (C.c_int * max(n, 1))()
        out = self._run_streams(entry, n, want, copy, (_bytes_array(files), arr) + args, status)
        return out, list(status)[:n]

    def run_jpeg_jpeg(self, files, quality=85, want=("resize", "thumbnail", "watermark"), copy=True, texts=None):
        """JPEG byte strings in -> ({operator: [jpeg bytes | None] * n}, status list): decode, operators, encode on the GPU.
        texts: None, or one (glyphs, col) per file (ipx_plan_run_jpeg_jpeg_texts)."""
        if texts is not None:
            return self._run_files_texts(lib().ipx_plan_run_jpeg_jpeg_texts, files, texts, want, copy, (int(quality),))
        return self._run_files(lib().ipx_plan_run_jpeg_jpeg, files, want, copy, (int(quality),))

    def run_gif_gif(self, files, quality=85, want=("resize", "thumbnail", "watermark"), copy=True, texts=None):
        """GIF byte strings in -> ({operator: [bytes | None] * n}, status list): gif.Decode, operators, gif.Encode of resize / thumbnail
        and jpeg.Encode (at `quality`) of the watermark on the GPU.  texts: None, or one (glyphs, col) per file."""
        if texts is not None:
            return self._run_files_texts(lib().ipx_plan_run_gif_gif_texts, files, texts, want, copy, (int(quality),))
        return self._run_files(lib().ipx_plan_run_gif_gif, files, want, copy, (int(quality),))

    def run_png_png(self, files, want=("resize", "thumbnail", "watermark"), copy=True, texts=None):
        """PNG byte strings of any kind in -> ({operator: [png bytes | None] * n}, status list): png.Decode, operators and png.Encode of
        every output on the GPU.  texts: None, or one (glyphs, col) per file."""
        if texts is not None:
            return self._run_files_texts(lib().ipx_plan_run_png_png_texts, files, texts, want, copy)
        return self._run_files(lib().ipx_plan_run_png_png, files, want, copy)

    def run_dev_nrgba(self, n, src_ptr, resize_ptr=None, thumb_ptr=None, wm_ptr=None, stream=None,
                      sstride=None, src_frame_stride=None, resize_frame_stride=None,
                      thumb_frame_stride=None, wm_frame_stride=None):
        """*image.NRGBA frames resident in HBM, tightly packed unless the strides say otherwise (ipx_plan_run_dev_nrgba)"""
        sstride = self._sw * 4 if sstride is None else sstride
        self._run(lib().ipx_plan_run_dev_nrgba, (stream,), n,
                  (src_ptr, sstride, sstride * self._sh if src_frame_stride is None else src_frame_stride),
                  (resize_ptr, thumb_ptr, wm_ptr), (resize_frame_stride, thumb_frame_stride, wm_frame_stride))

    def run_dev_deep(self, n, kind, src_ptr, stride, frame_stride, resize_ptr=None, thumb_ptr=None, wm_ptr=None, stream=None,
                     resize_frame_stride=None, thumb_frame_stride=None, wm_frame_stride=None):
        """*image.NRGBA64 / RGBA64 / Gray16 / CMYK frames (Go's Pix) resident in HBM (ipx_plan_run_dev_deep)"""
        self._run(lib().ipx_plan_run_dev_deep, (stream,), n, (kind, src_ptr, stride, frame_stride), (resize_ptr, thumb_ptr, wm_ptr),
                  (resize_frame_stride, thumb_frame_stride, wm_frame_stride))

    def run_dev_gray(self, n, gray_ptr, stride, frame_stride, resize_ptr=None, thumb_ptr=None, wm_ptr=None, stream=None,
                     resize_frame_stride=None, thumb_frame_stride=None, wm_frame_stride=None):
        """*image.Gray frames resident in HBM (ipx_plan_run_dev_gray)"""
        self._run(lib().ipx_plan_run_dev_gray, (stream,), n, (gray_ptr, stride, frame_stride), (resize_ptr, thumb_ptr, wm_ptr),
                  (resize_frame_stride, thumb_frame_stride, wm_frame_stride))

    def run_dev_paletted(self, n, index_ptr, stride, frame_stride, palettes_ptr, resize_ptr=None, thumb_ptr=None, wm_ptr=None, stream=None,
                         resize_frame_stride=None, thumb_frame_stride=None, wm_frame_stride=None):
        """*image.Paletted frames resident in HBM: index bytes plus 256 x (R, G, B, A) per frame (ipx_plan_run_dev_paletted)"""
        self._run(lib().ipx_plan_run_dev_paletted, (stream,), n, (index_ptr, stride, frame_stride, palettes_ptr), (resize_ptr, thumb_ptr, wm_ptr),
                  (resize_frame_stride, thumb_frame_stride, wm_frame_stride))

    def run_dev_ycbcr(self, n, y_ptr, cb_ptr, cr_ptr, ratio, ystride, cstride, y_frame_stride, c_frame_stride,
                      resize_ptr=None, thumb_ptr=None, wm_ptr=None, stream=None,
                      resize_frame_stride=None, thumb_frame_stride=None, wm_frame_stride=None):
        b = _lib.YCbCrBatch(y_ptr, cb_ptr, cr_ptr, ystride, cstride, y_frame_stride, c_frame_stride, int(ratio))
        self._run(lib().ipx_plan_run_dev_ycbcr, (stream,), n, (C.byref(b),), (resize_ptr, thumb_ptr, wm_ptr),
                  (resize_frame_stride, thumb_frame_stride, wm_frame_stride))

    def run_host_ycbcr(self, y, cb, cr, ratio, want=("resize", "thumbnail", "watermark")):
        """A batch of decoded JPEG frames: y n x H x W, cb / cr n x CH x CW uint8 (image.YCbCr planes)."""
        y, cb, cr = (np.ascontiguousarray(a, dtype=np.uint8) for a in (y, cb, cr))
        n, h, w = y.shape
        assert (w, h) == (self._sw, self._sh) and cb.shape == cr.shape and cb.shape[0] == n
        b = _lib.YCbCrBatch(y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, cb.shape[2], h * w,
                            cb.shape[1] * cb.shape[2], int(ratio))
        return self._run_host(lib().ipx_plan_run_host_ycbcr, n, (C.byref(b),), want)

    def close(self):
        if self.handle:
            lib().ipx_plan_destroy(self.ctx.handle, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One per process and GPU (ipx_create)."""

    def __init__(self, device=-1, lanes=0, lane_bytes=0):
        cfg = Config(device, lanes, lane_bytes)
        h = C.c_void_p()
        _check(lib().ipx_create(C.byref(cfg), C.byref(h)))
        self.handle = h.value

    def close(self):
        if self.handle:
            lib().ipx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def alloc(self, nbytes):
        return DevBuffer(self, nbytes)

    def host_alloc(self, shape, dtype=np.uint8):
        """Pinned (hipHostMalloc) staging as a numpy array; free with host_free(arr)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = lib().ipx_host_alloc(self.handle, max(1, n))
        if not p:
            raise IpxError(-2, lib().ipx_last_error().decode())
        arr = np.frombuffer((C.c_uint8 * n).from_address(p), dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            lib().ipx_host_free(self.handle, p)

    def stream(self):
        """A stream of the caller's own for the asynchronous device-pointer entries (free with stream_destroy)."""
        st = lib().ipx_stream_create(self.handle)
        if not st:
            raise IpxError(-3, lib().ipx_last_error().decode())
        return st

    def stream_destroy(self, st):
        _check(lib().ipx_stream_destroy(self.handle, st))

    def sync(self, stream=None):
        _check(lib().ipx_stream_sync(self.handle, stream))

    def device_sync(self):
        _check(lib().ipx_device_sync(self.handle))

    def copy_d2d(self, dst_ptr, src_ptr, nbytes):
        _check(lib().ipx_memcpy_d2d(self.handle, dst_ptr, src_ptr, nbytes))

    def link_probe(self, up_bytes, down_bytes, reps=3):
        """-> {"up", "down", "up_while_down", "down_while_up"} in GB/s: what pinned copies get from the host link on this box"""
        out = (C.c_double * 4)()
        _check(lib().ipx_link_probe(self.handle, int(up_bytes), int(down_bytes), int(reps), C.byref(out)))
        return {"up": round(out[0], 2), "down": round(out[1], 2), "up_while_down": round(out[2], 2), "down_while_up": round(out[3], 2)}

    def stream_copy(self, dst_ptr, src_ptr, nbytes, stream=None):
        """A plain streaming copy kernel: what this box's HBM gives a copy (bench.py's copy_ceiling)."""
        _check(lib().ipx_stream_copy(self.handle, stream, dst_ptr, src_ptr, nbytes))

    def timed(self, fn, stream=None):
        """Runs fn() bracketed by HIP events on `stream`; returns milliseconds (syncs)."""
        L = lib()
        e0, e1 = L.ipx_event_create(self.handle), L.ipx_event_create(self.handle)
        try:
            _check(L.ipx_event_record(self.handle, e0, stream))
            fn()
            _check(L.ipx_event_record(self.handle, e1, stream))
            ms = C.c_float()
            _check(L.ipx_event_elapsed_ms(self.handle, e0, e1, C.byref(ms)))
            return ms.value
        finally:
            L.ipx_event_destroy(self.handle, e0)
            L.ipx_event_destroy(self.handle, e1)

    def glyphset(self, glyphs, col):
        return GlyphSet(self, glyphs, col)

    def textset(self, texts, w, h, stream=None):
        return TextSet(self, texts, w, h, stream)

    def plan(self, sw, sh, **kw):
        return Plan(self, sw, sh, **kw)

    # ---- per-operation seam on frames in HBM (asynchronous on `stream`; null: the context's) ----------
    def dev_scale_bilinear(self, dst_ptr, dw, dh, dstride, dr, src_ptr, sw, sh, sstride, sr, op=OP_OVER, stream=None):
        """xdraw.BiLinear.Scale on RGBA8 frames resident in HBM (ipx_dev_scale_bilinear_rgba8)"""
        _check(lib().ipx_dev_scale_bilinear_rgba8(self.handle, stream, dst_ptr, dw, dh, dstride, _rect(dr), src_ptr, sw, sh, sstride,
                                                  _rect(sr), op))

    def dev_draw(self, dst_ptr, dw, dh, dstride, r, src_ptr, sw, sh, sstride, sp=(0, 0), op=OP_SRC, stream=None):
        """draw.Draw on RGBA8 frames resident in HBM (ipx_dev_draw_rgba8)"""
        _check(lib().ipx_dev_draw_rgba8(self.handle, stream, dst_ptr, dw, dh, dstride, _rect(r), src_ptr, sw, sh, sstride,
                                        int(sp[0]), int(sp[1]), op))

    def dev_composite_glyphs(self, dst_ptr, dw, dh, dstride, glyphset, stream=None):
        """the text of a GlyphSet onto one RGBA8 frame resident in HBM (ipx_dev_composite_glyphs_rgba8)"""
        _check(lib().ipx_dev_composite_glyphs_rgba8(self.handle, stream, dst_ptr, dw, dh, dstride, glyphset.handle))

    def dev_composite_texts(self, dst_ptr, w, h, dstride, frame_stride, n_frames, textset, first=0, map=None, stream=None):
        """frame z of n_frames RGBA8 frames in HBM gets text map[z] (first + z without a map) of a TextSet, in one launch
        (ipx_dev_composite_texts_rgba8)"""
        m = None if map is None else (C.c_int32 * max(1, len(map)))(*[int(v) for v in map])
        _check(lib().ipx_dev_composite_texts_rgba8(self.handle, stream, dst_ptr, w, h, dstride, frame_stride, n_frames, textset.handle,
                                                   int(first), m))

    # ---- per-operation seam on host arrays (synchronous) ----------------------------------------
    def scale_bilinear(self, src, dw, dh, sr=None, dr=None, op=OP_OVER, dst=None):
        """xdraw.BiLinear.Scale(dst, dr, src, sr, op, nil); dst defaults to a zeroed frame."""
        src, sstride = _frame(src)
        sh, sw = src.shape[:2]
        if dst is None:
            dst = np.zeros((dh, dw, 4), np.uint8)
        dstride = _dst(dst, (dh, dw, 4))
        _check(lib().ipx_scale_bilinear_rgba8(
            self.handle, dst.ctypes.data, dw, dh, dstride, _rect(dr if dr is not None else (0, 0, dw, dh)),
            src.ctypes.data, sw, sh, sstride, _rect(sr if sr is not None else (0, 0, sw, sh)), op))
        return dst

    def draw(self, dst, r, src, sp=(0, 0), op=OP_SRC):
        src, sstride = _frame(src)
        dstride = _dst(dst)
        dh, dw = dst.shape[:2]
        sh, sw = src.shape[:2]
        _check(lib().ipx_draw_rgba8(self.handle, dst.ctypes.data, dw, dh, dstride, _rect(r),
                                    src.ctypes.data, sw, sh, sstride, int(sp[0]), int(sp[1]), op))
        return dst

    # ---- the deep source types: Go's Pix rows (H x W*bpp uint8) of *image.NRGBA64 / RGBA64 / Gray16 / CMYK frames ----------
    def scale_bilinear_deep(self, pix, kind, dw, dh, sr=None, dr=None, op=OP_OVER, dst=None):
        pix, pstride = _rows(pix)
        sh, row = pix.shape
        sw = row // {DEEP_GRAY16: 2, DEEP_CMYK: 4}.get(kind, 8)
        if dst is None:
            dst = np.zeros((dh, dw, 4), np.uint8)
        dstride = _dst(dst, (dh, dw, 4))
        _check(lib().ipx_scale_bilinear_deep(self.handle, dst.ctypes.data, dw, dh, dstride, _rect(dr if dr is not None else (0, 0, dw, dh)),
                                             pix.ctypes.data, sw, sh, pstride, kind, _rect(sr if sr is not None else (0, 0, sw, sh)), op))
        return dst

    def draw_deep(self, dst, r, pix, kind, sp=(0, 0), op=OP_SRC):
        pix, pstride = _rows(pix)
        dstride = _dst(dst)
        dh, dw = dst.shape[:2]
        sh, row = pix.shape
        sw = row // {DEEP_GRAY16: 2, DEEP_CMYK: 4}.get(kind, 8)
        _check(lib().ipx_draw_deep(self.handle, dst.ctypes.data, dw, dh, dstride, _rect(r), pix.ctypes.data, sw, sh, pstride, kind,
                                   int(sp[0]), int(sp[1]), op))
        return dst

    # ---- source-type variants: *image.NRGBA and *image.YCbCr sources -------------
    def scale_bilinear_nrgba(self, src, dw, dh, sr=None, dr=None, op=OP_OVER, dst=None):
        src, sstride = _frame(src)
        sh, sw = src.shape[:2]
        if dst is None:
            dst = np.zeros((dh, dw, 4), np.uint8)
        dstride = _dst(dst, (dh, dw, 4))
        _check(lib().ipx_scale_bilinear_nrgba8(
            self.handle, dst.ctypes.data, dw, dh, dstride, _rect(dr if dr is not None else (0, 0, dw, dh)),
            src.ctypes.data, sw, sh, sstride, _rect(sr if sr is not None else (0, 0, sw, sh)), op))
        return dst

    def draw_nrgba(self, dst, r, src, sp=(0, 0), op=OP_SRC):
        src, sstride = _frame(src)
        dstride = _dst(dst)
        dh, dw = dst.shape[:2]
        sh, sw = src.shape[:2]
        _check(lib().ipx_draw_nrgba8(self.handle, dst.ctypes.data, dw, dh, dstride, _rect(r), src.ctypes.data, sw, sh,
                                     sstride, int(sp[0]), int(sp[1]), op))
        return dst

    @staticmethod
    def _ycbcr(y, cb, cr, ratio):
        (y, ystride), (cb, cstride), (cr, rstride) = (_rows(a) for a in (y, cb, cr))
        if rstride != cstride:          # (one stride serves both chroma planes)
            cb, cr = np.ascontiguousarray(cb), np.ascontiguousarray(cr)
            cstride = cb.shape[1]
        h, w = y.shape
        return _lib.YCbCr(y.ctypes.data, cb.ctypes.data, cr.ctypes.data, ystride, cstride, w, h, int(ratio)), (y, cb, cr)

    def scale_bilinear_ycbcr(self, y, cb, cr, ratio, dw, dh, sr=None, dr=None, dst=None):
        st, keep = self._ycbcr(y, cb, cr, ratio)
        if dst is None:
            dst = np.zeros((dh, dw, 4), np.uint8)
        dstride = _dst(dst, (dh, dw, 4))
        _check(lib().ipx_scale_bilinear_ycbcr(self.handle, dst.ctypes.data, dw, dh, dstride,
                                              _rect(dr if dr is not None else (0, 0, dw, dh)), C.byref(st),
                                              _rect(sr if sr is not None else (0, 0, st.w, st.h))))
        return dst

    def draw_ycbcr(self, dst, r, y, cb, cr, ratio, sp=(0, 0)):
        st, keep = self._ycbcr(y, cb, cr, ratio)
        dstride = _dst(dst)
        dh, dw = dst.shape[:2]
        _check(lib().ipx_draw_ycbcr(self.handle, dst.ctypes.data, dw, dh, dstride, _rect(r), C.byref(st), int(sp[0]),
                                    int(sp[1])))
        return dst

    # ---- jpeg.Encode (include/ipx.h, "jpeg.Encode") -------------------------------------------------------
    def jpeg_encode(self, frame, quality=85):
        """jpeg.Encode(w, *image.RGBA, &jpeg.Options{Quality}) of one host frame -> bytes"""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w = frame.shape[:2]
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().ipx_jpeg_encode_rgba8(self.handle, frame.ctypes.data, w, h, w * 4, int(quality), C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value)
        lib().ipx_buffer_free(out)
        return data

    def jpeg_fdct_dev(self, src_ptr, w, h, n, coefs_ptr, quality=85, stride=None, frame_stride=None, stream=None):
        _check(lib().ipx_dev_jpeg_fdct_rgba8(self.handle, stream, src_ptr, w, h, stride or w * 4,
                                             frame_stride if frame_stride is not None else w * h * 4, n, int(quality), coefs_ptr))

    def _stream_block(self, blob, offs, lens, n, copy):
        """what an *_encode_*_dev entry hands back (n streams in one pinned block) -> n byte strings, the block freed; copy=False:
        (memoryviews into the block, release()) instead"""
        if n == 0:
            return ([], (lambda: None)) if not copy else []
        if not copy:
            total = offs[n - 1] + lens[n - 1]
            buf = (C.c_uint8 * total).from_address(blob.value)
            mv = memoryview(buf)
            return [mv[offs[i]:offs[i] + lens[i]] for i in range(n)], (lambda: lib().ipx_host_free(self.handle, blob))
        res = [C.string_at(blob.value + offs[i], lens[i]) for i in range(n)]
        lib().ipx_host_free(self.handle, blob)
        return res

    def jpeg_encode_batch_dev(self, src_ptr, w, h, n, quality=85, stride=None, frame_stride=None, copy=True):
        """n frames in HBM -> n streams.  copy=False returns (memoryviews into the pinned block, release()) instead of bytes."""
        blob, offs, lens = C.c_void_p(), (C.c_size_t * n)(), (C.c_size_t * n)()
        _check(lib().ipx_jpeg_encode_batch_dev(self.handle, src_ptr, w, h, stride or w * 4,
                                               frame_stride if frame_stride is not None else w * h * 4, n, int(quality),
                                               C.byref(blob), offs, lens))
        return self._stream_block(blob, offs, lens, n, copy)

    def gif_encode(self, frame):
        """gif.Encode(w, *image.RGBA, nil) of one host frame (H x W x 4 uint8, premultiplied) -> bytes"""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w = frame.shape[:2]
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().ipx_gif_encode_rgba8(self.handle, frame.ctypes.data, w, h, w * 4, C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value)
        lib().ipx_buffer_free(out)
        return data

    def gif_dither_dev(self, src_ptr, w, h, n, index_ptr, stride=None, frame_stride=None, stream=None):
        """Plan 9 + Floyd-Steinberg of n frames in HBM -> n dense w x h index frames at index_ptr (HBM).  Asynchronous."""
        _check(lib().ipx_dev_gif_dither_rgba8(self.handle, stream, src_ptr, w, h, stride or w * 4,
                                              frame_stride if frame_stride is not None else w * h * 4, n, index_ptr))

    def gif_encode_batch_dev(self, src_ptr, w, h, n, stride=None, frame_stride=None, copy=True):
        """n frames in HBM -> n GIF streams.  copy=False returns (memoryviews into the pinned block, release()) instead of bytes."""
        blob, offs, lens = C.c_void_p(), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
        _check(lib().ipx_gif_encode_batch_dev(self.handle, src_ptr, w, h, stride or w * 4,
                                              frame_stride if frame_stride is not None else w * h * 4, n, C.byref(blob), offs, lens))
        return self._stream_block(blob, offs, lens, n, copy)

    def png_encode(self, frame):
        """png.Encode(w, *image.RGBA) of one host frame (H x W x 4 uint8, premultiplied) -> bytes (the zlib stream is this project's own)"""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        h, w = frame.shape[:2]
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().ipx_png_encode_rgba8(self.handle, frame.ctypes.data, w, h, w * 4, C.byref(out), C.byref(n)))
        data = C.string_at(out, n.value)
        lib().ipx_buffer_free(out)
        return data

    def png_encode_batch_dev(self, src_ptr, w, h, n, stride=None, frame_stride=None, copy=True):
        """n frames in HBM -> n PNG streams.  copy=False returns (memoryviews into the pinned block, release()) instead of bytes."""
        blob, offs, lens = C.c_void_p(), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
        _check(lib().ipx_png_encode_batch_dev(self.handle, src_ptr, w, h, stride or w * 4,
                                              frame_stride if frame_stride is not None else w * h * 4, n, C.byref(blob), offs, lens))
        return self._stream_block(blob, offs, lens, n, copy)

    def _decode_batch(self, entry, free, files, dims, batch, download):
        """What the *_decode_batch methods share: the call of `entry` (dims: the size, and the kind, asked for; batch: the entry's
        batch struct, filled here) -> (dims as the entry set them, status list, done).  done is None when no file was decodable;
        else done(info) ends the method: the device blocks are released (download) or go into info as `batch` and `free`."""
        n = len(files)
        cdims = [C.c_int(v) for v in dims]
        status = (C.c_int * max(n, 1))()
        owner = C.c_void_p()
        _check(getattr(lib(), entry)(self.handle, None, _bytes_array(files), n, *[C.byref(d) for d in cdims], C.byref(batch), status,
                                     C.byref(owner)))
        release = lambda: getattr(lib(), free)(self.handle, owner)

        def done(info):
            if download:
                release()
            else:
                info.update(batch=batch, free=release)
            return info
        # (every batch struct starts with the pointer that is null when there are no frames)
        return [d.value for d in cdims], list(status)[:n], (done if getattr(batch, batch._fields_[0][0]) else None)

    def _grab(self, ptr, n, frame_stride):
        """n frames frame_stride bytes apart in HBM -> an n x frame_stride uint8 array"""
        out = np.empty((n, frame_stride), np.uint8)
        _check(lib().ipx_memcpy_d2h(self.handle, out.ctypes.data, ptr, out.nbytes))
        return out

    def jpeg_decode_batch(self, files, w=0, h=0, download=True):
        """image.Decode of a batch of JPEG byte strings on the GPU.  -> (info, status list); info = dict(w, h, ratio, ystride,
        cstride, y, cb, cr) with the planes as n x rows x stride arrays (download=True) or device pointers + `free()`."""
        n, b = len(files), _lib.YCbCrBatch()
        (w, h), st, done = self._decode_batch("ipx_jpeg_decode_batch", "ipx_jpeg_planes_free", files, (w, h), b, download)
        if done is None:
            return None, st
        info = {"w": w, "h": h, "ratio": b.ratio, "ystride": b.ystride, "cstride": b.cstride}
        v0 = 2 if b.ratio in (2, 3, YCBCR_410) else 1   # 4:2:0, 4:4:0 and 4:1:0 halve the chroma rows (Gray: 8 x 8 MCUs)
        myy = (h + 8 * v0 - 1) // (8 * v0)
        yrows, crows = 8 * v0 * myy, 8 * myy            # image.NewYCbCr(Rect(0, 0, 8*h0*mxx, 8*v0*myy), ratio)
        if download:
            info["y"] = self._grab(b.y, n, b.y_frame_stride)[:, :yrows * b.ystride].reshape(n, yrows, b.ystride)
            if b.cb:   # *image.Gray has no chroma planes
                info["cb"] = self._grab(b.cb, n, b.c_frame_stride)[:, :crows * b.cstride].reshape(n, crows, b.cstride)
                info["cr"] = self._grab(b.cr, n, b.c_frame_stride)[:, :crows * b.cstride].reshape(n, crows, b.cstride)
        return done(info), st

    def jpeg_decode_mixed(self, files, download=True):
        """image.Decode of JPEG byte strings of ANY sizes and samplings, one decode pass per sampling class (ipx_jpeg_decode_mixed).
        A file given as None goes in as a NULL entry.  -> (frames, status list); frames[i] is None for a non-OK file, else dict(w, h,
        ratio, ystride, cstride, y, cb, cr) with the
        planes over the image's MCU-padded extent as rows x stride uint8 arrays, cb and cr None for a Gray file (download=True), or the
        device pointers.  With download=False a third value, free(), releases the planes."""
        def frame(f):
            if not f.y:
                return None
            d = {"w": f.w, "h": f.h, "ratio": f.ratio, "ystride": f.ystride, "cstride": f.cstride, "y": f.y, "cb": f.cb, "cr": f.cr}
            if download:
                v0 = 2 if f.ratio in (2, 3) else 1          # 4:2:0 and 4:4:0 halve the chroma rows (Gray: 8 x 8 MCUs)
                myy = (f.h + 8 * v0 - 1) // (8 * v0)
                d["y"] = self._grab(f.y, 8 * v0 * myy, f.ystride)
                d["cb"] = self._grab(f.cb, 8 * myy, f.cstride) if f.cb else None
                d["cr"] = self._grab(f.cr, 8 * myy, f.cstride) if f.cr else None
            return d
        return self._decode_mixed("ipx_jpeg_decode_mixed", "ipx_jpeg_planes_free", files, _lib.JpegFrame, frame, download)

    def _decode_mixed(self, entry, free, files, frame_type, frame, download):
        """What the *_decode_mixed methods share: the arrays (a file given as None goes in as a NULL entry: IPX_ERR_INVALID for that file
        alone), the call of `entry`, then frame(record) for every file -- the dict of a decoded frame, downloading what it downloads,
        or None -- and the release of the device blocks: here (download), or left to the caller as a third value."""
        n = len(files)
        arr = _bytes_array([f if f is not None else b"" for f in files])
        for i, f in enumerate(files):
            if f is None:
                arr[i].data = None
        fr = (frame_type * max(n, 1))()
        status = (C.c_int * max(n, 1))()
        owner = C.c_void_p()
        _check(getattr(lib(), entry)(self.handle, None, arr, n, fr, status, C.byref(owner)))
        release = lambda: getattr(lib(), free)(self.handle, owner)
        try:
            out = [frame(fr[i]) for i in range(n)]
        finally:
            if download:
                release()
        return (out, list(status)[:n]) if download else (out, list(status)[:n], release)

    JPEG_ROUTE_PAR, JPEG_ROUTE_HOST_SCANS, JPEG_ROUTE_GPU_SCANS = 0, 1, 2

    @staticmethod
    def jpeg_scan_route(data):
        """Which decoder the scans of this JPEG would reach now (IPX_JPEG_PROG_GPU is read): -> (parse status, JPEG_ROUTE_*).  Host
        only: needs no device."""
        buf = bytes(data)
        route = C.c_int(-1)
        st = lib().ipx_jpeg_scan_route(buf, len(buf), C.byref(route))
        return st, route.value

    def jpeg_decode_counts(self):
        """Since the context was made: files that reached the decoder of route [0..2], and [3] files the GPU scan walk ended with a
        status other than IPX_OK."""
        counts = (C.c_longlong * 4)()
        _check(lib().ipx_jpeg_decode_counts(self.handle, counts))
        return list(counts)

    def png_decode_counts(self):
        """Since the context was made, under IPX_PNG_PAR=1: [0] files that entered the parallel inflate, [1] files it finished, [2] files
        its redo bit handed to the serial decoder, [3] tokens decoded by the parallel lanes, [4] tokens decoded by the wave-uniform
        loop inside that kernel ([3], [4]: files of [1] only).  All 0 while the switch is unset."""
        counts = (C.c_longlong * 5)()
        _check(lib().ipx_png_decode_counts(self.handle, counts))
        return list(counts)

    def gif_decode_counts(self):
        """Since the context was made, under IPX_GIF_PAR=1: [0] files that entered the parallel code walk, [1] files it finished, [2]
        files its redo bit handed to the serial walk, [3] code records written by the parallel lanes (files of [1] only).  All 0
        while the switch is unset."""
        counts = (C.c_longlong * 4)()
        _check(lib().ipx_gif_decode_counts(self.handle, counts))
        return list(counts)

    def jpeg_decode_batch_cmyk(self, files, w=0, h=0, download=True):
        """image.Decode of a batch of four-component JPEG byte strings (Adobe CMYK / YCCK) on the GPU, under IPX_JPEG_CMYK=1.
        -> (info, status list); info = dict(w, h, stride, pix) with pix as an n x h x w x 4 uint8 array of *image.CMYK pixels
        (download=True), or the device batch (CmykBatch) + `free()`; None when no file was decodable."""
        n, b = len(files), _lib.CmykBatch()
        (w, h), st, done = self._decode_batch("ipx_jpeg_decode_batch_cmyk", "ipx_jpeg_planes_free", files, (w, h), b, download)
        if done is None:
            return None, st
        info = {"w": w, "h": h, "stride": b.stride}
        if download:
            info["pix"] = self._grab(b.pix, n, b.frame_stride)[:, :h * b.stride].reshape(n, h, w, 4)
        return done(info), st

    def jpeg_cmyk_files(self):
        """Since the context was made: files that reached the four-component JPEG decoder."""
        files = C.c_longlong(0)
        _check(lib().ipx_jpeg_cmyk_files(self.handle, C.byref(files)))
        return files.value

    def gif_decode_batch(self, files, w=0, h=0, download=True):
        """image.Decode of a batch of GIF byte strings on the GPU (the first image of each).  -> (info, status list); info = dict(w, h,
        stride, index, palettes) with index as n x h x w and palettes as n x 256 x 4 uint8 arrays (download=True), or the device
        batch (PalettedBatch) + `free()`; None when no file was decodable."""
        n, b = len(files), _lib.PalettedBatch()
        (w, h), st, done = self._decode_batch("ipx_gif_decode_batch", "ipx_gif_frames_free", files, (w, h), b, download)
        if done is None:
            return None, st
        info = {"w": w, "h": h, "stride": b.stride}
        if download:
            info["index"] = self._grab(b.index, n, b.frame_stride)[:, :w * h].reshape(n, h, w)
            info["palettes"] = self._grab(b.palettes, n, 1024).reshape(n, 256, 4)
        return done(info), st

    PNG_BPP = (1, 4, 4, 1, 2, 8, 8)     # bytes per pixel of the PNG_* frame layouts

    def png_decode_batch(self, files, w=0, h=0, kind=-1, download=True):
        """image.Decode of a batch of PNG byte strings on the GPU.  -> (info, status list); info = dict(w, h, kind, stride, pix, palettes)
        with pix as n x h x (w * bytes per pixel) uint8 (Go's Pix rows) and palettes as n x 256 x 4 uint8 (PNG_PALETTED) or None
        (download=True), or the device batch (PngBatch) + `free()`; None when no file was decodable."""
        n, b = len(files), _lib.PngBatch()
        (w, h, kind), st, done = self._decode_batch("ipx_png_decode_batch", "ipx_png_frames_free", files, (w, h, kind), b, download)
        if done is None:
            return None, st
        info = {"w": w, "h": h, "kind": kind, "stride": b.stride}
        if download:
            info["pix"] = self._grab(b.pix, n, b.frame_stride)[:, :b.stride * h].reshape(n, h, b.stride)
            info["palettes"] = self._grab(b.palettes, n, 1024).reshape(n, 256, 4) if b.palettes else None
        return done(info), st

    def png_decode_mixed(self, files, download=True):
        """image.Decode of PNG byte strings of ANY sizes and kinds in one decode pass (ipx_png_decode_mixed).  -> (frames, status
        list); frames[i] is None for a non-OK file, else dict(w, h, kind, stride, pix, palette) with pix as h x (w * bytes per pixel)
        uint8 (Go's Pix rows) and palette as 256 x 4 uint8 (PNG_PALETTED) or None (download=True), or the device pointers.  With
        download=False a third value, free(), releases the frames."""
        def frame(f):
            if not f.pix:
                return None
            d = {"w": f.w, "h": f.h, "kind": f.kind, "stride": f.stride, "pix": f.pix, "palette": f.palette}
            if download:
                d["pix"] = self._grab(f.pix, f.h, f.stride)
                d["palette"] = self._grab(f.palette, 256, 4) if f.palette else None
            return d
        return self._decode_mixed("ipx_png_decode_mixed", "ipx_png_frames_free", files, _lib.PngFrame, frame, download)

    def png_encode_mixed_dev(self, frames, copy=True):
        """frames: (device pointer, w, h, stride) per RGBA8 frame in HBM, of any sizes -> one PNG stream each (ipx_png_encode_mixed_dev).
        copy=False returns (memoryviews into the pinned block, release()) instead of bytes."""
        frames = list(frames)
        n = len(frames)
        arr = (_lib.RgbaFrame * max(n, 1))()
        for i, (ptr, w, h, stride) in enumerate(frames):
            arr[i] = _lib.RgbaFrame(ptr, int(w), int(h), int(stride))
        blob, offs, lens = C.c_void_p(), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
        _check(lib().ipx_png_encode_mixed_dev(self.handle, arr, n, C.byref(blob), offs, lens))
        return self._stream_block(blob, offs, lens, n, copy)

    def jpeg_encode_mixed_dev(self, frames, quality=85, copy=True):
        """frames: (device pointer, w, h, stride) per RGBA8 frame in HBM, of any sizes -> one JPEG stream each, byte for byte
        jpeg_encode_batch_dev's for that frame alone (ipx_jpeg_encode_mixed_dev).  copy=False returns (memoryviews into the pinned
        block, release()) instead of bytes."""
        frames = list(frames)
        n = len(frames)
        arr = (_lib.RgbaFrame * max(n, 1))()
        for i, (ptr, w, h, stride) in enumerate(frames):
            arr[i] = _lib.RgbaFrame(ptr, int(w), int(h), int(stride))
        blob, offs, lens = C.c_void_p(), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
        _check(lib().ipx_jpeg_encode_mixed_dev(self.handle, arr, n, int(quality), C.byref(blob), offs, lens))
        return self._stream_block(blob, offs, lens, n, copy)

    def gif_decode_mixed(self, files, download=True):
        """image.Decode of GIF byte strings of ANY sizes in one decode pass (ipx_gif_decode_mixed; the first image of each).  A file
        given as None goes in as a NULL entry.  -> (frames, status list); frames[i] is None for a non-OK file, else dict(w, h, stride,
        index, palette) with index as h x w and palette as 256 x 4 uint8 (download=True), or the device pointers.  With download=False
        a third value, free(), releases the frames."""
        def frame(f):
            if not f.index:
                return None
            d = {"w": f.w, "h": f.h, "stride": f.stride, "index": f.index, "palette": f.palette}
            if download:
                d["index"] = self._grab(f.index, f.h, f.stride)
                d["palette"] = self._grab(f.palette, 256, 4)
            return d
        return self._decode_mixed("ipx_gif_decode_mixed", "ipx_gif_frames_free", files, _lib.GifFrame, frame, download)

    def gif_encode_mixed_dev(self, frames, copy=True):
        """frames: (device pointer, w, h, stride) per RGBA8 frame in HBM, of any sizes -> one GIF stream each, byte for byte
        gif_encode_batch_dev's for that frame alone (ipx_gif_encode_mixed_dev).  copy=False returns (memoryviews into the pinned
        block, release()) instead of bytes."""
        frames = list(frames)
        n = len(frames)
        arr = (_lib.RgbaFrame * max(n, 1))()
        for i, (ptr, w, h, stride) in enumerate(frames):
            arr[i] = _lib.RgbaFrame(ptr, int(w), int(h), int(stride))
        blob, offs, lens = C.c_void_p(), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
        _check(lib().ipx_gif_encode_mixed_dev(self.handle, arr, n, C.byref(blob), offs, lens))
        return self._stream_block(blob, offs, lens, n, copy)

    def run_gif_gif_mixed(self, ops, files, quality=85, want=("resize", "thumbnail", "watermark"), copy=True, texts=None):
        """GIF byte strings of ANY sizes in -> ({operator: [bytes | None] * n}, status list): one decode pass per group, the operators
        per run of one size, one mixed-size gif.Encode of the resize and thumbnail outputs and one jpeg.Encode of the watermark
        outputs per chunk (ipx_run_gif_gif_mixed).  ops, texts and copy as for run_jpeg_jpeg_mixed."""
        ops, keep = _pool_ops(ops, glyph_list=True)
        return self._run_mixed(lib().ipx_run_gif_gif_mixed, ops, files, texts, want, copy, (int(quality),))

    def run_png_png_mixed(self, ops, files, want=("resize", "thumbnail", "watermark"), copy=True, texts=None):
        """PNG byte strings of ANY sizes and kinds in -> ({operator: [png bytes | None] * n}, status list): one decode pass per group,
        the operators per run of one size, one mixed-size png.Encode per output (ipx_run_png_png_mixed).  ops: a PoolOps with sw = sh
        = 0 and no glyphs, or dict(resize=(w, h, keep_aspect) | None, thumbnail=(size, crop_to_fit) | None, watermark=bool).
        texts: None, or one (glyphs, col) per file, positioned for that file's size.  copy=False: lengths instead of bytes."""
        ops, keep = _pool_ops(ops)
        return self._run_mixed(lib().ipx_run_png_png_mixed, ops, files, texts, want, copy)

    def run_jpeg_jpeg_mixed(self, ops, files, quality=85, want=("resize", "thumbnail", "watermark"), copy=True, texts=None):
        """JPEG byte strings of ANY sizes and samplings in -> ({operator: [jpeg bytes | None] * n}, status list): one decode pass per
        group and sampling class, the operators per run of one size, one jpeg.Encode per chunk (ipx_run_jpeg_jpeg_mixed).  ops:
        a PoolOps, or dict(resize=(w, h, keep_aspect) | None, thumbnail=(size, crop_to_fit) | None, watermark=bool | (glyphs, col): a
        glyph list every size's plan clips against its own frame).  texts: None, or one (glyphs, col) per file, positioned for that
        file's size (then no glyph list in ops).  copy=False: lengths instead of bytes."""
        ops, keep = _pool_ops(ops, glyph_list=True)
        return self._run_mixed(lib().ipx_run_jpeg_jpeg_mixed, ops, files, texts, want, copy, (int(quality),))

    def _run_mixed(self, entry, ops, files, texts, want, copy, args=()):
        """A mixed-size leg: the texts, an output array per wanted operator, the call (args go between the texts and the arrays), then
        ({operator: [bytes | length | None] * n}, status list); the result is freed."""
        n = len(files)
        tarr, keep = _texts_for(texts, n)
        arrs = {k: (_lib.Bytes * max(n, 1))() for k in ("resize", "thumbnail", "watermark") if k in want}
        status = (C.c_int * max(n, 1))()
        res = C.c_void_p()
        _check(entry(self.handle, C.byref(ops), n, _bytes_array(files), tarr, *args, arrs.get("resize"), arrs.get("thumbnail"),
                     arrs.get("watermark"), status, C.byref(res)))
        out = _streams(arrs, n, copy)
        lib().ipx_jpeg_result_free(self.handle, res)
        return out, list(status)[:n]

    def composite_glyphs(self, dst, glyphs, col):
        dstride = _dst(dst)
        dh, dw = dst.shape[:2]
        arr, keep = _glyph_array(list(glyphs))
        c = (C.c_uint8 * 4)(*[int(v) for v in col])
        _check(lib().ipx_composite_glyphs_rgba8(self.handle, dst.ctypes.data, dw, dh, dstride, arr,
                                                len(glyphs), c))
        return dst


class PoolJob:
    """One submitted job of a Pool: keeps the arrays the library writes into alive until wait()."""

    def __init__(self, pool, job, keep, outs, n):
        self.pool, self.job, self.keep, self.outs, self.n = pool, job, keep, outs, n
        t = C.c_uint64()
        _check(lib().ipx_job_submit(pool.handle, C.byref(job), C.byref(t)))
        self.ticket = t.value
        self.released = False

    def done(self):
        d = C.c_int()
        _check(lib().ipx_job_poll(self.pool.handle, self.ticket, C.byref(d)))
        return bool(d.value)

    def wait(self):
        """-> dict of outputs (arrays for a pixel job; ({operator: [bytes | None]}, status list) for a file job: JPEG, PNG or GIF);
        releases the job"""
        fd = C.c_int()
        try:
            _check(lib().ipx_job_wait(self.pool.handle, self.ticket, C.byref(fd)))
            if self.job.kind not in Pool.FILE_KINDS.values():      # every kind but the file jobs hands pixels back
                return self.outs
            return _streams(self.outs, self.n, True), list(self.keep["status"])[:self.n]
        finally:
            self.release()

    def release(self):
        if not self.released:
            self.released = True
            lib().ipx_job_release(self.pool.handle, self.ticket)


class Pool:
    """One process, several GPUs (ipx_pool_*): a context per listed device, feeder threads, one largest-first queue."""

    def __init__(self, devices=(0,), lanes_per_device=0, lane_bytes=0):
        arr = (C.c_int * len(devices))(*devices)
        cfg = _lib.PoolConfig(lanes_per_device, lane_bytes)
        h = C.c_void_p()
        _check(lib().ipx_pool_create(arr, len(devices), C.byref(cfg), C.byref(h)))
        self.handle = h.value

    def close(self):
        if self.handle:
            lib().ipx_pool_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def slots(self):
        return lib().ipx_pool_slots(self.handle)

    def frames_done(self, slot):
        return lib().ipx_pool_frames_done(self.handle, slot)

    def png_decode_counts(self):
        """Context.png_decode_counts summed over the pool's slots (IPX_JOB_PNG and the micro-batcher decode on the slots' contexts)"""
        total = [0] * 5
        for slot in range(self.slots()):
            counts = (C.c_longlong * 5)()
            _check(lib().ipx_pool_png_decode_counts(self.handle, slot, counts))
            total = [a + b for a, b in zip(total, counts)]
        return total

    def gif_decode_counts(self):
        """Context.gif_decode_counts summed over the pool's slots (IPX_JOB_GIF and the micro-batcher decode on the slots' contexts)"""
        total = [0] * 4
        for slot in range(self.slots()):
            counts = (C.c_longlong * 4)()
            _check(lib().ipx_pool_gif_decode_counts(self.handle, slot, counts))
            total = [a + b for a, b in zip(total, counts)]
        return total

    def host_alloc(self, slot, shape, dtype=np.uint8):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = lib().ipx_pool_host_alloc(self.handle, slot, max(1, n))
        if not p:
            raise IpxError(-2, lib().ipx_last_error().decode())
        arr = np.frombuffer((C.c_uint8 * n).from_address(p), dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = (slot, p)
        return arr

    def host_free(self, arr):
        slot, p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, (None, None))
        if p:
            lib().ipx_pool_host_free(self.handle, slot, p)

    @staticmethod
    def _ops(sw, sh, resize, thumbnail, glyphs, col, watermark):
        o = _lib.PoolOps()
        o.sw, o.sh = sw, sh
        if resize:
            o.do_resize, o.resize_w, o.resize_h, o.keep_aspect = 1, resize[0], resize[1], int(bool(resize[2]))
        if thumbnail:
            o.do_thumbnail, o.thumb_size, o.crop_to_fit = 1, thumbnail[0], int(bool(thumbnail[1]))
        keep = None
        if watermark or glyphs:
            o.do_watermark = 1
            if glyphs:
                arr, keep = _glyph_array(list(glyphs))
                o.glyphs, o.n_glyphs = arr, len(glyphs)
                keep = (arr, keep)
                for i in range(4):
                    o.col[i] = int(col[i])
        return o, keep

    JOB_KINDS = {"rgba": (0, 4), "nrgba": (2, 4), "gray": (3, 1), "nrgba64": (4, 8), "rgba64": (5, 8), "gray16": (6, 2), "cmyk": (7, 4)}   # IPX_JOB_*: (kind, bytes per pixel)

    def submit(self, frames, resize=(1024, 768, True), thumbnail=(200, True), glyphs=None, col=(0, 0, 0, 0), watermark=False, out=None,
               kind="rgba"):
        """frames: n x H x W x 4 uint8 (host); for another `kind` (JOB_KINDS) n x H x (W * bpp) uint8, the type's Pix rows.
        -> PoolJob; wait() gives {"resize", "thumbnail", "watermark"} arrays."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        jk, bpp = self.JOB_KINDS[kind]
        if kind != "rgba":
            frames = frames.reshape(frames.shape[0], frames.shape[1], -1)
        n, sh = frames.shape[:2]
        sw = frames.shape[2] if kind == "rgba" else frames.shape[2] // bpp
        ops, keep = self._ops(sw, sh, resize, thumbnail, glyphs, col, watermark)
        outs = dict(out) if out else {}
        if resize and "resize" not in outs:
            outs["resize"] = np.empty((n,) + tuple(reversed(resize_dims(sw, sh, resize[0], resize[1], resize[2]))) + (4,), np.uint8)
        if thumbnail and "thumbnail" not in outs:
            _, tw, th = thumb_geometry(sw, sh, thumbnail[0] or 200, thumbnail[1])
            outs["thumbnail"] = np.empty((n, th, tw, 4), np.uint8)
        if ops.do_watermark and "watermark" not in outs:
            outs["watermark"] = np.empty((n, sh, sw, 4), np.uint8)
        j = _lib.Job()
        j.kind, j.ops, j.n = jk, ops, n
        j.src, j.sstride, j.src_frame_stride = frames.ctypes.data, sw * bpp, sw * sh * bpp

        def fs(a):
            return int(np.prod(a.shape[1:]))
        if "resize" in outs:
            j.resize_out, j.resize_frame_stride = outs["resize"].ctypes.data, fs(outs["resize"])
        if "thumbnail" in outs:
            j.thumb_out, j.thumb_frame_stride = outs["thumbnail"].ctypes.data, fs(outs["thumbnail"])
        if "watermark" in outs:
            j.wm_out, j.wm_frame_stride = outs["watermark"].ctypes.data, fs(outs["watermark"])
        return PoolJob(self, j, {"frames": frames, "glyphs": keep}, outs, n)

    FILE_KINDS = {"jpeg": 1, "png": 8, "gif": 9}      # IPX_JOB_JPEG / _PNG / _GIF

    def submit_jpeg(self, files, sw, sh, quality=85, resize=(1024, 768, True), thumbnail=(200, True), glyphs=None, col=(0, 0, 0, 0),
                    watermark=False):
        """JPEG byte strings of sw x sh images in -> PoolJob; wait() gives ({operator: [bytes | None]}, status list)."""
        return self.submit_files(files, sw, sh, "jpeg", quality, resize, thumbnail, glyphs, col, watermark)

    def submit_files(self, files, sw, sh, format="jpeg", quality=85, resize=(1024, 768, True), thumbnail=(200, True), glyphs=None,
                     col=(0, 0, 0, 0), watermark=False, want=("resize", "thumbnail", "watermark"), texts=None):
        """Uploaded files of one format ("jpeg", "png", "gif") and of sw x sh images in -> PoolJob; wait() gives ({operator: [bytes |
        None]}, status list) with streams of the job's format (PNG: three PNGs; GIF: GIF, GIF and a JPEG at `quality` for the
        watermark).  An operator not in `want` gets no output array and is left out.  texts: None, or one (glyphs, col) per file
        (ipx_job.texts; `glyphs` must then be left out)."""
        n = len(files)
        ops, keep = self._ops(sw, sh, resize, thumbnail, glyphs, col, watermark or texts is not None)
        tarr = None
        if texts is not None:
            texts = list(texts)
            if len(texts) != n:
                raise ValueError("one text per file")
            tarr = _text_array(texts)
        arr = _bytes_array(files)
        status = (C.c_int32 * max(1, n))()
        outs = {}
        j = _lib.Job()
        j.kind, j.ops, j.n, j.files, j.quality, j.status = self.FILE_KINDS[format], ops, n, arr, int(quality), status
        if tarr is not None:
            j.texts = tarr[0]
        if resize and "resize" in want:
            outs["resize"] = (_lib.Bytes * max(1, n))()
            j.resize_jpeg = outs["resize"]
        if thumbnail and "thumbnail" in want:
            outs["thumbnail"] = (_lib.Bytes * max(1, n))()
            j.thumb_jpeg = outs["thumbnail"]
        if ops.do_watermark and "watermark" in want:
            outs["watermark"] = (_lib.Bytes * max(1, n))()
            j.wm_jpeg = outs["watermark"]
        return PoolJob(self, j, {"files": arr, "status": status, "glyphs": keep, "texts": tarr}, outs, n)


def jpeg_entropy_encode(coefs, w, h, quality=85):
    """Host half of jpeg.Encode: quantised coefficients (int16, 6 x 64 per MCU, zig-zag) -> the byte stream."""
    coefs = np.ascontiguousarray(coefs, dtype=np.int16)
    assert coefs.size == lib().ipx_jpeg_coef_count(w, h)
    out, n = C.c_void_p(), C.c_size_t()
    _check(lib().ipx_jpeg_entropy_encode(coefs.ctypes.data, w, h, int(quality), C.byref(out), C.byref(n)))
    data = C.string_at(out, n.value)
    lib().ipx_buffer_free(out)
    return data


def jpeg_quant_tables(quality):
    out = (C.c_uint8 * 128)()
    _check(lib().ipx_jpeg_quant_tables(int(quality), out))
    return np.frombuffer(out, np.uint8).reshape(2, 64).copy()


class Batcher:
    """Micro-batching of single uploads (ipx_batcher_*): what the goroutines of internal/worker/worker.go:112-149 would call, one file each.

    submit(file bytes -- JPEG, PNG or GIF, told apart by the library --, frame size, operators) -> ticket; wait(ticket) -> (status, {operator: bytes | None}); the ticket is released by wait."""

    def __init__(self, pool, max_batch=0, max_wait_us=0, quality=0):
        self.pool = pool
        cfg = _lib.BatcherConfig(max_batch, max_wait_us, quality)
        h = C.c_void_p()
        _check(lib().ipx_batcher_create(pool.handle, C.byref(cfg), C.byref(h)))
        self.handle = h.value
        self._keep = {}
        self._mu = __import__("threading").Lock()

    def close(self):
        if self.handle:
            lib().ipx_batcher_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def submit(self, data, sw, sh, resize=None, thumbnail=None, glyphs=None, col=(255, 255, 255, 127), watermark=False):
        ops_, keep = Pool._ops(sw, sh, resize, thumbnail, glyphs, col, watermark)
        buf = C.create_string_buffer(bytes(data), len(data))
        fb = _lib.Bytes(C.cast(buf, C.c_void_p), len(data))
        t = C.c_uint64()
        _check(lib().ipx_batcher_submit(self.handle, C.byref(fb), C.byref(ops_), C.byref(t)))
        with self._mu:
            self._keep[t.value] = buf          # the file's bytes stay where they are until the ticket is released
        return t.value

    def wait(self, ticket):
        res = _lib.BatchResult()
        try:
            _check(lib().ipx_batcher_wait(self.handle, ticket, C.byref(res)))
            out = {k: (C.string_at(getattr(res, f).data, getattr(res, f).len) if getattr(res, f).data else None)
                   for k, f in (("resize", "resize"), ("thumbnail", "thumb"), ("watermark", "wm"))}
            return res.status, out
        finally:
            lib().ipx_batcher_release(self.handle, ticket)
            with self._mu:
                self._keep.pop(ticket, None)

    def stats(self):
        st = _lib.BatcherStats()
        _check(lib().ipx_batcher_get_stats(self.handle, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}
