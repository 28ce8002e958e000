"""Frame layouts for the entries that take frames in HBM (tests/test_layouts.py, tests/test_layouts_gpu.py): the same pixels at other
pointer alignments, row strides and frame strides, as data plus one helper per direction.

A source batch is laid out by lay_out(): the frames at `offset` into a 256-byte aligned allocation, rows `extra_stride` bytes wider than
the pixels, frames `extra_frame` bytes further apart than their rows, every byte that is no pixel 0xA5.  An output batch gets the mirror:
out_alloc() gives an allocation of 0xA5 with a guard region before the first frame and behind the last, out_frames() takes the frames
out of it after the call and asserts that every other byte is still 0xA5."""
import numpy as np

# (numpy only: the codec corpora take lay_out() from here; the expected outputs of these cases are in tests/layout_expected.py)
FILL = 0xA5
GUARD = 256        # bytes of guard on either side of an output batch (a multiple of the allocation's alignment: `offset` is the misalignment)


def lay_out(frames, extra_stride, extra_frame, offset):
    """n x H x (anything: W x 4 pixels, W bytes of a plane, W * bpp bytes of Pix) -> (bytes of the allocation, offset of frame 0, row
    stride, frame stride); the padding is filled with 0xA5 so that a kernel reading it would show"""
    frames = np.asarray(frames, dtype=np.uint8)
    n, h = frames.shape[:2]
    rows = frames.reshape(n, h, -1)
    row = rows.shape[2]
    stride = row + extra_stride
    fs = h * stride + extra_frame
    buf = np.full(offset + n * fs + 64, FILL, np.uint8)
    for i in range(n):
        view = np.lib.stride_tricks.as_strided(buf[offset + i * fs:], (h, row), (stride, 1))
        view[...] = rows[i]
    return buf, offset, stride, fs


def out_alloc(n, frame_bytes, offset, extra_frame):
    """-> (bytes of the allocation, all 0xA5; offset of frame 0; frame stride) for n output frames of frame_bytes each"""
    fs = frame_bytes + extra_frame
    first = GUARD + offset
    return np.full(first + (n - 1) * fs + frame_bytes + GUARD, FILL, np.uint8), first, fs


def out_frames(buf, n, frame_bytes, first, fs, shape=None, what=""):
    """The n frames of an output allocation after the call (a copy, n x shape), having asserted that every byte outside them -- the
    guards and the gaps between the frames -- is still 0xA5."""
    buf = np.asarray(buf, dtype=np.uint8)
    assert buf.size == first + (n - 1) * fs + frame_bytes + GUARD, "%s: not the allocation of out_alloc" % what
    outside = np.ones(buf.size, bool)
    frames = np.empty((n, frame_bytes), np.uint8)
    for i in range(n):
        outside[first + i * fs: first + i * fs + frame_bytes] = False
        frames[i] = buf[first + i * fs: first + i * fs + frame_bytes]
    touched = np.flatnonzero(outside & (buf != FILL))
    assert touched.size == 0, "%s: %d bytes outside the frames were written, first at %d (frame 0 at %d, %d bytes, frame stride %d)" % (
        what, touched.size, int(touched[0]), first, frame_bytes, fs)
    return frames.reshape((n,) + tuple(shape)) if shape is not None else frames


# ---- the layouts ----------------------------------------------------------------------------------------------------------------------
# sources: (offset, extra row stride, extra frame stride) in bytes
TIGHT = (0, 0, 0)
DWORD_LAYOUTS = [(4, 0, 0), (8, 0, 0), (12, 0, 0), (0, 4, 0), (0, 12, 0), (0, 16, 24), (12, 16, 20)]   # dword-aligned; none keeps 16 bytes
MOST_PADDED = (12, 16, 20)
UNALIGNED_LAYOUTS = [(1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 2)]                           # not dword-aligned
SRC_LAYOUTS = [TIGHT] + DWORD_LAYOUTS + UNALIGNED_LAYOUTS
# chroma planes, next to a tight Y plane: 2 leaves the gate of 4:4:4 / 4:4:0 (dword loads) and stays inside that of 4:2:0 / 4:2:2 (word
# loads); 1 leaves both, and none leaves that of 4:1:1 / 4:1:0 (byte loads)
CHROMA_LAYOUTS = [(2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
# outputs: (offset, extra frame stride)
OUT_TIGHT = (0, 0)
OUT_PADDED = (4, 20)
OUT_LAYOUTS = [OUT_TIGHT, (16, 32), (4, 4), OUT_PADDED, (0, 12)]
OUT_REFUSED = [(1, 0), (0, 1), (2, 3)]              # not dword-aligned: IPX_ERR_INVALID before any launch (include/ipx.h)

N = 3
# (source w, h, resize (w, h, keep aspect) | None, thumbnail (size, crop) | None, watermark): the smallest shapes at which the paths differ
SHAPES = [(104, 61, (52, 30, False), (24, True), True),
          (101, 60, (52, 30, False), (24, True), True),            # ragged rows: sw & 3
          (25, 25, (128, 128, False), None, False)]                # an upscale the per-output kernels get (more than four row accumulators)
# host batches into outputs with gaps (RGBA only): a resize output of 1500 bytes, no multiple of 16, which the lanes' scratch pads to 256
HOST_GAP_SHAPE = (104, 61, (25, 15, False), (24, True), True)
DEEP_KINDS = ("nrgba64", "rgba64", "gray16", "cmyk")
RATIO = {"ycbcr444": 0, "ycbcr422": 1, "ycbcr420": 2, "ycbcr440": 3, "ycbcr411": 5, "ycbcr410": 6}      # include/ipx.h's IPX_YCBCR_*, as scaler_cases has it
FULL_KINDS = ["rgba", "nrgba", "gray", "ycbcr420", "ycbcr444", "ycbcr411"]      # every layout; the others: three to five each (kind_layouts)
COL = (255, 255, 255, 127)


def corner_glyphs(w, h, seed=0xC0):
    """A glyph set whose boxes reach the last column and the last row: the text then writes the very end of each watermark frame"""
    rng = np.random.default_rng(seed)
    out = []
    for x0, y0, x1, y1 in ((w - 19, h - 23, w, h), (w - 40, h - 30, w - 17, h - 2), (3, h - 12, 20, h), (w - 9, 2, w, 30), (0, 0, 7, 9)):
        m = rng.integers(0, 256, (y1 - y0, x1 - x0), dtype=np.uint8)
        sel = rng.random(m.shape)
        m[sel < 0.3] = 0
        m[sel > 0.7] = 255
        out.append({"mask": m, "dr": (x0, y0, x1, y1), "mp": (0, 0)})
    return out


def kind_layouts(kind):
    """-> [(source layout, chroma layout | None)] the kind runs.  A chroma layout of None: the chroma planes take the Y plane's."""
    if kind in FULL_KINDS:
        out = [(l, None) for l in SRC_LAYOUTS]
        if kind.startswith("ycbcr"):
            out += [(TIGHT, c) for c in CHROMA_LAYOUTS]
        return out
    if kind == "ycbcr410":                         # tight, padded, chroma at an odd pointer, at odd strides (all inside its gate), Y off its gate
        return [(TIGHT, None), (MOST_PADDED, None), (TIGHT, (1, 0, 0)), (TIGHT, (0, 1, 1)), ((1, 0, 0), TIGHT)]
    if kind.startswith("ycbcr"):                   # 4:2:2, 4:4:0: tight, padded, chroma off its gate, Y off its gate
        return [(TIGHT, None), (MOST_PADDED, None), (TIGHT, (2, 0, 0)), (TIGHT, (0, 1, 0)), ((1, 0, 0), TIGHT)]
    # Paletted and the deep types are expanded into scratch of the library's own before the scaler sees them: no legal source layout leaves
    # the one-pass kernel.  The third layout is the least aligned one src_check admits (index bytes: any; 16-bit samples: 2; CMYK: 4)
    last = {"cmyk": (4, 4, 4), "nrgba64": (2, 2, 2), "rgba64": (2, 2, 2), "gray16": (2, 2, 2)}.get(kind, (1, 1, 1))
    return [(TIGHT, None), (MOST_PADDED, None), (last, None)]


def one_pass(kind, shape, layout, chroma, env=None):
    """Does this batch run on the one-pass kernel (True) or on the per-output kernels (False)?  Written from the gates of
    launch_ks_fused (csrc/ipx_ks_fused.hip), not from what the library does: a gate that moves fails the test."""
    w, h, resize, thumb, wm = shape
    if (env or {}).get("IPX_FUSED") == "0":
        return False
    if resize and resize[1] > 2 * h:               # ks_fused_plan (csrc/ipx_ks_host.cpp): a source row feeds about 2 dh / sh destination rows at once, and
        return False                               # more than four (nacc > 4) has no one-pass plan: a large upscale
    off, es, ef = layout
    bpp = 4 if kind in ("rgba", "nrgba") else 1
    stride = w * bpp + es
    fs = h * stride + ef
    dword = lambda *v: all(x % 4 == 0 for x in v)
    if kind in ("rgba", "nrgba"):                  # pixels are dwords: pointer, row stride and frame stride multiples of 4; ragged rows are served
        return dword(off, stride, fs)
    if kind.startswith("paletted"):                # expanded to tight NRGBA frames in scratch
        return True
    if kind in DEEP_KINDS:                            # expanded to tight frames of taps in scratch: only ragged rows leave
        return w % 4 == 0
    if w % 4:                                      # planes: ragged rows only where a pixel is a dword
        return False
    if not dword(off, stride, fs):
        return False
    if kind == "gray":
        return True
    ratio = RATIO[kind]
    if ratio in (5, 6):                            # 4:1:1 and 4:1:0 load one byte of chroma per chunk (`al = hs == 2 ? 0 : ...`): planes of
        return True                                # (w + 3) // 4 columns and h or (h + 1) // 2 rows pass at any pointer, stride and frame stride
    cw, chh = (w + 1) // 2 if ratio in (1, 2) else w, (h + 1) // 2 if ratio in (2, 3) else h     # image.YCbCr's chroma planes
    coff, ces, cef = layout if chroma is None else chroma
    cstride = cw + ces
    cfs = chh * cstride + cef
    al = 2 if ratio in (1, 2) else 4               # 4:2:2 and 4:2:0 load a word of chroma per chunk, 4:4:4 and 4:4:0 a dword
    return all(x % al == 0 for x in (coff, cstride, cfs))
