"""Frames one pixel gives away: RGBA frames that are opaque except for ONE premultiplied pixel, for the speculative opaque pass of
the one-pass scaler (csrc/ipx_ks_fused.hip), the whole-image alpha scans of the per-operation scalers and png.Encode's choice of
colour type.  Helpers and the case table of tests/test_opaque_cases.py (CPU: the oracle held to the float64 reference, and every
probe shown to have teeth) and tests/test_opaque_spec_gpu.py (GPU: the kernels byte for byte against the oracle).  No GPU here.

A speculative item (one strip x row segment of a frame) that meets alpha != 0xff is redone by the four-channel kernel.  Where the
pixel sits decides which exit the item takes and which of a frame's items are redone at all, so the positions are swept densely:
every column at three rows and every row at three columns hit every row group, apron, segment, strip and chunk boundary of any
tiling, without restating the planner."""
import numpy as np

import oracle
import scaler_reference as R
from helpers import DEFAULT_COL, rgba_frames, text_glyphs
from scaler_cases import Source

KEYS = ("resize", "thumbnail", "watermark")
FORCED = {"IPX_KS_STRIPS": "3", "IPX_KS_SPLIT": "1", "IPX_KS_SPLIT_ROWS": "8"}
# every knob a case or a test of these files sets
KNOBS = sorted(set(FORCED) | {"IPX_KS_TAIL", "IPX_KS_FAST", "IPX_KS_FIX_CAP", "IPX_KS_SPEC", "IPX_KS_STATS", "IPX_KS_DEBUG", "IPX_FUSED",
                              "IPX_KS_TAPSPLIT", "IPX_KS_FAST_DBUF", "IPX_NO_FUSE"})

# name -> (w, h, resize, thumbnail, tiling knobs, probe alphas).  On a downscale a pixel of alpha 254 leaves no output byte with
# alpha < 255, so it cannot show a miss there: the downscales probe with 0 and 1, the equal-size case with 254 as well.
CASES = {
    "a": (300, 40, (200, 30, False), (24, True), FORCED, (0, 1)),          # three strips, five row segments of eight rows
    "b": (300, 40, (200, 30, False), (24, True), {}, (0, 1)),              # the same sizes at the tiling the planner picks
    "c301": (301, 40, (200, 30, False), (24, True), {}, (0, 1)),           # ragged last chunks of one, two and three pixels
    "c302": (302, 40, (200, 30, False), (24, True), {}, (0, 1)),
    "c303": (303, 40, (200, 30, False), (24, True), {}, (0, 1)),
    "d": (256, 96, (128, 48, False), (24, True), {}, (0, 1)),              # exactly 2:1, for boundary_frame
    "e": (61, 47, (61, 47, False), (24, True), {}, (0, 1, 254)),           # equal size: one tap of weight 1, the pixel survives exactly
}
SWEEP_CASES = ("a", "b", "c301", "c302", "c303")


def one_pixel_frames(w, h, positions, alpha, seed, base=None):
    """-> (len(positions) x h x w x 4 frames, base): copies of ONE opaque frame (helpers.rgba_frames, or `base`), copy i with alpha
    `alpha` at positions[i] = (x, y) and its colours clamped to it, as a premultiplied frame holds them."""
    if base is None:
        base = rgba_frames(1, w, h, seed=seed)[0]
    assert base.shape == (h, w, 4) and (base[..., 3] == 255).all()
    frames = np.repeat(base[None], len(positions), axis=0)
    for i, (x, y) in enumerate(positions):
        frames[i, y, x, :3] = np.minimum(frames[i, y, x, :3], alpha)
        frames[i, y, x, 3] = alpha
    return frames, base


def sweep(w, h):
    """every column at rows {0, h // 2, h - 1} and every row at columns {0, w // 2, w - 1}, each position once -> [(x, y)]"""
    out = [(x, y) for y in (0, h // 2, h - 1) for x in range(w)] + [(x, y) for x in (0, w // 2, w - 1) for y in range(h)]
    return list(dict.fromkeys(out))


def subset(w, h):
    """The positions the CPU half holds to the float64 reference, all of them in sweep(w, h): the corners; the rows either side of
    the first row group and of the first forced segment; the columns either side of the forced strips' boundaries (k * ceil(w / 3)
    rounded up to 4); the last column."""
    pos = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, h // 2)]
    pos += [(x, y) for y in (3, 4, 7, 8) if y < h for x in (0, w // 2, w - 1)]
    strip = (-(-w // 3) + 3) // 4 * 4
    for k in (1, 2):
        pos += [(x, y) for y in (0, h // 2) for x in range(k * strip - 2, k * strip + 2) if 0 <= x < w]
    pos = list(dict.fromkeys(pos))
    assert set(pos) <= set(sweep(w, h))
    return pos


def boundary_frame(w, h, seed=0xA11):
    """The period-2 tile of test_parity_gpu.test_values_exactly_on_a_rounding_boundary: per channel four values that sum to 510, so
    that under an exact 2:1 plan every interior value is 257 * 510 / 4 = 32767.5 -- + 0.5 is 128 * 256 exactly, which no float sum
    decides: every wave of the float pass lists pixels.  Opaque."""
    rng = np.random.default_rng(seed)
    f = np.full((h, w, 4), 255, np.uint8)
    for ch in range(3):
        a, b, c = (int(v) for v in rng.integers(100, 156, 3))
        f[0::2, 0::2, ch] = a; f[0::2, 1::2, ch] = b; f[1::2, 0::2, ch] = c; f[1::2, 1::2, ch] = 510 - a - b - c
    return f


def on_boundary(frame):
    """how many values of the exact 2:1 output of `frame` sit exactly on a rounding boundary (integer arithmetic: the interior
    weights are (1, 3, 3, 1) / 8 per axis; edge rows and columns have renormalised weights of their own and are left out)"""
    f = frame[..., :3].astype(np.int64)
    h, w = f.shape[:2]
    wy = np.array([1, 3, 3, 1])
    rows = sum(wy[k] * np.pad(f, ((1, 1), (0, 0), (0, 0)), mode="edge")[k:k + h:2] for k in range(4))[:h // 2]
    cols = sum(wy[k] * np.pad(rows, ((0, 0), (1, 1), (0, 0)), mode="edge")[:, k:k + w:2] for k in range(4))[:, :w // 2]
    return int(np.count_nonzero((257 * cols[1:-1, 1:-1] + 32) % (256 * 64) == 0))


def glyphs_for(w, h):
    """a short text at the bottom right whose boxes cover probe positions of rows h // 2 and h - 1 and of the last column"""
    return text_glyphs(w, h, n=6, width_px=min(120, w - 8), height_px=min(28, h - 4), margin=2)


def in_text(glyphs, x, y):
    return any(g["dr"][0] <= x < g["dr"][2] and g["dr"][1] <= y < g["dr"][3] for g in glyphs)


def expected(frame, case, glyphs=()):
    """the oracle's three outputs of one frame"""
    w, h, resize, thumb = CASES[case][:4]
    return oracle.process(frame, resize=resize, thumb=thumb, glyphs=glyphs, col=DEFAULT_COL)


def has_teeth(want):
    """A miss leaves the three-channel bytes, whose alpha is 0xff everywhere: the probe can show it only where the expected resize
    or thumbnail holds an alpha byte below 255.  (The watermark copy stores the staged pixels as they are, redone or not.)"""
    return bool((want["resize"][..., 3] < 255).any() or (want["thumbnail"][..., 3] < 255).any())


class Frame(Source):
    """a given RGBA frame as a scaler_cases.Source: the oracle's routines and the float64 reference of its operators"""

    def __init__(self, px):
        self.kind, self.h, self.w = "rgba", px.shape[0], px.shape[1]
        self.data = np.ascontiguousarray(px)
        self.ref = R.rgba(self.data)


def reference(frame, case):
    """-> (the oracle's outputs without text, the float64 reference's Refs) for one frame"""
    _, _, resize, thumb = CASES[case][:4]
    s = Frame(frame)
    want, stage1 = s.oracle_ops(resize, thumb)
    return want, s.ref_ops(resize, thumb, stage1)
