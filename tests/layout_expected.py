"""Expected outputs of the cases of tests/layout_cases.py: per kind and shape N sources with the oracle's outputs and the float64
reference's, which never see a layout.  Computed once, shared by tests/test_layouts.py and tests/test_layouts_gpu.py, never changed."""
import numpy as np

import oracle
import scaler_reference as R
from layout_cases import COL, N, corner_glyphs
from scaler_cases import Source, cap


class Case:
    """One kind at one shape: N sources, per frame the oracle's outputs and the reference's (want[i][k], ref[i][k]), the glyphs, and the
    watermark frames with the text (want_text[i])."""

    def __init__(self, kind, shape):
        w, h, resize, thumb, wm = shape
        self.kind, self.shape = kind, shape
        self.srcs = [Source(kind, w, h, seed=w * 131 + h * 7 + i) for i in range(N)]
        self.keys = [k for k, on in (("resize", resize), ("thumbnail", thumb), ("watermark", wm)) if on]
        self.glyphs = corner_glyphs(w, h) if wm else None
        self.want, self.ref, self.want_text = [], [], []
        for s in self.srcs:
            o, stage1 = s.oracle_ops(resize or (w, h, False), thumb or (8, False))
            r = s.ref_ops(resize or (w, h, False), thumb or (8, False), stage1)
            self.want.append({k: o[k] for k in self.keys})
            self.ref.append({k: r[k] for k in self.keys})
            self.want_text.append(oracle.composite_glyphs(o["watermark"].copy(), self.glyphs, COL) if wm else None)

    def planes(self):
        """the source as the batch entries take it: [n x H x row bytes] per plane (YCbCr: y, cb, cr), and the palettes or None"""
        k = self.kind
        if k.startswith("ycbcr"):
            return [np.stack([s.data[c] for s in self.srcs]) for c in range(3)], None
        if k.startswith("paletted"):
            return [np.stack([s.data[0] for s in self.srcs])], np.stack([s.data[1] for s in self.srcs])
        return [np.stack([s.data for s in self.srcs]).reshape(N, self.shape[1], -1)], None

    def check_reference(self):
        """the CPU half: the oracle's bytes stay inside the caps by the reference alone"""
        for i in range(N):
            for k in self.keys:
                R.assert_matches(self.want[i][k], *self.ref[i][k], max_ambiguous=cap(self.kind), what="%s %s frame %d %r" % (self.kind, k, i, self.shape))


_cases = {}


def case(kind, shape):
    """computed once, shared, and never changed by a test"""
    key = (kind, shape)
    if key not in _cases:
        _cases[key] = Case(kind, shape)
    return _cases[key]
