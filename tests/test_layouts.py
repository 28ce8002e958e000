"""CPU: the layout helpers of tests/layout_cases.py, and the oracle against the float64 reference at every kind, shape and operator
tests/test_layouts_gpu.py runs -- the expected bytes there stay inside the unchanged caps by the reference alone."""
import numpy as np
import pytest

import layout_cases as L
import layout_expected as E
from scaler_cases import KINDS


@pytest.mark.parametrize("bpp", [1, 2, 4, 8])
def test_lay_out_round_trips(bpp):
    rng = np.random.default_rng(bpp)
    n, h, w = 3, 7, 13
    frames = rng.integers(0, 256, (n, h, w * bpp), dtype=np.uint8)
    frames[frames == L.FILL] = 0                       # so that every 0xA5 below is padding
    for off, es, ef in L.SRC_LAYOUTS + L.CHROMA_LAYOUTS:
        buf, o, stride, fs = L.lay_out(frames, es, ef, off)
        assert (o, stride, fs) == (off, w * bpp + es, h * (w * bpp + es) + ef)
        back = np.stack([np.lib.stride_tricks.as_strided(buf[o + i * fs:], (h, w * bpp), (stride, 1)) for i in range(n)])
        np.testing.assert_array_equal(back, frames)
        assert int((buf != L.FILL).sum()) == int((frames != L.FILL).sum())     # nothing but the pixels was written
        assert buf.size >= o + (n - 1) * fs + (h - 1) * stride + w * bpp
    four = frames[:, :, :12].reshape(n, h, 3, 4)       # pixels in, as the JPEG corpus passes them
    np.testing.assert_array_equal(L.lay_out(four, 4, 0, 8)[0], L.lay_out(four.reshape(n, h, 12), 4, 0, 8)[0])


def test_the_jpeg_corpus_uses_this_lay_out():
    import jpeg_encode_corpus
    assert jpeg_encode_corpus.lay_out is L.lay_out


@pytest.mark.parametrize("layout", L.OUT_LAYOUTS + L.OUT_REFUSED)
def test_out_frames_round_trips_and_sees_one_byte(layout):
    off, ef = layout
    n, fb = 3, 52
    rng = np.random.default_rng(off * 16 + ef)
    frames = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    buf, first, fs = L.out_alloc(n, fb, off, ef)
    assert (buf == L.FILL).all() and first == L.GUARD + off and fs == fb + ef
    for i in range(n):
        buf[first + i * fs: first + i * fs + fb] = frames[i]
    np.testing.assert_array_equal(L.out_frames(buf, n, fb, first, fs), frames)
    assert L.out_frames(buf, n, fb, first, fs, (13, 4)).shape == (n, 13, 4)
    # every byte just outside a frame, and the ends of the allocation: one flipped byte fails the check
    outside = {0, first - 1, first + (n - 1) * fs + fb, buf.size - 1}
    for i in range(n - 1):
        if ef:
            outside |= {first + i * fs + fb, first + (i + 1) * fs - 1}
    for at in sorted(outside):
        bad = buf.copy()
        bad[at] ^= 1
        with pytest.raises(AssertionError, match="outside the frames"):
            L.out_frames(bad, n, fb, first, fs)
    # ... and every byte just inside one is a pixel: changing it is no error, and it comes back
    for i in range(n):
        for at in (first + i * fs, first + i * fs + fb - 1):
            ok = buf.copy()
            ok[at] ^= 1
            assert L.out_frames(ok, n, fb, first, fs)[i, at - first - i * fs] == buf[at] ^ 1


def test_the_layouts_are_what_the_gates_turn_on():
    assert L.TIGHT in L.SRC_LAYOUTS and L.MOST_PADDED in L.DWORD_LAYOUTS
    for off, es, ef in L.DWORD_LAYOUTS:
        assert off % 4 == 0 and es % 4 == 0 and ef % 4 == 0 and (off % 16 or es % 16 or ef % 16)
    for l in L.UNALIGNED_LAYOUTS:
        assert any(v % 4 for v in l)
    assert {v % 4 for l in L.CHROMA_LAYOUTS for v in l} == {0, 1, 2}
    for off, ef in L.OUT_LAYOUTS:
        assert off % 4 == 0 and ef % 4 == 0
    for l in L.OUT_REFUSED:
        assert any(v % 4 for v in l)
    assert {k for k in KINDS if k not in L.FULL_KINDS} and set(L.FULL_KINDS) <= set(KINDS)
    assert any(w & 3 for w, *_ in L.SHAPES) and any(not w & 3 for w, *_ in L.SHAPES)
    for w, h, *_ in L.SHAPES[:2]:                      # the glyph boxes reach the last column and the last row
        g = L.corner_glyphs(w, h)
        assert max(b["dr"][2] for b in g) == w and max(b["dr"][3] for b in g) == h
        assert any(b["dr"][2] == w and b["dr"][3] == h for b in g)


def test_the_path_table_is_consistent():
    """A sanity check of one_pass() itself, at the points its rules separate: it guards the table against a slip of the pen, not the
    library against anything -- what holds the library to the table is the comparison in test_layouts_gpu.test_batch_layouts."""
    s0, s1, s2 = L.SHAPES
    for kind in KINDS:
        assert not L.one_pass(kind, s2, L.TIGHT, None)                       # the upscale has no one-pass plan
        assert not L.one_pass(kind, s0, L.TIGHT, None, {"IPX_FUSED": "0"})
        assert L.one_pass(kind, s0, L.TIGHT, None) and L.one_pass(kind, s0, L.MOST_PADDED, None, {"IPX_KS_FAST": "0"})
        ragged_ok = kind in ("rgba", "nrgba") or kind.startswith("paletted")
        assert L.one_pass(kind, s1, L.TIGHT, None) == ragged_ok
    for kind in ("rgba", "nrgba", "gray", "ycbcr420", "ycbcr444", "ycbcr411", "ycbcr410"):
        for l in L.DWORD_LAYOUTS:
            assert L.one_pass(kind, s0, l, None)
        for l in L.UNALIGNED_LAYOUTS:
            assert not L.one_pass(kind, s0, l, None)
    for c in L.CHROMA_LAYOUTS:
        assert L.one_pass("ycbcr420", s0, L.TIGHT, c) == L.one_pass("ycbcr422", s0, L.TIGHT, c) == all(v % 2 == 0 for v in c)
        assert not L.one_pass("ycbcr444", s0, L.TIGHT, c) and not L.one_pass("ycbcr440", s0, L.TIGHT, c)
        assert L.one_pass("ycbcr411", s0, L.TIGHT, c) and L.one_pass("ycbcr410", s0, L.TIGHT, c)       # byte loads: no chroma layout leaves
        assert not L.one_pass("ycbcr411", s0, (1, 0, 0), c) and not L.one_pass("ycbcr411", s1, L.TIGHT, c)
    assert sum(any(v % 2 for v in c) for _, c in L.kind_layouts("ycbcr410") if c) == 2      # an odd pointer, odd strides
    assert sum(not L.one_pass("ycbcr410", s0, l, c) for l, c in L.kind_layouts("ycbcr410")) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_matches_the_reference(kind):
    for shape in L.SHAPES + ([L.HOST_GAP_SHAPE] if kind == "rgba" else []):
        E.case(kind, shape).check_reference()
