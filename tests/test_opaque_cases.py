"""CPU half of tests/test_opaque_spec_gpu.py: the expected bytes of the one-pixel frames (tests/opaque_cases.py) rest on the float64
reference of tests/scaler_reference.py, not on the code under test, and every probe has teeth.

Per case and probe alpha, on opaque_cases.subset (corners, the rows either side of the first row group and of the first forced
segment, the columns either side of the forced strip boundaries, the last column):
  * the oracle matches the reference within scaler_cases.cap("rgba");
  * the expected resize or thumbnail holds an alpha byte below 255 -- else the position could not show a miss and is dropped from
    the GPU table, and this test names it;
  * the opaque base frame's outputs, offered as the result for the probe frame, FAIL the comparison with the reference: a kernel
    that misses the pixel leaves exactly those bytes.
Over the whole sweep no more than a tenth of the positions may lack teeth (oracle only)."""
import numpy as np
import pytest

import opaque_cases as OC
import scaler_reference as R
from scaler_cases import cap

PARAMS = [(c, a) for c in OC.CASES for a in OC.CASES[c][5]]


@pytest.mark.parametrize("case,alpha", PARAMS)
def test_oracle_matches_reference_and_probes_have_teeth(case, alpha):
    w, h = OC.CASES[case][:2]
    pos = OC.subset(w, h)
    frames, base = OC.one_pixel_frames(w, h, pos, alpha, seed=w * 31 + h)
    missed, _ = OC.reference(base, case)                      # what a kernel that never sees the pixel stores
    dropped = []
    for i, p in enumerate(pos):
        want, ref = OC.reference(frames[i], case)
        for k in OC.KEYS:
            R.assert_matches(want[k], *ref[k], max_ambiguous=cap("rgba"), what="case %s alpha %d pixel %r %s" % (case, alpha, p, k))
        if not OC.has_teeth(want):
            dropped.append(p)
            continue
        caught = 0
        for k in ("resize", "thumbnail"):
            if (want[k][..., 3] < 255).any():
                assert not np.array_equal(missed[k], want[k])
                with pytest.raises(AssertionError):
                    R.assert_matches(missed[k], *ref[k], max_ambiguous=cap("rgba"), what="mutation")
                caught += 1
        assert caught, p
    if dropped:
        print("case %s alpha %d: no output alpha below 255 for the pixel at %r: dropped from the GPU table" % (case, alpha, dropped))
    assert len(dropped) * 10 <= len(pos), dropped


@pytest.mark.parametrize("case,alpha", [(c, a) for c, a in PARAMS if c in OC.SWEEP_CASES and c != "b"])
def test_at_most_a_tenth_of_the_sweep_lacks_teeth(case, alpha):
    w, h = OC.CASES[case][:2]
    pos = OC.sweep(w, h)
    assert len(pos) == 3 * w + 3 * h - 9
    frames, _ = OC.one_pixel_frames(w, h, pos, alpha, seed=w * 31 + h)
    dropped = [p for i, p in enumerate(pos) if not OC.has_teeth(OC.expected(frames[i], case))]
    if dropped:
        print("case %s alpha %d: dropped from the GPU table: %r" % (case, alpha, dropped))
    assert len(dropped) * 10 <= len(pos), dropped


def test_pixels_outside_the_crop_square_change_only_the_resize():
    """(expected, and the reason has_teeth looks at both outputs)"""
    w, h = OC.CASES["a"][:2]
    frames, base = OC.one_pixel_frames(w, h, [(0, 0), (w // 2, h // 2)], 0, seed=w * 31 + h)
    b, out, mid = OC.expected(base, "a"), OC.expected(frames[0], "a"), OC.expected(frames[1], "a")
    assert np.array_equal(out["thumbnail"], b["thumbnail"]) and not np.array_equal(out["resize"], b["resize"])
    assert not np.array_equal(mid["thumbnail"], b["thumbnail"]) and not np.array_equal(mid["resize"], b["resize"])


def test_boundary_frame_lists_every_interior_pixel():
    w, h = OC.CASES["d"][:2]
    f = OC.boundary_frame(w, h)
    assert (f[..., 3] == 255).all()
    assert OC.on_boundary(f) == 3 * (w // 2 - 2) * (h // 2 - 2)
    want, ref = OC.reference(f, "d")
    for k in OC.KEYS:   # every interior byte of the resize is ambiguous by construction: only the +-1 condition and the watermark bind here
        R.assert_matches(want[k], *ref[k], max_ambiguous=1.0, what="boundary frame %s" % k)


def test_glyph_boxes_cover_probe_positions():
    for case in OC.SWEEP_CASES + ("d", "e"):
        w, h = OC.CASES[case][:2]
        g = OC.glyphs_for(w, h)
        covered = [p for p in OC.sweep(w, h) if OC.in_text(g, *p)]
        assert len(covered) >= 10 and len(covered) < len(OC.sweep(w, h)) // 2, (case, len(covered))
