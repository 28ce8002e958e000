"""A float64 reference of jpeg.Encode's transform half, for tests/test_jpeg_reference.py and tests/test_jpeg_reference_gpu.py.

Written from ITU-T T.81 (A.3.3: the 8x8 FDCT of the level-shifted samples; A.3.4: quantisation; A.2.3 / A.2.4: 2x2 Y sampling and the
order of the blocks inside an MCU) and from the rules the header of csrc/ipx_jpeg.hip and DESIGN.md 4.5 quote from Go's writer -- not
from oracle/ipx_jpeg_oracle.c, which is one of the two things this reference judges (the other is the GPU encoder):
  * colour   color.RGBToYCbCr's integer formulas on the stored R, G, B bytes, alpha ignored (ycbcr()).  They are an integer rounding of
             the JFIF matrix; test_jpeg_reference.py checks all 2^24 triples against the real matrix before anything relies on them;
  * padding  edge pixels replicated to whole 16x16 MCUs;
  * chroma   the 2x2 box (a + b + c + d + 2) >> 2, in integers;
  * DCT      the real 2-D DCT-II of sample - 128 in float64 (orthonormal: T.81's 1/4 C(u) C(v) sum), divided by the quantiser the
             stream's own DQT segment carries.
Go then rounds half away from zero.  Its transform is libjpeg's fixed-point jfdctint, so next to a rounding boundary the integer code
may honestly land on either side: reference() gives, per coefficient, the real value x and the admissible set -- round-half-away(x)
alone when x is further than E / q from a half-integer, else the two integers around x.
"""
import numpy as np

# Error bound of the jfdctint transform (CONST_BITS 13, PASS1_BITS 2) against the real DCT, in unquantised DCT units.
# MEASURED on the CPU: the largest |oracle coefficient at quality 100 - x| - 0.5 over the corpus of tests/jpeg_encode_corpus.py
# (every frame kind at every geometry of GEOMETRIES plus the 4K photo frame; at quality 100 every quantiser is 1, so the figure is
# in unquantised units) is E_SEEN; E is 1.5 x that.  tests/test_jpeg_reference.py::test_error_bound_holds_on_the_cpu recomputes the
# figure and asserts it stays under E.  Nothing here was taken from the GPU's output.
E_SEEN = 0.1629
E = 0.2443

# The largest share of ambiguous coefficients (x within E / q of a half-integer) a case may have, per quality: about twice the most the
# reference alone shows over this suite's cases (SEEN_AMBIGUOUS, computed on the CPU by `python tests/jpeg_encode_corpus.py --caps`;
# test_jpeg_reference.py::test_ambiguous_shares_stay_under_their_caps holds every case to it).  At quality 100 every quantiser is 1
# and a large part of all values is honestly undecided: the cap is kept, the weight of the check lies at 85, 50 and 20.
SEEN_AMBIGUOUS = {85: 0.0521, 50: 0.0130, 20: 0.0052, 100: 0.4844}
MAX_AMBIGUOUS = {85: 0.105, 50: 0.026, 20: 0.0105, 100: 0.97}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])          # T.81 figure A.6: natural index of the zig-th coefficient

# JFIF: Y = Kr R + (1 - Kr - Kb) G + Kb B, Cb = 128 + (B - Y) / (2 - 2 Kb), Cr = 128 + (R - Y) / (2 - 2 Kr), Kr = 0.299, Kb = 0.114
JFIF = np.array([[0.299, 0.587, 0.114],
                 [-0.299 / 1.772, -0.587 / 1.772, 0.5],
                 [0.5, -0.587 / 1.402, -0.114 / 1.402]])
COLOUR_TOLERANCE = 0.5 + 2.0 ** -7


def cap(quality):
    return MAX_AMBIGUOUS[quality]


def ycbcr(r, g, b):
    """color.RGBToYCbCr in integers (int64 arrays in, int64 arrays out): 16-bit fixed point, rounded; Cb / Cr clamped to 0..255"""
    r, g, b = (np.asarray(v, np.int64) for v in (r, g, b))
    y = (19595 * r + 38470 * g + 7471 * b + (1 << 15)) >> 16
    cb = np.clip((-11056 * r - 21712 * g + 32768 * b + (257 << 15)) >> 16, 0, 255)
    cr = np.clip((32768 * r - 27440 * g - 5328 * b + (257 << 15)) >> 16, 0, 255)
    return y, cb, cr


def jfif_real(r, g, b):
    """the real JFIF matrix value of each channel, clamped to 0..255 (float64)"""
    rgb = np.stack([np.asarray(v, np.float64) for v in (r, g, b)])
    out = np.tensordot(JFIF, rgb, 1)
    out[1:] += 128.0
    return np.clip(out, 0.0, 255.0)


def planes(frame):
    """H x W x 4 uint8 -> (Y, Cb, Cr) int64: Y of whole MCUs (16 mh x 16 mw), Cb / Cr after the box (8 mh x 8 mw)"""
    f = np.asarray(frame)
    h, w = f.shape[:2]
    ph, pw = -h % 16, -w % 16
    f = np.pad(f[..., :3], ((0, ph), (0, pw), (0, 0)), mode="edge")
    y, cb, cr = ycbcr(f[..., 0], f[..., 1], f[..., 2])

    def box(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return y, box(cb), box(cr)


def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    m = np.cos((2 * n + 1) * k * np.pi / 16.0) / 2.0
    m[0] /= np.sqrt(2.0)
    return m


_D = _dct_matrix()


def dct_blocks(plane):
    """(8 R) x (8 C) samples -> R x C x 64 real DCT-II coefficients of sample - 128, natural order"""
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    b = (plane.astype(np.float64) - 128.0).reshape(r, 8, c, 8).transpose(0, 2, 1, 3)
    out = np.einsum("ui,rcij,vj->rcuv", _D, b, _D, optimize=True)
    for u in (0, 4):                                                 # EXACT_NATURAL: integer sums / 8, exact in float64, so that ties stay ties
        for v in (0, 4):
            su, sv = (_SIGN4 if u else np.ones(8, np.int64)), (_SIGN4 if v else np.ones(8, np.int64))
            out[:, :, u, v] = np.einsum("i,rcij,j->rc", su, b, sv) / 8.0
    return out.reshape(r, c, 64)


def dqt_tables(stream):
    """the quantisers of a stream's DQT segments -> {table id: 64 values in zig-zag order, as the segment carries them}"""
    b = bytes(stream)
    assert b[:2] == b"\xff\xd8"
    i, out = 2, {}
    while b[i + 1] != 0xDA:
        assert b[i] == 0xFF
        n = b[i + 2] << 8 | b[i + 3]
        if b[i + 1] == 0xDB:
            p = i + 4
            while p < i + 2 + n:
                assert b[p] >> 4 == 0, "8-bit tables only"
                out[b[p] & 15] = np.frombuffer(b[p + 1:p + 65], np.uint8).astype(np.int64)
                p += 65
        i += 2 + n
    return out


# Four coefficients of a block take no multiplication in jfdctint: (0,0), (0,4), (4,0) and (4,4) are sums and differences of the samples,
# scaled by PASS1_BITS in the row pass and descaled in the column pass without loss (the sums are multiples of 4).  Their real value is
# the same signed sum / 8, so for them the transform's error bound is 0, DERIVED, and a tie is decided by the rounding rule alone.
EXACT_NATURAL = (0, 4, 32, 36)
_SIGN4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])              # cos((2 n + 1) 4 pi / 16) * sqrt(2)
E_ZIG = np.where(np.isin(ZIGZAG, EXACT_NATURAL), 0.0, 1.0)      # x E: the bound per coefficient, zig-zag order


class Ref:
    """x: the real quantised value of every coefficient, (MCUs, 6, 64), blocks in scan order Y0 Y1 Y2 Y3 Cb Cr, zig-zag order inside a
    block -- the layout of the product's and the oracle's coefficient arrays; lo / hi: the admissible integers (lo == hi where clear)"""

    def __init__(self, x, q):
        self.x = x
        a = np.abs(x)
        near = np.abs(a - np.floor(a) - 0.5) * q < E * E_ZIG    # within E / q of a half-integer (never, where the transform is exact)
        rnd = np.sign(x) * np.floor(a + 0.5)                       # round half away from zero
        self.lo = np.where(near, np.floor(x), rnd).astype(np.int64)
        self.hi = np.where(near, np.ceil(x), rnd).astype(np.int64)
        self.ambiguous = float(near.mean())


def real_coefficients(frame):
    """the unquantised real DCT of a frame in the product's layout: (MCUs, 6, 64) float64"""
    y, cb, cr = planes(frame)
    mh, mw = y.shape[0] // 16, y.shape[1] // 16
    out = np.empty((mh, mw, 6, 64), np.float64)
    yb = dct_blocks(y)                                               # 2 mh x 2 mw x 64
    for j in range(4):                                               # T.81 A.2.3: the four Y blocks of an MCU, left to right, top to bottom
        out[:, :, j] = yb[j >> 1::2, j & 1::2][..., ZIGZAG]
    out[:, :, 4] = dct_blocks(cb)[..., ZIGZAG]
    out[:, :, 5] = dct_blocks(cr)[..., ZIGZAG]
    return out.reshape(mh * mw, 6, 64)


def reference(frame, dqt):
    """frame: H x W x 4 uint8; dqt: dqt_tables() of the stream under test (table 0: Y, table 1: Cb and Cr, as SOF0 says) -> Ref"""
    q = np.stack([dqt[0]] * 4 + [dqt[1]] * 2).astype(np.float64)    # 6 x 64, zig-zag order like the coefficients
    return Ref(real_coefficients(frame) / q, q)


def assert_matches(got, ref, cap, what=""):
    """every coefficient of `got` (MCUs, 6, 64) lies in its admissible set, and the case's ambiguous share stays under `cap`"""
    got = np.asarray(got).astype(np.int64).reshape(ref.x.shape)
    bad = (got != ref.lo) & (got != ref.hi)
    if bad.any():
        m, j, z = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d coefficients outside the reference; first at MCU %d block %d zig %d: got %d, real value %.4f"
                             % (what, int(bad.sum()), bad.size, m, j, z, got[m, j, z], ref.x[m, j, z]))
    assert ref.ambiguous <= cap, "%s: %.4f of the coefficients are ambiguous, the cap is %.4f" % (what, ref.ambiguous, cap)


def scan_order_of(decoded_coefs):
    """tests/jpeg_decode_model.py decode(..., want_coefs=True)["coefs"] of a 4:2:0 stream -> (MCUs, 6, 64) in scan order"""
    yb, cb, cr = decoded_coefs
    mh, mw = cb.shape[0], cb.shape[1]
    out = np.empty((mh, mw, 6, 64), np.int64)
    for j in range(4):
        out[:, :, j] = yb[j >> 1::2, j & 1::2]
    out[:, :, 4] = cb
    out[:, :, 5] = cr
    return out.reshape(mh * mw, 6, 64)
