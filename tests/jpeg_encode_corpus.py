"""Frames, geometries, memory layouts, batches and stream-length recipes for the encoder tests (tests/test_jpeg_reference.py on the
CPU, tests/test_jpeg_reference_gpu.py on the GPU).  Everything is built from seeds; nothing large is committed.

`python tests/jpeg_encode_corpus.py --search` is the CPU search (with the oracle) that found STREAM_RECIPES and PHASE_RECIPE;
`--caps` prints the figures written beside E and MAX_AMBIGUOUS in tests/jpeg_encode_reference.py.  No search runs at test time:
test_jpeg_reference.py::test_stream_length_edges_are_present asserts every property on the committed list."""
import numpy as np

from layout_cases import lay_out  # noqa: F401  (n x H x W x 4 -> (allocation, offset, stride, frame stride); the padding is 0xA5)

KINDS = ["noise", "binary", "smooth", "photo", "checker", "translucent", "edge"]
EXTRA_KINDS = ["flat", "basis"]


def frame(kind, w, h, seed):
    """H x W x 4 uint8 as an *image.RGBA holds it"""
    rng = np.random.default_rng([seed, w, h, (KINDS + EXTRA_KINDS).index(kind)])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int32)
    f = np.empty((h, w, 4), np.uint8)
    f[..., 3] = 255
    if kind == "noise":
        f[...] = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "binary":                      # the largest coefficients, the longest codes, the most 0xff bytes
        f[..., :3] = rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255
    elif kind in ("smooth", "translucent", "edge"):
        f[..., 0] = (np.sin(xx / 23.0 + seed) * 100 + 128).clip(0, 255)
        f[..., 1] = (np.cos(yy / 17.0 - seed) * 100 + 128).clip(0, 255)
        f[..., 2] = (xx * 3 + yy * 2 + seed * 11) % 256
        if kind == "translucent":               # premultiplied, alpha of every value: jpeg.Encode reads R, G, B as stored
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            f[..., 3] = a
            f[..., :3] = (f[..., :3].astype(np.int32) * a[..., None].astype(np.int32) // 255).astype(np.uint8)
        if kind == "edge":                      # the last column and the last row differ sharply from their neighbours
            f[:, -1, :3] = 255 - f[:, max(w - 2, 0), :3] // 2 if w > 1 else 255
            f[-1, :, :3] = 255 - f[max(h - 2, 0), :, :3] // 2 if h > 1 else 0
            f[-1, -1, :3] = (255, 0, 255)
    elif kind == "photo":                       # gradients + noise + a flat patch
        n = rng.integers(-12, 13, (h, w, 3), dtype=np.int16)
        f[..., 0] = (xx * 255 // max(w - 1, 1) + n[..., 0]).clip(0, 255)
        f[..., 1] = (yy * 255 // max(h - 1, 1) + n[..., 1]).clip(0, 255)
        f[..., 2] = (128 + ((xx + yy) % 512 - 256) // 3 + n[..., 2]).clip(0, 255)
        f[h // 4:h // 2, w // 3:2 * w // 3, :3] = (200, 120, 40)
    elif kind == "checker":
        f[..., :3] = ((xx + yy) % 2 * 255)[..., None]
    elif kind == "basis":                       # black / white by the sign of one DCT basis function per 8x8 block: the largest value
        k, n = np.mgrid[0:8, 0:8]               # every single coefficient can take, where a wrong transform constant shows most
        c = np.cos((2 * n + 1) * k * np.pi / 16.0)
        u, v = (yy // 8 + seed) % 8, (xx // 8) % 8
        f[..., :3] = ((c[u, yy % 8] * c[v, xx % 8] > 0) * 255)[..., None]
    elif kind == "flat":
        f[..., :3] = (seed * 37 % 256, seed * 101 % 256, seed * 53 % 256)
    else:
        raise ValueError(kind)
    return f


# ---- geometries ----------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 7, 8, 9, 15, 16, 17, 112, 113, 127, 128, 129, 143, 144, 145, 257]     # around the block, the MCU and the 8-MCU workgroup
HEIGHTS = [1, 15, 16, 17, 33]
# (kind, w, h, seed): every kind meets every residue of the grid (7 kinds against 5 heights and 16 widths)
GEOMETRIES = [(KINDS[(i * len(HEIGHTS) + j) % len(KINDS)], w, h, 100 + i * len(HEIGHTS) + j)
              for i, w in enumerate(WIDTHS) for j, h in enumerate(HEIGHTS)]
# every (u, v) basis pattern in luma, 16 x 16 MCUs in two alignments of the patterns
GEOMETRIES += [("basis", 64, 64, 0), ("basis", 64, 64, 1), ("basis", 128, 64, 3)]
QUALITIES = [85, 50, 20, 100]
# one photo-like frame each at quality 85 (BASELINE config 5: the watermark output is encoded at source size)
LARGE = [("photo", 3840, 2160, 1), ("photo", 7680, 4320, 2)]
# the longest sides the entries accept; 65535 = 16 * 4095 + 15, so the last MCU is partial
LONG = [("noise", 65535, 1, 3), ("noise", 1, 65535, 4), ("edge", 65535, 17, 5), ("edge", 17, 65535, 6)]


def reference_cases():
    """(kind, w, h, seed, quality) the float64 reference is computed for: every geometry at every quality of QUALITIES, the 4K frame"""
    return [g + (q,) for g in GEOMETRIES for q in QUALITIES] + [LARGE[0] + (85,)]


# ---- layouts: the same pixels at other strides, frame strides and pointer alignments ----------------------------------------------
# (name, stride - 4 w, frame stride padding on top of h * stride, byte offset of the first frame into the allocation)
LAYOUTS = [("stride 4w+4", 4, 0, 0), ("stride 4w+12", 12, 0, 0), ("stride 4w+16", 16, 0, 0),
           ("frame stride + 4", 0, 4, 0), ("frame stride + 24, stride 4w+16", 16, 24, 0),
           ("pointer + 4", 0, 0, 4), ("pointer + 8", 0, 0, 8), ("pointer + 12", 0, 0, 12),
           ("pointer + 12, stride 4w+16, frame stride + 16", 16, 16, 12)]
# (w, h, n): whole workgroups (128 x 16 pixels) that take the aligned 16-byte loads when the layout allows, next to partial ones; the
# widths are multiples of 4, so that the tightly packed call itself is the aligned one (stride and frame stride multiples of 16)
LAYOUT_SHAPES = [(128, 16, 3), (260, 33, 2), (144, 17, 2), (132, 48, 1), (512, 64, 2)]


# ---- stream-length edges ----------------------------------------------------------------------------------------------------
# The stuffing kernel works on 64-byte chunks of the UNSTUFFED scan, 256 chunks (16 KiB) per workgroup, and shifts each workgroup's
# piece by (header length + piece start + 0xff bytes before it) mod 16.  (property, (kind, w, h, seed, quality)); found by --search.
STREAM_RECIPES = [
    ("64k-1", ("noise", 27, 17, 30, 85)),
    ("64k", ("binary", 26, 21, 29, 100)),
    ("64k+1", ("binary", 32, 21, 89, 100)),
    ("16384-1", ("binary", 112, 64, 22466, 100)),
    ("16384", ("binary", 112, 64, 24889, 100)),
    ("16384+1", ("binary", 112, 64, 7474, 100)),
    ("ff ends a chunk", ("noise", 24, 17, 0, 85)),
    ("ff ends a piece", ("binary", 113, 64, 11, 100)),
    ("ff is the last byte", ("binary", 31, 19, 7, 100)),
]
# one long quality-100 stream whose pieces after the first show all 16 shifts
PHASE_RECIPE = ("binary", 640, 512, 0, 100)

CHUNK, PIECE = 64, 16384


def scan_of(stream):
    """(header length, the entropy-coded bytes as written, the same with every 0xff 0x00 reduced to 0xff)"""
    b = bytes(stream)
    i = 2
    while b[i + 1] != 0xDA:
        i += 2 + (b[i + 2] << 8 | b[i + 3])
    i += 2 + (b[i + 2] << 8 | b[i + 3])
    assert b[-2:] == b"\xff\xd9"
    scan = b[i:-2]
    return i, scan, scan.replace(b"\xff\x00", b"\xff")


def phases(stream):
    """the shifts (header length + piece start + 0xff bytes before it) mod 16 of the pieces after the first"""
    hdr, _, u = scan_of(stream)
    a = np.frombuffer(u, np.uint8)
    before = np.concatenate([[0], np.cumsum(a == 0xFF)])
    return {int((hdr + p + before[p]) % 16) for p in range(PIECE, len(u), PIECE)}


PROPERTIES = {
    "64k-1": lambda u: len(u) % CHUNK == CHUNK - 1 and len(u) > CHUNK,
    "64k": lambda u: len(u) % CHUNK == 0 and len(u) > CHUNK,
    "64k+1": lambda u: len(u) % CHUNK == 1 and len(u) > CHUNK,
    "16384-1": lambda u: len(u) == PIECE - 1,
    "16384": lambda u: len(u) == PIECE,
    "16384+1": lambda u: len(u) == PIECE + 1,
    "ff ends a chunk": lambda u: any(u[i] == 0xFF for i in range(CHUNK - 1, len(u) - 1, CHUNK)),
    "ff ends a piece": lambda u: len(u) > PIECE + 1 and u[PIECE - 1] == 0xFF,
    "ff is the last byte": lambda u: len(u) > 1 and u[-1] == 0xFF,
}


def _search():
    import oracle
    found = {}

    def tryit(names, kind, w, h, seed, q):
        u = scan_of(oracle.jpeg_encode_rgba(frame(kind, w, h, seed), q))[2]
        for n in names:
            if n not in found and PROPERTIES[n](u):
                found[n] = (kind, w, h, seed, q)
        return len(u)
    small = ["64k-1", "64k", "64k+1", "ff ends a chunk", "ff is the last byte"]
    for seed in range(4000):
        if all(n in found for n in small):
            break
        tryit(small, "binary" if seed & 1 else "noise", 24 + seed % 9, 17 + seed % 5, seed, 100 if seed & 1 else 85)
    near = ["16384-1", "16384", "16384+1", "ff ends a piece"]
    for w in (113, 112, 114):                    # binary noise of 112 x 64 at quality 100: 16 274 bytes on average, 34 either way
        for seed in range(30000):
            if all(n in found for n in near):
                break
            tryit(near, "binary", w, 64, seed, 100)
    print("STREAM_RECIPES = [")
    for n in PROPERTIES:
        print("    (%r, %r)," % (n, found.get(n)))
    print("]")
    for w, h in ((512, 512), (640, 512), (768, 512), (768, 640)):
        for seed in range(6):
            r = ("binary", w, h, seed, 100)
            if len(phases(oracle.jpeg_encode_rgba(frame(*r[:4]), 100))) == 16:
                print("PHASE_RECIPE = %r" % (r,))
                return


def _caps():
    import oracle
    import jpeg_encode_reference as R
    R.E = 1e9                                    # (the figures below do not depend on it)
    worst = 0.0
    for kind, w, h, seed in GEOMETRIES + LARGE[:1]:
        f = frame(kind, w, h, seed)
        data, coefs = oracle.jpeg_encode_rgba(f, 100, want_coefs=True)
        assert (R.dqt_tables(data)[0] == 1).all() and (R.dqt_tables(data)[1] == 1).all()
        worst = max(worst, float(np.abs(coefs - R.real_coefficients(f)).max()) - 0.5)
    print("E_SEEN = %.4f\nE = %.4f" % (worst, 1.5 * worst))
    R.E = 1.5 * worst
    seen = {}
    for kind, w, h, seed, q in reference_cases():
        f = frame(kind, w, h, seed)
        r = R.reference(f, R.dqt_tables(oracle.jpeg_encode_rgba(f, q)))
        seen[q] = max(seen.get(q, 0.0), r.ambiguous)
    print("SEEN_AMBIGUOUS = %r" % ({q: round(v, 4) for q, v in seen.items()},))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _search() if "--search" in sys.argv else _caps()
