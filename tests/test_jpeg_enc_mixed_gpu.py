"""GPU: jpeg.Encode of frames of mixed sizes in one call (ipx_jpeg_encode_mixed_dev; the records: csrc/ipx_jpeg_enc_mixed_plan.h;
DESIGN.md section 4.6), and the mixed-size JPEG leg's route through it.

Every stream of a mixed call is held byte for byte against ipx_jpeg_encode_batch_dev of that frame in a call of its own, and a subset
against oracle/ipx_jpeg_oracle.c.  The frames are the smallest at which the per-frame indexing can go wrong: one MCU, replicated
edges, one transform workgroup per row exactly and one more, a last workgroup of one MCU, many one-MCU rows, 264 blocks (one full
sizing workgroup and a partial one), a long noisy scan between flat ones, strides and bases that choose the 16-byte load path per frame.
The leg's streams are held against ipx_plan_run_jpeg_jpeg with a plan of each file's size."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
# (size, the edge it reaches); kMcuPerWg is 8, so 128 pixels is one transform workgroup wide
EDGES = [(1, 1), (16, 16), (17, 15), (128, 16), (129, 16), (1040, 16), (16, 129), (176, 64)]
KINDS = ("noise", "flat", "gradient")
LAYOUTS = ("stride16", "pad4", "off4")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


def frame(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 4, dtype=np.uint8), (h, w, 4)).copy()
    y, x = np.mgrid[0:h, 0:w]
    a, b = (int(v) for v in rng.integers(1, 9, 2))
    return np.stack([(a * x + y) & 255, (x + b * y) & 255, (a * x + b * y) >> 1 & 255, np.full((h, w), 255)], axis=-1).astype(np.uint8)


class Frames:
    """host frames laid out in one HBM allocation, each its own way: 'stride16' (base and stride multiples of 16: the 16-byte load
    path), 'pad4' (stride 4 w + 4), 'off4' (a base 4 bytes off 16-byte alignment).  The padding is 0xA5.  recs[i] = (ptr, w, h, stride)"""

    def __init__(self, ctx, frames, layouts):
        self.ctx, self.host, self.layouts = ctx, frames, layouts
        place, at = [], 0
        for f, lay in zip(frames, layouts):
            h, w = f.shape[:2]
            stride = {"stride16": (4 * w + 15) & ~15, "pad4": 4 * w + 4, "off4": (4 * w + 15) & ~15}[lay]
            off = at + (4 if lay == "off4" else 0)
            place.append((off, w, h, stride))
            at = (off + stride * h + 255) & ~255
        buf = np.full(max(at, 256), 0xA5, np.uint8)
        for f, (off, w, h, stride) in zip(frames, place):
            rows = np.lib.stride_tricks.as_strided(buf[off:], (h, 4 * w), (stride, 1))
            rows[:] = f.reshape(h, 4 * w)
        self.buf = ctx.alloc(buf.nbytes).upload(buf)
        assert self.buf.ptr % 256 == 0
        self.recs = [(self.buf.ptr + off, w, h, stride) for off, w, h, stride in place]
        self._alone = {}

    def alone(self, i, quality):
        """ipx_jpeg_encode_batch_dev of frame i in a call of its own, computed once"""
        if (i, quality) not in self._alone:
            ptr, w, h, stride = self.recs[i]
            self._alone[i, quality] = self.ctx.jpeg_encode_batch_dev(ptr, w, h, 1, quality, stride=stride, frame_stride=(stride * h + 255) & ~255)[0]
        return self._alone[i, quality]

    def check(self, order, quality, oracle_every=0):
        """one mixed call of the frames `order`; every stream against the uniform entry, every oracle_every-th against the oracle"""
        got = self.ctx.jpeg_encode_mixed_dev([self.recs[i] for i in order], quality)
        assert len(got) == len(order)
        for k, i in enumerate(order):
            what = "frame %d (%dx%d, %s) at place %d of %d, quality %d" % (i, self.recs[i][1], self.recs[i][2], self.layouts[i], k, len(order), quality)
            assert got[k] == self.alone(i, quality), what
            if oracle_every and k % oracle_every == 0:
                assert got[k] == oracle.jpeg_encode_rgba(self.host[i], quality), what + " against the oracle"
        return got

    def free(self):
        self.buf.free()


@pytest.fixture(scope="module")
def edges(ctx):
    """the eight edge sizes, each in the three kinds and the three layouts (frame j: size j // 3, kind and layout by j)"""
    frames = [frame(KINDS[(s + k) % 3], w, h, 100 * s + k) for s, (w, h) in enumerate(EDGES) for k in range(3)]
    layouts = [LAYOUTS[k] for s in range(len(EDGES)) for k in range(3)]
    f = Frames(ctx, frames, layouts)
    yield f
    f.free()


@pytest.mark.parametrize("order", ["forward", "reverse", "shuffled"])
def test_the_transforms_edges_in_one_call(ctx, edges, order):
    """Every edge size in every layout, 24 frames in one call, forward, reversed and shuffled: every size is first, last and beside
    every kind of neighbour, and the 16-byte load path is chosen per frame."""
    idx = list(range(len(edges.recs)))
    if order == "reverse":
        idx = idx[::-1]
    if order == "shuffled":
        random.Random(20261021).shuffle(idx)
    got = edges.check(idx, 85, oracle_every=3 if order == "forward" else 0)
    # a stream carries its own frame's size in SOF0
    for k, i in enumerate(idx):
        sof = got[k].index(b"\xff\xc0")
        assert (int.from_bytes(got[k][sof + 5:sof + 7], "big"), int.from_bytes(got[k][sof + 7:sof + 9], "big")) == (edges.recs[i][2], edges.recs[i][1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_layout_per_call(ctx, edges, layout):
    """the same frames with every frame of the call in one layout"""
    edges.check([i for i in range(len(edges.recs)) if edges.layouts[i] == layout], 85)


@pytest.mark.parametrize("quality", [1, 50, 85, 100])
def test_qualities(ctx, edges, quality):
    edges.check(list(range(0, len(edges.recs), 2)) + [23], quality, oracle_every=4)


def _scan_bits(ctx, monkeypatch, rec):
    """the length of a frame's scan in bits, as the uniform encoder's refusal reports it"""
    import imageprocessor_amd as ipx
    monkeypatch.setenv("IPX_JPEG_MAX_SCAN_BITS", "1")
    try:
        with pytest.raises(ipx.IpxError) as e:
            ctx.jpeg_encode_batch_dev(rec[0], rec[1], rec[2], 1, 100, stride=rec[3], frame_stride=(rec[3] * rec[2] + 255) & ~255)
    finally:
        monkeypatch.delenv("IPX_JPEG_MAX_SCAN_BITS")
    return int(re.search(r"\((\d+) bits", e.value.text).group(1))


def test_byte_stuffing(ctx, monkeypatch):
    """A 256 x 256 noise frame at quality 100 -- hundreds of 0xff bytes, over a thousand chunks, several stuffing workgroups -- between
    16 x 16 flat frames whose scans fit one chunk with no 0xff at all: a frame's chunk count and 0xff offsets are its own.  With them,
    a frame whose scan ends on a byte boundary (no padding bits), found by a seeded search."""
    monkeypatch.delenv("IPX_JPEG_MAX_SCAN_BITS", raising=False)
    def flat(seed):                                           # the first seeded colour from `seed` on whose scan holds no 0xff
        return next(f for f in (frame("flat", 16, 16, s) for s in range(seed, seed + 100)) if b"\xff\x00" not in oracle.jpeg_encode_rgba(f, 100))
    frames = [flat(100), frame("noise", 256, 256, 2), flat(200), flat(300)]
    cand = [frame("noise", 16, 16, 5000 + s) for s in range(300)]
    f = Frames(ctx, frames + cand, ["stride16"] * (4 + len(cand)))
    try:
        whole = next((4 + s for s in range(len(cand)) if _scan_bits(ctx, monkeypatch, f.recs[4 + s]) % 8 == 0), None)
        print("a scan that ends on a byte boundary: candidate", whole)
        order = [0, 1, 2] + ([whole, 3] if whole is not None else [3])
        got = f.check(order, 100, oracle_every=1)
        assert got[1].count(b"\xff\x00") > 100 and len(got[1]) > 64 * 256 * 2
        for k in (0, 2):
            assert b"\xff\x00" not in got[k] and len(got[k]) - got[k].index(b"\xff\xda") - 14 - 2 <= 64
        f.check(order[::-1], 100)
    finally:
        f.free()


def test_counts(ctx):
    """n = 1; and 300 tiny frames of seven sizes, the same 21 device frames at many places: the search runs over more than 256 frames"""
    sizes = [(1, 1), (7, 9), (16, 16), (17, 17), (33, 15), (48, 8), (8, 40)]
    frames = [frame(KINDS[(s + k) % 3], w, h, 900 + 10 * s + k) for s, (w, h) in enumerate(sizes) for k in range(3)]
    f = Frames(ctx, frames, [LAYOUTS[(j // 3 + j) % 3] for j in range(21)])
    try:
        for i in (0, 5, 20):
            f.check([i], 85, oracle_every=1)
        rng = random.Random(7)
        f.check([rng.randrange(21) for _ in range(300)], 85, oracle_every=50)
        views, release = ctx.jpeg_encode_mixed_dev(f.recs[:4], 85, copy=False)
        assert [bytes(v) for v in views] == [f.alone(i, 85) for i in range(4)]
        release()
    finally:
        f.free()


def _raw(ctx, recs, n=None, quality=85):
    """the entry itself -> (status, blob pointer afterwards)"""
    import imageprocessor_amd as m
    n = len(recs) if n is None else n
    arr = (m._lib.RgbaFrame * max(len(recs), 1))()
    for i, (ptr, w, h, stride) in enumerate(recs):
        arr[i] = m._lib.RgbaFrame(ptr, w, h, stride)
    blob, offs, lens = C.c_void_p(1), (C.c_size_t * max(n, 1))(), (C.c_size_t * max(n, 1))()
    return m.lib().ipx_jpeg_encode_mixed_dev(ctx.handle, arr if recs else None, n, quality, C.byref(blob), offs, lens), blob.value


def test_refusals(ctx, edges, monkeypatch):
    """each a call of its own that leaves *blob NULL; a good frame before and behind the bad one"""
    import imageprocessor_amd as ipx
    import imageprocessor_amd as m
    monkeypatch.delenv("IPX_JPEG_MAX_SCAN_BITS", raising=False)
    good, other = edges.recs[4], edges.recs[10]
    ptr, w, h, stride = good
    assert ctx.jpeg_encode_mixed_dev([]) == []
    assert _raw(ctx, []) == (0, None)
    for bad in ((0, w, h, stride), (ptr, 0, h, stride), (ptr, w, 0, stride), (ptr, -1, h, stride), (ptr, w, h, 4 * w - 4), (ptr, 65536, 1, 4 * 65536),
                (ptr, 1, 65536, 4)):
        assert _raw(ctx, [good, bad, other]) == (INVALID, None), bad
    # 65535 x 65535 is a valid size beyond the span the kernels address (ipx_frame_supported); it needs no memory behind it
    assert m.lib().ipx_frame_supported(65535, 65535, 4 * 65535, 4) == UNSUPPORTED
    assert _raw(ctx, [good, (ptr, 65535, 65535, 4 * 65535)]) == (UNSUPPORTED, None)
    # a malformed frame behind it decides: IPX_ERR_INVALID first
    assert _raw(ctx, [(ptr, 65535, 65535, 4 * 65535), (ptr, 0, 1, 4)]) == (INVALID, None)
    arr = (m._lib.RgbaFrame * 65536)()
    blob, offs, lens = C.c_void_p(1), (C.c_size_t * 65536)(), (C.c_size_t * 65536)()
    assert m.lib().ipx_jpeg_encode_mixed_dev(ctx.handle, arr, 65536, 85, C.byref(blob), offs, lens) == UNSUPPORTED and not blob.value
    assert m.lib().ipx_jpeg_encode_mixed_dev(ctx.handle, arr, 1, 85, None, offs, lens) == INVALID
    assert m.lib().ipx_jpeg_encode_mixed_dev(ctx.handle, None, 1, 85, C.byref(blob), offs, lens) == INVALID
    assert m.lib().ipx_jpeg_encode_mixed_dev(ctx.handle, arr, -1, 85, C.byref(blob), offs, lens) == INVALID
    # a scan beyond the limit refuses the call and names the frame; the same call without the knob, and after it, is whole
    noisy = 7 * 3 + 2                                          # 176 x 64, noise
    assert edges.recs[noisy][1:3] == (176, 64) and KINDS[(7 + 2) % 3] == "noise"
    flat = [i for i in range(len(edges.recs)) if edges.recs[i][1:3] == (16, 16)]   # far shorter scans, whatever they hold
    bits = _scan_bits(ctx, monkeypatch, edges.recs[noisy])
    monkeypatch.setenv("IPX_JPEG_MAX_SCAN_BITS", str(bits))
    with pytest.raises(ipx.IpxError) as e:
        ctx.jpeg_encode_mixed_dev([edges.recs[i] for i in flat + [noisy] + flat], 100)
    assert e.value.status == UNSUPPORTED and "jpeg: scan too long for the GPU entropy coder" in e.value.text
    assert "%d bits in frame %d," % (bits, len(flat)) in e.value.text
    assert _raw(ctx, [edges.recs[noisy]], quality=100) == (UNSUPPORTED, None)
    monkeypatch.setenv("IPX_JPEG_MAX_SCAN_BITS", str(bits + 1))
    edges.check(flat + [noisy] + flat, 100)
    monkeypatch.delenv("IPX_JPEG_MAX_SCAN_BITS")
    edges.check(flat + [noisy] + flat, 100)


def test_the_switches_do_not_apply(ctx, edges, monkeypatch):
    """IPX_JPEG_FUSED_LEN=0 and IPX_JPEG_HOST_ENTROPY=1 move the uniform entry to other code, not this one: the same bytes"""
    idx = list(range(0, len(edges.recs), 3))
    want = edges.check(idx, 85)
    for env in ({"IPX_JPEG_FUSED_LEN": "0"}, {"IPX_JPEG_HOST_ENTROPY": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert ctx.jpeg_encode_mixed_dev([edges.recs[i] for i in idx], 85) == want
        for k in env:
            monkeypatch.delenv(k)


# ---- the leg: every chunk with outputs of several sizes is one mixed encode --------------------------------------------------------

OUTS = ("resize", "thumbnail", "watermark")
QUALITY = 85
LEG_ENVS = ("IPX_JPEG_MIXED_GROUP", "IPX_JPEG_MIXED_CHUNK_MB", "IPX_JPEG_JPEG_CHUNK", "IPX_JPEG_JPEG_PART")
# a keep_aspect resize into 160 x 120, an uncropped thumbnail and the watermarked frame: no output has one size for all files
RESIZE, THUMB = (160, 120, True), (32, False)
LEG_FILES = [((33, 15), "420"), ((200, 120), "444"), ((64, 48), "gray"), ((129, 65), "420"), ((17, 17), "444"), ((200, 120), "444"), ((33, 15), "420"),
             ((64, 48), "420"), ((129, 65), "gray")]


def _uniform_leg(ctx, files, sizes, glyphset=None, texts=None):
    """ipx_plan_run_jpeg_jpeg (or its _texts twin) per size and class with a plan of that size -> ({operator: [bytes | None]}, statuses)"""
    n = len(files)
    want, status = {k: [None] * n for k in OUTS}, [None] * n
    for key in sorted(set(sizes)):
        idx = [i for i in range(n) if sizes[i] == key]
        plan = ctx.plan(key[0][0], key[0][1], resize=RESIZE, thumbnail=THUMB, watermark=glyphset if glyphset is not None else True)
        try:
            out, st = plan.run_jpeg_jpeg([files[i] for i in idx], quality=QUALITY, texts=None if texts is None else [texts[i] for i in idx])
        finally:
            plan.close()
        for j, i in enumerate(idx):
            status[i] = st[j]
            for k in OUTS:
                want[k][i] = out.get(k, [None] * len(idx))[j]
    return want, status


@pytest.fixture(scope="module")
def leg_case(ctx):
    """nine files of five sizes and three sampling classes, and what the uniform leg makes of each with a plan of its size: once with
    the shared glyph list, once with a text per file"""
    import imageprocessor_amd as ipx
    from helpers import DEFAULT_COL
    from test_jpeg_mixed_gpu import leg_glyphs, leg_text, make
    files = [make(w, h, cls, seed=1200 + i) for i, ((w, h), cls) in enumerate(LEG_FILES)]
    gs = ctx.glyphset(leg_glyphs(), DEFAULT_COL)
    try:
        shared = _uniform_leg(ctx, files, LEG_FILES, glyphset=gs)
    finally:
        gs.close()
    texts = [leg_text(ipx, i, *LEG_FILES[i][0]) for i in range(len(files))]
    texted = _uniform_leg(ctx, files, LEG_FILES, texts=texts)
    assert shared[1] == texted[1] == [0] * len(files)
    assert len({(len(s), s[:200]) for s in shared[0]["resize"]}) > 1
    return files, shared[0], texts, texted[0]


def _ops(watermark):
    return {"resize": RESIZE, "thumbnail": THUMB, "watermark": watermark}


@pytest.mark.parametrize("env", [{}, {"IPX_JPEG_MIXED_CHUNK_MB": "0"}, {"IPX_JPEG_MIXED_GROUP": "2"}, {"IPX_JPEG_MIXED_CHUNK_MB": "1"}],
                         ids=["one-chunk", "chunk-per-file", "chunks-of-one-and-two", "chunks-of-one-mib"])
def test_leg_streams_are_the_uniform_legs(ctx, leg_case, monkeypatch, env):
    """Every output of a file differs in size from its neighbours', so a chunk of several sizes is one mixed-size jpeg.Encode.  With
    chunks of 0 MiB every file is a chunk of its own (one size: the uniform encode).  Decode groups of two files -- in the leg's order
    (17 x 17, 33 x 15), (33 x 15, 64 x 48), (64 x 48, 129 x 65), (129 x 65, 200 x 120), (200 x 120) -- are chunks of two files of two
    sizes and one chunk of one.  Chunks of 1 MiB (a file costs 150 to 419 KiB of frames and encoder scratch) hold five files of three
    sizes, three of two, and one."""
    from helpers import DEFAULT_COL
    from test_jpeg_mixed_gpu import leg_glyphs
    files, want, _, _ = leg_case
    for k in LEG_ENVS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, st = ctx.run_jpeg_jpeg_mixed(_ops((leg_glyphs(), DEFAULT_COL)), files, quality=QUALITY)
    assert st == [0] * len(files)
    for k in OUTS:
        for i in range(len(files)):
            assert got[k][i] is not None and got[k][i] == want[k][i], (k, i, LEG_FILES[i])


def test_leg_texts_per_file(ctx, leg_case, monkeypatch):
    files, want, texts, texted = leg_case
    for k in LEG_ENVS:
        monkeypatch.delenv(k, raising=False)
    got, st = ctx.run_jpeg_jpeg_mixed(_ops(True), files, quality=QUALITY, texts=texts)
    assert st == [0] * len(files) and got == texted and texted["watermark"] != want["watermark"]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_leg_with_an_undecodable_file(ctx, leg_case, monkeypatch, where):
    """a file the parser refuses, and one the decoder gives up on only in its scan (it has a plan and a place in its chunk): their
    outputs are {NULL, 0} and every other stream is what it is without them"""
    from helpers import DEFAULT_COL
    from test_jpeg_mixed_gpu import bad_code_file, leg_glyphs
    files, want, _, _ = leg_case
    for k in LEG_ENVS:
        monkeypatch.delenv(k, raising=False)
    at = {"first": 0, "middle": 4, "last": len(files)}[where]
    for bad in (b"\xff\xd8 not a jpeg", bad_code_file()):
        batch = files[:at] + [bad] + files[at:]
        got, st = ctx.run_jpeg_jpeg_mixed(_ops((leg_glyphs(), DEFAULT_COL)), batch, quality=QUALITY)
        assert st[at] == INVALID and st[:at] + st[at + 1:] == [0] * len(files)
        for k in OUTS:
            assert got[k][at] is None and got[k][:at] + got[k][at + 1:] == want[k], k
