"""GPU: jpeg.Encode's five kernels (csrc/ipx_jpeg.hip, csrc/ipx_jpeg_entropy.hip, jpeg_encode_sets of csrc/ipx_jpeg_runtime.hip) against
the float64 reference of tests/jpeg_encode_reference.py and, byte for byte, against oracle/ipx_jpeg_oracle.c, over the corpus of
tests/jpeg_encode_corpus.py: the widths around the 8-MCU workgroup edge, 4K / 8K / 65535-long frames, strided and misaligned sources,
batches of a thousand frames, and the stream lengths on which the stuffing kernel's chunks, pieces and shifts turn.

Two conditions per coefficient, as in test_scaler_reference_gpu.py: it lies in the reference's admissible set, and it equals the oracle
(where the real value is next to a rounding boundary, libjpeg's fixed-point transform decides, and the oracle restates it).  The last
test is the refusal of a scan too long for the 32-bit offsets of the entropy coder; no frame larger than the corpus' own is encoded."""
import io

import numpy as np
import pytest

import jpeg_decode_model as jdm
import jpeg_encode_corpus as C
import jpeg_encode_reference as R
import oracle

pytestmark = pytest.mark.gpu

# IPX_JPEG_HOST_ENTROPY, IPX_JPEG_FUSED_LEN: the pairs of test_jpeg.py::test_gpu_batch_entropy_paths
ENTROPY_PATHS = [("0", "1"), ("0", "0"), ("1", "1")]
ENTROPY_IDS = ["gpu-entropy", "gpu-entropy-separate-sizing-pass", "host-entropy"]


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


def _entropy(monkeypatch, path):
    monkeypatch.setenv("IPX_JPEG_HOST_ENTROPY", path[0])
    monkeypatch.setenv("IPX_JPEG_FUSED_LEN", path[1])
    monkeypatch.delenv("IPX_JPEG_MAX_SCAN_BITS", raising=False)


class Dev:
    """frames (n x H x W x 4) in HBM, tightly packed or laid out as one of corpus.LAYOUTS"""

    def __init__(self, ctx, frames, layout=None):
        import imageprocessor_amd as ipx
        self.ctx = ctx
        self.n, self.h, self.w = frames.shape[:3]
        if layout is None:
            buf, off, self.stride, self.fs = np.ascontiguousarray(frames), 0, 4 * self.w, 4 * self.w * self.h
        else:
            buf, off, self.stride, self.fs = C.lay_out(frames, *layout)
        self.buf = ctx.alloc(buf.nbytes).upload(buf)
        assert self.buf.ptr % 256 == 0                    # the offsets of the layouts are offsets from an aligned allocation
        self.ptr = self.buf.ptr + off
        self.count = ipx.lib().ipx_jpeg_coef_count(self.w, self.h)

    def coefs(self, quality):
        out = self.ctx.alloc(self.n * self.count * 2)
        self.ctx.jpeg_fdct_dev(self.ptr, self.w, self.h, self.n, out.ptr, quality, stride=self.stride, frame_stride=self.fs)
        self.ctx.sync()
        got = out.download((self.n, self.count // 384, 6, 64), np.int16)
        out.free()
        return got

    def streams(self, quality):
        return self.ctx.jpeg_encode_batch_dev(self.ptr, self.w, self.h, self.n, quality, stride=self.stride, frame_stride=self.fs)

    def free(self):
        self.buf.free()


def _one(ctx, f):
    return Dev(ctx, f[None])


# ---- coefficients against the reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("quality", C.QUALITIES)
def test_coefficients_against_the_reference(ctx, quality):
    """Context.jpeg_fdct_dev over the corpus.  The quantiser of the reference is the one the product's own stream carries in DQT."""
    for recipe in C.reference_cases():
        kind, w, h, seed, q = recipe
        if q != quality:
            continue
        f = C.frame(kind, w, h, seed)
        d = _one(ctx, f)
        got = d.coefs(q)[0]
        dqt = R.dqt_tables(d.streams(q)[0])
        d.free()
        R.assert_matches(got, R.reference(f, dqt), R.cap(q), what="%r" % (recipe,))
        want = oracle.jpeg_encode_rgba(f, q, want_coefs=True)[1]
        np.testing.assert_array_equal(got, want, err_msg="%r: the kernel differs from the oracle" % (recipe,))


# ---- finished streams, read back by the decoder model ----------------------------------------------------------------------------

def _sof0(stream):
    b = bytes(stream)
    i = 2
    while b[i + 1] != 0xC0:
        i += 2 + (b[i + 2] << 8 | b[i + 3])
    return b[i + 4:i + 2 + (b[i + 2] << 8 | b[i + 3])]


@pytest.mark.parametrize("path", ENTROPY_PATHS, ids=ENTROPY_IDS)
def test_streams_decode_to_the_reference(ctx, path, monkeypatch):
    """jpeg_encode_batch_dev under each entropy path: every stream of the geometry grid (each at one quality of 85 / 50 / 20 / 100, all
    at or below 64 k pixels) is read by tests/jpeg_decode_model.py; its coefficients lie in the reference's sets and equal the
    oracle's; SOF0 carries the size and the 2x2 / 1x1 / 1x1 sampling; Pillow opens it at the right size."""
    from PIL import Image
    _entropy(monkeypatch, path)
    for i, (kind, w, h, seed) in enumerate(C.GEOMETRIES):
        assert w * h <= 65536
        q = C.QUALITIES[i % len(C.QUALITIES)]
        f = C.frame(kind, w, h, seed)
        d = _one(ctx, f)
        stream = d.streams(q)[0]
        d.free()
        what = "%r quality %d" % ((kind, w, h, seed), q)
        assert _sof0(stream) == bytes([8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]), what
        dec = jdm.decode(stream, want_coefs=True)
        assert (dec["w"], dec["h"], dec["ratio"]) == (w, h, 2), what
        got = R.scan_order_of(dec["coefs"])
        R.assert_matches(got, R.reference(f, R.dqt_tables(stream)), R.cap(q), what=what)
        np.testing.assert_array_equal(got, oracle.jpeg_encode_rgba(f, q, want_coefs=True)[1], err_msg=what)
        assert Image.open(io.BytesIO(stream)).size == (w, h), what


# ---- exact colour ------------------------------------------------------------------------------------------------------------

def test_colour_lattice_is_exact(ctx):
    """One frame of flat 16x16 MCUs, one per colour of the lattice r, g, b in {0, 1, 2, 5, 10, ..., 250, 253, 254, 255} (56 values a
    channel, 175 616 MCUs, 7168 x 6272 pixels).  At quality 100 every quantiser is 1 and the DC path of the transform is exact: each
    block's DC is 8 (v - 128) for the integer Y, Cb, Cr of jpeg_encode_reference.ycbcr, every AC coefficient is 0.  No tolerance."""
    vals = np.array([0, 1, 2] + list(range(5, 251, 5)) + [253, 254, 255])
    assert len(vals) == 56
    r, g, b = (v.ravel() for v in np.meshgrid(vals, vals, vals, indexing="ij"))
    mh, mw = 392, 448
    assert mh * mw == r.size
    mcus = np.stack([r, g, b, np.full_like(r, 255)], -1).astype(np.uint8).reshape(mh, mw, 4)
    f = np.repeat(np.repeat(mcus, 16, 0), 16, 1)
    d = _one(ctx, f)
    del f
    got = d.coefs(100)[0]
    d.free()
    y, cb, cr = R.ycbcr(r, g, b)
    assert not got[:, :, 1:].any(), "an AC coefficient of a flat block is not 0"
    for j, v in enumerate((y, y, y, y, cb, cr)):
        bad = np.nonzero(got[:, j, 0] != 8 * (v - 128))[0]
        assert bad.size == 0, "block %d of colour %r: DC %d, expected %d" % (j, (r[bad[0]], g[bad[0]], b[bad[0]]), got[bad[0], j, 0],
                                                                              8 * (v[bad[0]] - 128))


# ---- byte-exact against the oracle -----------------------------------------------------------------------------------------------

def test_every_geometry_is_byte_exact(ctx, monkeypatch):
    _entropy(monkeypatch, ENTROPY_PATHS[0])
    for i, (kind, w, h, seed) in enumerate(C.GEOMETRIES):
        f = C.frame(kind, w, h, seed)
        d = _one(ctx, f)
        for q in (85, (30, 100, 5, 60)[i % 4]):
            assert d.streams(q)[0] == oracle.jpeg_encode_rgba(f, q), ((kind, w, h, seed), q)
        if kind == "translucent":                          # alpha must not matter
            opaque = f.copy()
            opaque[..., 3] = 255
            assert d.streams(85)[0] == oracle.jpeg_encode_rgba(opaque, 85), (kind, w, h, seed)
        d.free()


@pytest.mark.parametrize("recipe", C.LARGE + C.LONG, ids=lambda r: "%s-%dx%d" % r[:3])
def test_large_and_long_frames_are_byte_exact(ctx, recipe, monkeypatch):
    """3840 x 2160 and 7680 x 4320 (the watermark output of a 4K / 8K source is encoded at source size) and the longest sides the
    entries accept, at quality 85: streams and coefficients"""
    _entropy(monkeypatch, ENTROPY_PATHS[0])
    kind, w, h, seed = recipe
    f = C.frame(kind, w, h, seed)
    want, coefs = oracle.jpeg_encode_rgba(f, 85, want_coefs=True)
    d = _one(ctx, f)
    got = d.streams(85)[0]
    assert len(got) == len(want) and got == want, recipe
    np.testing.assert_array_equal(d.coefs(85)[0], coefs, err_msg=repr(recipe))
    d.free()


@pytest.mark.parametrize("path", ENTROPY_PATHS, ids=ENTROPY_IDS)
def test_stream_length_edges_are_byte_exact(ctx, path, monkeypatch):
    """unstuffed scans of k 64 - 1 / k 64 / k 64 + 1 and 16384 - 1 / 16384 / 16384 + 1 bytes, a 0xff as the last byte of a chunk, of a
    16 KiB piece and of the scan, and the long stream whose pieces show all 16 shifts (test_jpeg_reference.py proves the properties);
    alone, and all frames of one size as one batch, so that the neighbours' streams bound each one's"""
    _entropy(monkeypatch, path)
    recipes = [r for _, r in C.STREAM_RECIPES] + [C.PHASE_RECIPE]
    for kind, w, h, seed, q in recipes:
        f = C.frame(kind, w, h, seed)
        d = _one(ctx, f)
        assert d.streams(q)[0] == oracle.jpeg_encode_rgba(f, q), (kind, w, h, seed, q)
        d.free()
    same = [r for r in recipes if r[1:3] == (112, 64) and r[4] == 100]
    assert len(same) == 3
    frames = np.stack([C.frame(*r[:4]) for r in same] * 2)
    d = Dev(ctx, frames)
    got = d.streams(100)
    d.free()
    for k in range(len(frames)):
        assert got[k] == oracle.jpeg_encode_rgba(frames[k], 100), k


def test_every_quality_is_byte_exact(ctx, monkeypatch):
    """qualities 1 .. 100 on one 64 x 48 frame; 0, -3, 101 and 1000 are clamped to 1 and 100 as Go clamps them"""
    _entropy(monkeypatch, ENTROPY_PATHS[0])
    f = C.frame("photo", 64, 48, 9)
    d = _one(ctx, f)
    by_q = {}
    for q in range(1, 101):
        by_q[q] = d.streams(q)[0]
        assert by_q[q] == oracle.jpeg_encode_rgba(f, q), q
    for q, same_as in ((0, 1), (-3, 1), (101, 100), (1000, 100)):
        got = d.streams(q)[0]
        assert got == by_q[same_as] and got == oracle.jpeg_encode_rgba(f, q), q
        np.testing.assert_array_equal(d.coefs(q), d.coefs(same_as))
    assert by_q[1] != by_q[2] and by_q[99] != by_q[100]
    d.free()


@pytest.mark.parametrize("path", ENTROPY_PATHS, ids=ENTROPY_IDS)
def test_batches_are_byte_exact(ctx, path, monkeypatch):
    """a thousand 1 x 1 and a thousand 16 x 16 frames per call; flat frames between quality-100 binary noise (stream lengths of one
    batch three orders of magnitude apart)"""
    _entropy(monkeypatch, path)
    rng = np.random.default_rng(5)
    for (w, h), q in (((1, 1), 85), ((16, 16), 85)):
        frames = rng.integers(0, 256, (1000, h, w, 4), dtype=np.uint8)
        d = Dev(ctx, frames)
        got = d.streams(q)
        d.free()
        assert len(got) == 1000
        for k in range(1000):
            assert got[k] == oracle.jpeg_encode_rgba(frames[k], q), ((w, h), k)
    frames = np.stack([C.frame("flat" if k % 2 == 0 else "binary", 96, 80, k) for k in range(7)])
    d = Dev(ctx, frames)
    got = d.streams(100)
    d.free()
    for k in range(7):
        assert got[k] == oracle.jpeg_encode_rgba(frames[k], 100), k
    assert len(got[0]) * 20 < len(got[1])


def test_three_outputs_with_a_one_pixel_thumbnail(ctx, monkeypatch):
    """ipx_plan_run_host_jpeg: a 1 x 1 thumbnail beside a large resize and the source-size watermark copy, in one call of
    jpeg_encode_sets (three sets of very different block counts)"""
    _entropy(monkeypatch, ENTROPY_PATHS[0])
    w, h, n = 96, 64, 5
    frames = np.stack([C.frame(("photo", "noise", "edge", "smooth", "checker")[k], w, h, k) for k in range(n)])
    plan = ctx.plan(w, h, resize=(2048, 1536, False), thumbnail=(1, True), watermark=True)
    try:
        assert (plan.info.thumb_w, plan.info.thumb_h) == (1, 1)
        got = plan.run_host_jpeg(frames, 85)
    finally:
        plan.close()
    assert set(got) == {"resize", "thumbnail", "watermark"}
    for k in range(n):
        want = oracle.process(frames[k], resize=(2048, 1536, False), thumb=(1, True), glyphs=[])
        assert want["thumbnail"].shape == (1, 1, 4) and want["resize"].shape == (1536, 2048, 4)
        for key in got:
            assert got[key][k] == oracle.jpeg_encode_rgba(want[key], 85), (key, k)


# ---- the same pixels in other layouts: fast path against slow path ---------------------------------------------------------------

@pytest.mark.parametrize("shape", C.LAYOUT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_layouts_give_the_same_coefficients_and_bytes(ctx, shape, monkeypatch):
    """Strides of 4w+4, 4w+12 and 4w+16, frame strides that are no multiple of 16, source pointers 4, 8 and 12 bytes into an
    allocation: whole workgroups of the transform kernel then take the per-pixel loads instead of the aligned 16-byte ones (or, for
    4w+16 alone, the aligned ones over padded rows).  Equal coefficient buffers need no oracle; the streams equal the packed call's
    and the oracle's."""
    _entropy(monkeypatch, ENTROPY_PATHS[0])
    w, h, n = shape
    frames = np.stack([C.frame(("noise", "photo", "binary")[k % 3], w, h, 40 + k) for k in range(n)])
    packed = Dev(ctx, frames)
    assert (packed.ptr | packed.stride | packed.fs) % 16 == 0          # the packed call is the aligned one
    coefs = {q: packed.coefs(q) for q in (85, 100)}
    streams = packed.streams(85)
    packed.free()
    for k in range(n):
        assert streams[k] == oracle.jpeg_encode_rgba(frames[k], 85), k
    for name, es, ef, off in C.LAYOUTS:
        d = Dev(ctx, frames, (es, ef, off))
        for q in (85, 100):
            np.testing.assert_array_equal(d.coefs(q), coefs[q], err_msg="%s quality %d" % (name, q))
        assert d.streams(85) == streams, name
        d.free()


# ---- a scan too long for the 32-bit offsets ----------------------------------------------------------------------------------------

def test_too_long_a_scan_is_refused(ctx, monkeypatch):
    """The block offsets of the GPU entropy coder are 32-bit; jpeg_encode_sets carries each frame's total in 64 bits and refuses a
    batch with a frame at or beyond the limit (2^32 - 1 bits; IPX_JPEG_MAX_SCAN_BITS lowers it, here to 100 000) before anything uses
    the offsets: IPX_ERR_UNSUPPORTED and a clear message.  Flat frames under the same setting, and any call after the refusal, match
    the oracle; the three-output entry propagates the refusal; the host entropy path has no such limit."""
    import imageprocessor_amd as ipx
    _entropy(monkeypatch, ENTROPY_PATHS[0])
    w, h = 320, 200
    frames = np.stack([C.frame("flat", w, h, 1), C.frame("noise", w, h, 2), C.frame("flat", w, h, 3)])
    small = np.stack([C.frame("flat", 64, 64, k) for k in range(3)])
    want = [oracle.jpeg_encode_rgba(f, 100) for f in frames]
    assert len(C.scan_of(want[1])[2]) * 8 > 100000 > len(C.scan_of(want[0])[2]) * 8
    big, flat = Dev(ctx, frames), Dev(ctx, small)
    plan = ctx.plan(w, h, resize=(64, 40, False), thumbnail=(16, True), watermark=True)
    try:
        for fused in ("1", "0"):
            monkeypatch.setenv("IPX_JPEG_FUSED_LEN", fused)
            monkeypatch.setenv("IPX_JPEG_MAX_SCAN_BITS", "100000")
            with pytest.raises(ipx.IpxError) as e:
                big.streams(100)
            assert e.value.status == -4 and "jpeg: scan too long for the GPU entropy coder" in e.value.text
            got = flat.streams(100)                                    # flat frames alone, same setting
            for k in range(3):
                assert got[k] == oracle.jpeg_encode_rgba(small[k], 100), k
            with pytest.raises(ipx.IpxError) as e:                     # the three-output entry: the watermark copy is the noise frame
                plan.run_host_jpeg(frames, 100)
            assert e.value.status == -4 and "jpeg: scan too long for the GPU entropy coder" in e.value.text
            monkeypatch.setenv("IPX_JPEG_HOST_ENTROPY", "1")           # no such limit on the host
            assert big.streams(100) == want
            monkeypatch.setenv("IPX_JPEG_HOST_ENTROPY", "0")
            monkeypatch.setenv("IPX_JPEG_MAX_SCAN_BITS", "2000000000")  # a larger value than the limit cannot raise it: same bytes
            assert big.streams(100) == want
            monkeypatch.delenv("IPX_JPEG_MAX_SCAN_BITS")
            assert big.streams(100) == want                            # a normal call on the same context after the refusals
            got = plan.run_host_jpeg(frames, 100)
            for k in range(3):
                ops = oracle.process(frames[k], resize=(64, 40, False), thumb=(16, True), glyphs=[])
                for key in got:
                    assert got[key][k] == oracle.jpeg_encode_rgba(ops[key], 100), (key, k)
    finally:
        plan.close()
        big.free()
        flat.free()

