"""The scans of progressive JPEGs walked on the GPU (IPX_JPEG_PROG_GPU=1, csrc/ipx_jpeg_dec_scans.hip): one wave per file, scans in
file order.  Everything is byte-exact against oracle.jpeg_decode (Go's full decoder restated), never against the host route alone; and
ipx_jpeg_decode_counts shows which route ran -- the outputs are identical either way, so a silent fall-back to the host would pass
every comparison.  On the clean corpora the walk hands back no file (counts[3] stays); tests/test_jpeg_prog_writer.py shows the oracle
alone decodes every one of them."""
import numpy as np
import pytest

import jpeg_prog_writer as pw
import jpeg_writer as jw
import oracle
from test_jpeg_decode import picture, pil_jpeg

pytestmark = pytest.mark.gpu

PAR, HOST, GPU, ENDED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")


def decode(ctx, files):
    """-> (info, status, how far each count rose)"""
    before = ctx.jpeg_decode_counts()
    info, st = ctx.jpeg_decode_batch(files)
    return info, st, [a - b for a, b in zip(ctx.jpeg_decode_counts(), before)]


def same_planes(info, i, want, what=""):
    for k in ("y", "cb", "cr") if want["ratio"] != 4 else ("y",):
        np.testing.assert_array_equal(info[k][i], want[k], err_msg="%s file %d plane %s" % (what, i, k))


def pillow_batch(w, h, sub):
    return [pil_jpeg(picture(w, h, seed=60 + i + w), quality=(70, 85, 95, 40)[i], subsampling=sub, progressive=True, optimize=bool(i & 1)) for i in range(4)]


# ---- Pillow's files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("size", [(333, 211), (64, 48), (17, 9), (1, 1), (200, 8)])
def test_pillow_colour_files_are_walked_on_the_gpu(ctx, on, size, sub):
    files = pillow_batch(*size, sub)
    info, st, rose = decode(ctx, files)
    assert st == [0] * len(files)
    assert rose == [0, 0, len(files), 0], rose
    for i, f in enumerate(files):
        same_planes(info, i, oracle.jpeg_decode(f))


def test_pillow_grey_file(ctx, on):
    g = picture(120, 80, seed=4)[..., 0]
    files = [pil_jpeg(g, quality=85, progressive=True), pil_jpeg(g, quality=60, progressive=True, optimize=True)]
    info, st, rose = decode(ctx, files)
    assert st == [0, 0] and rose == [0, 0, 2, 0], (st, rose)
    for i, f in enumerate(files):
        same_planes(info, i, oracle.jpeg_decode(f))


def test_switch_unset_keeps_the_host_route(ctx, monkeypatch):
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False)
    files = pillow_batch(333, 211, 2)
    info, st, rose = decode(ctx, files)
    assert st == [0] * len(files) and rose == [0, len(files), 0, 0], (st, rose)
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    info2, st2, rose2 = decode(ctx, files)
    assert st2 == st and rose2 == [0, 0, len(files), 0], (st2, rose2)
    for i, f in enumerate(files):
        want = oracle.jpeg_decode(f)
        same_planes(info, i, want, "host")
        same_planes(info2, i, want, "gpu")


# ---- the writer's corpus: scripts libjpeg never writes -------------------------------------------------------------------------------
NAMES = [c[0] for c in pw.corpus()]


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_writer_corpus(ctx, on, k):
    name, frame, prog, base = pw.corpus()[k]
    info, st, rose = decode(ctx, [prog])
    assert st == [0] and rose == [0, 0, 1, 0], (st, rose)
    same_planes(info, 0, oracle.jpeg_decode(prog), name)


def test_writer_corpus_as_batches(ctx, on):
    """the files of one geometry side by side, each with its own scans and tables"""
    groups = {}
    for name, frame, prog, base in pw.corpus():
        groups.setdefault((frame.w, frame.h, tuple(frame.hv)), []).append(prog)
    for files in groups.values():
        info, st, rose = decode(ctx, files)
        assert st == [0] * len(files) and rose == [0, 0, len(files), 0], (st, rose)
        for i, f in enumerate(files):
            same_planes(info, i, oracle.jpeg_decode(f))


# ---- damaged files -------------------------------------------------------------------------------------------------------------------
def test_damaged_files_end_as_on_the_host_route(ctx, monkeypatch):
    """the 45 cases of test_damaged_progressive_files_never_disagree with the switch on: the status the same call returns with the switch
    off, the oracle's planes wherever both decode, and the call returns"""
    rng = np.random.default_rng(11)
    img = picture(333, 250, seed=8, noise=10.0)
    clean = [pil_jpeg(img, quality=85, progressive=True), pil_jpeg(img, quality=90, subsampling=0, optimize=True, progressive=True),
             pil_jpeg(img[..., 0], quality=80, progressive=True)]
    walked = ended = 0
    for t in range(45):
        f = bytearray(clean[t % 3])
        sos = f.index(b"\xff\xda")
        kind = (t // 3) % 5
        if kind == 0:
            for _ in range(3):
                f[int(rng.integers(sos + 14, len(f) - 2))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            f[int(rng.integers(sos + 14, len(f) - 2))] = int(rng.integers(0, 256))
        elif kind == 2:
            f[int(rng.integers(2, sos + 14))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 3:
            f = f[:int(rng.integers(sos, len(f)))]
        else:
            a = int(rng.integers(sos + 14, len(f) - 10))
            del f[a:a + int(rng.integers(1, 1500))]
        f = bytes(f)
        monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False)
        info_off, st_off = ctx.jpeg_decode_batch([f, clean[t % 3]])
        monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
        info, st, rose = decode(ctx, [f, clean[t % 3]])
        assert st == st_off, (t, kind, st, st_off)
        assert st[1] == 0
        walked += rose[GPU]
        ended += rose[ENDED]
        if st[0] == 0:
            want = oracle.jpeg_decode(f)
            if (want["w"], want["h"], want["ratio"]) == (info["w"], info["h"], info["ratio"]):
                same_planes(info, 0, want, "case %d" % t)
            for k in ("y", "cb", "cr") if info["ratio"] != 4 else ("y",):
                np.testing.assert_array_equal(info[k][0], info_off[k][0], err_msg="case %d plane %s against the host route" % (t, k))
    print("damaged files: %d walks, %d ended with a status" % (walked, ended))
    # the clean neighbour is walked every time; a changed byte inside a scan (nine cases) leaves the markers alone unless it makes or
    # breaks an 0xff, so damaged files reach the walk too
    assert walked > 45, (walked, ended)
    # cut or changed entropy data ends a walk with a status somewhere among 27 such cases (each error branch by hand: below)
    assert ended > 0, (walked, ended)


# ---- every way the walk ends a file, made by hand ------------------------------------------------------------------------------------
def _ended_cases():
    """(name, file, status): two grey blocks, a clean DC scan, then the scan that ends the file"""
    frame = pw.gray_frame(16, 8)
    blocks = jw.all_blocks(frame, np.random.default_rng(3), density=0.0)
    blocks[0][0, :, 2] = (5, -7)
    blocks[0][0, :, 9] = (3, 2)
    dc, first = ([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1)
    ones = [("bits", 0xFFFF, 16), ("bits", 0xFFFF, 16)]
    out = [
        ("reader runs dry", [dc, ([0], 1, 63, 0, 0, {"raw": [("sym", 0x01)]})], -1),                      # a 16-bit code, then no bit for the value
        ("bad Huffman code", [dc, ([0], 1, 63, 0, 0, {"raw": ones + [("sym", 0x00)]})], -1),              # sixteen ones match no code
        ("excessive DC component", [([0], 0, 0, 0, 0, {"raw": [("sym", 17)] + ones})], -4),
        ("unexpected Huffman code in a refinement", [dc, first, ([0], 1, 63, 1, 0, {"raw": [("sym", 0x02)] + ones})], -1),
        ("too many coefficients in a refinement", [dc, ([0], 1, 5, 0, 1), ([0], 1, 5, 1, 0, {"raw": [("sym", 0xF1)] + ones})], -1),
        ("reader runs dry in a DC refinement", [([0], 0, 0, 0, 1), ([0], 0, 0, 1, 0, {"raw": []})], -1),
    ]
    files = [(name, pw.progressive(frame, blocks, script), st) for name, script, st in out]
    # coefficients beyond int16: flagged, the walk goes on, UNSUPPORTED at the end; and one that int16 truncates to exactly zero, where
    # the host decoder is asked for the verdict (its non-zero mask and the stored block disagree from there on)
    wide = [b.copy() for b in blocks]
    wide[0][0, 0, 2] = 3 << 14
    files.append(("a coefficient beyond int16", pw.progressive(frame, wide, [dc, ([0], 1, 63, 0, 14)]), -4))
    zero = [b.copy() for b in blocks]
    zero[0][0, 0, 2] = 2 << 15
    files.append(("a coefficient that int16 truncates to zero", pw.progressive(frame, zero, [dc, ([0], 1, 63, 0, 15), ([0], 1, 63, 0, 0)]), -4))
    return files


ENDED_NAMES = [c[0] for c in _ended_cases()]


@pytest.mark.parametrize("k", range(len(ENDED_NAMES)), ids=ENDED_NAMES)
def test_the_walk_ends_a_file_as_the_host_route_does(ctx, monkeypatch, k):
    name, f, want = _ended_cases()[k]
    good = pw.progressive(pw.gray_frame(16, 8), jw.all_blocks(pw.gray_frame(16, 8), np.random.default_rng(4)), pw.libjpeg_script(pw.gray_frame(16, 8)))
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False)
    _, st_off = ctx.jpeg_decode_batch([f, good])
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    info, st, rose = decode(ctx, [f, good])
    assert st == st_off == [want, 0], (name, st, st_off)
    assert rose == [0, 0, 2, 1], rose                                    # walked, and ended by the walk
    same_planes(info, 1, oracle.jpeg_decode(good), name)
    if "int16" not in name:                                              # (Go keeps int32: the oracle decodes those)
        with pytest.raises(ValueError, match="malformed" if want == -1 else "unsupported"):
            oracle.jpeg_decode(f)


def test_more_table_definitions_than_a_16_bit_index_holds(ctx, on):
    """66 000 unused DHT definitions before the scans': the scans decode with the tables in effect, whatever came before"""
    frame = pw.colour_frame(48, 40)
    blocks = jw.all_blocks(frame, np.random.default_rng(2), amp=200, ac=40, density=0.2)
    files = [pw.progressive(frame, blocks, pw.libjpeg_script(frame), extra=pw.unused_tables(66000)),
             pw.progressive(frame, blocks, pw.libjpeg_script(frame), ids="same", extra=pw.unused_tables(9))]
    info, st, rose = decode(ctx, files)
    assert st == [0, 0] and rose == [0, 0, 2, 0], (st, rose)
    for i, f in enumerate(files):
        same_planes(info, i, oracle.jpeg_decode(f))


# ---- one batch of every route --------------------------------------------------------------------------------------------------------
def test_mixed_batch(ctx, on):
    w, h = 64, 48
    img = picture(w, h, seed=21)
    frame = pw.colour_frame(w, h)
    blocks = jw.all_blocks(frame, np.random.default_rng(5))
    dct = jw.Huff(jw.spread(16, 2, 9), list(range(16)))
    act = jw.Huff(jw.spread(256, 3, 12), sorted(range(256), key=lambda s: (s & 15, s >> 4)))
    seq = jw.soi() + jw.app0_jfif() + jw.dqt([(0, [2] * 64, 0), (1, [3] * 64, 0)]) + jw.sof(w, h, frame.comps) + jw.dht([(0, 0, dct), (1, 0, act)])
    for c in range(3):
        seq += jw.sos(frame.comps, [(c, 0, 0)]) + jw.scan(frame, [(c, 0, 0)], blocks, ({0: dct}, {0: act}))
    seq += jw.eoi()
    prog = pil_jpeg(img, quality=85, subsampling=0, progressive=True)
    files = [pil_jpeg(img, quality=85, subsampling=0),                                              # baseline
             prog,                                                                                  # walked on the GPU
             seq,                                                                                   # multi-scan sequential
             pil_jpeg(img, quality=85, subsampling=0, progressive=True, restart_marker_blocks=5),   # progressive with DRI
             prog[:len(prog) * 2 // 3],                                                             # its scans run out, no EOI
             pw.progressive(frame, blocks, pw.libjpeg_script(frame))]                               # walked on the GPU
    assert b"\xff\xdd" in files[3]
    info, st, rose = decode(ctx, files)
    assert st == [0, 0, 0, 0, -1, 0], st
    assert rose == [1, 3, 2, 0], rose                # the truncated file has no EOI: the pre-pass leaves it to the host
    for i in (0, 1, 2, 3, 5):
        same_planes(info, i, oracle.jpeg_decode(files[i]))
    with pytest.raises(ValueError, match="malformed"):
        oracle.jpeg_decode(files[4])


# ---- the worker's whole job ----------------------------------------------------------------------------------------------------------
def _job(w, h):
    from helpers import text_glyphs
    return text_glyphs(w, h, n=6, width_px=150, height_px=30), (512, 384, True), (100, True)


def _expected(files, w, h, glyphs, resize, thumb):
    from helpers import DEFAULT_COL
    from test_sources_gpu import _expect_ycbcr_ops
    out = []
    for f in files:
        d = oracle.jpeg_decode(f)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        want = _expect_ycbcr_ops(np.ascontiguousarray(d["y"][:h, :w]), np.ascontiguousarray(d["cb"][:ch, :cw]), np.ascontiguousarray(d["cr"][:ch, :cw]),
                                 2, resize, thumb, glyphs, DEFAULT_COL)
        out.append({k: oracle.jpeg_encode_rgba(v, 85) for k, v in want.items()})
    return out


def test_progressive_uploads_through_compressed_in_compressed_out(ctx, on):
    from helpers import DEFAULT_COL
    w, h = 320, 200
    files = [pil_jpeg(picture(w, h, seed=70 + i), quality=80 + i, progressive=bool(i % 3)) for i in range(8)]
    glyphs, resize, thumb = _job(w, h)
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=resize, thumbnail=thumb, watermark=gs)
    before = ctx.jpeg_decode_counts()
    got, st = plan.run_jpeg_jpeg(files)
    rose = [a - b for a, b in zip(ctx.jpeg_decode_counts(), before)]
    assert st == [0] * 8
    assert rose == [3, 0, 5, 0], rose
    for k, want in enumerate(_expected(files, w, h, glyphs, resize, thumb)):
        for key in got:
            assert got[key][k] == want[key], (key, k)
    plan.close()
    gs.close()


def test_progressive_uploads_through_a_pool_job(on):
    import imageprocessor_amd as ipx
    from helpers import DEFAULT_COL
    w, h = 320, 200
    files = [pil_jpeg(picture(w, h, seed=90 + i), quality=75 + 5 * i, progressive=True, optimize=bool(i & 1)) for i in range(3)]
    glyphs, resize, thumb = _job(w, h)
    pool = ipx.Pool(devices=(0,), lanes_per_device=2, lane_bytes=64 << 20)
    try:
        got, st = pool.submit_jpeg(files, w, h, 85, resize=resize, thumbnail=thumb, glyphs=glyphs, col=DEFAULT_COL).wait()
    finally:
        pool.close()
    assert st == [0, 0, 0]
    for k, want in enumerate(_expected(files, w, h, glyphs, resize, thumb)):
        for key in got:
            assert got[key][k] == want[key], (key, k)
