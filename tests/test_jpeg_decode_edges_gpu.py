"""image.Decode on the GPU on JPEG streams libjpeg never writes (tests/jpeg_edge_corpus.py): 16-bit quantisation tables with entries
that make idct.go's int32 arithmetic wrap, AC sizes 11..15 and DC sizes 12..16, 16-bit codes on common symbols, single-symbol, complete
and 256-symbol tables, ZRL runs to and past zig 63, restart intervals of 1, odd and longer than the image, tables after SOF, several
scans; 1 x 1 to 1920 x 1080.  Under every kernel-path switch, alone and mixed into batches of Pillow's files, and through
run_jpeg_jpeg.  The status contract:
  0  -> every plane equals tests/jpeg_decode_model.py's and the oracle's, byte for byte
  -1 <-> the model says malformed
  -4 -> the model says unsupported, or a DC value beyond int16 (the documented hand-back classes)"""
import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_edge_corpus as je
import oracle
from test_jpeg_decode import picture, pil_jpeg

pytestmark = pytest.mark.gpu

PATHS = [{}, {"IPX_JPEG_PIECE": "0"}, {"IPX_JPEG_PIECE": "0", "IPX_JPEG_SHARED_TABLES": "0"}, {"IPX_JPEG_PAR": "0"}]
PATH_IDS = ["default", "bytewise-shared-tables", "bytewise-per-lane-tables", "pieces"]


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context()
    yield c
    c.close()


_MODEL = {}


def model(data):
    """the model's verdict and planes, once per file"""
    if data not in _MODEL:
        try:
            _MODEL[data] = ("ok", dm.decode(data))
        except ValueError as e:
            _MODEL[data] = (str(e).split(":")[0], None)
    return _MODEL[data]


def check(ctx, files):
    """one batch (one shape): every file's status and planes against the model and the oracle"""
    info, st = ctx.jpeg_decode_batch(files)
    for i, f in enumerate(files):
        verdict, m = model(f)
        if verdict == "malformed":
            assert st[i] == -1, (i, st[i])
            continue
        if verdict == "unsupported" and b"\xff\xc2" not in f:
            assert st[i] == -4, (i, st[i])
            continue
        o = oracle.jpeg_decode(f)
        if o["dc_wide"]:
            assert st[i] == -4, (i, st[i])
            continue
        assert st[i] == 0, (i, st[i])
        for k in ("y", "cb", "cr") if o["ratio"] != 4 else ("y",):
            np.testing.assert_array_equal(info[k][i], o[k], err_msg="file %d plane %s vs oracle" % (i, k))
            if m is not None:
                np.testing.assert_array_equal(info[k][i], m[k], err_msg="file %d plane %s vs model" % (i, k))
    return st


def by_shape(cases):
    out = {}
    for c in cases:
        out.setdefault((c.w, c.h, c.ratio), []).append(c)
    return out


def twin(w, h, ratio, seed):
    """a Pillow file of the same shape (Gray, or YCbCr at the ratio's sampling; Pillow cannot write 4:4:0)"""
    img = picture(w, h, seed=seed)
    if ratio == 4:
        return pil_jpeg(img[..., 0], quality=85)
    return pil_jpeg(img, quality=85, subsampling={0: 0, 1: 1, 2: 2}[ratio])


@pytest.fixture(scope="module")
def corpus():
    return je.corpus()


@pytest.mark.parametrize("env", PATHS, ids=PATH_IDS)
def test_corpus_alone_and_beside_pillow_files(ctx, corpus, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for k, ((w, h, ratio), cases) in enumerate(by_shape(corpus).items()):
        files = [c.data for c in cases]
        check(ctx, files)
        if ratio != 3:
            t = twin(w, h, ratio, k)
            st = check(ctx, [t] + files + [t, t])
            assert st[0] == 0 and st[-1] == 0


def test_the_wrap_cases_fail_without_the_row_shortcut(ctx, corpus):
    """the files where idct.go's shortcut and full path part ways decode to the model's planes -- which differ from the planes
    without the shortcut, so a kernel without it cannot pass"""
    for c in corpus:
        if "idct_wrap" not in c.edges:
            continue
        info, st = ctx.jpeg_decode_batch([c.data])
        assert st == [0], c.name
        plain = dm.decode(c.data, shortcut=False)
        assert any(not np.array_equal(info[k][0], plain[k]) for k in ("y", "cb", "cr") if k in info), c.name


@pytest.fixture(scope="module")
def big():
    return [c for c in je.corpus(big=True) if c.name.startswith("big_1080p")]


@pytest.mark.parametrize("stage", ["0", "1"], ids=["scan-through-l2", "scan-rows-in-lds"])
@pytest.mark.parametrize("sub_bytes", ["128", "256", "512", "1024"])
def test_long_scans_through_the_parallel_decoder(ctx, big, monkeypatch, sub_bytes, stage):
    monkeypatch.setenv("IPX_JPEG_PAR_SUB", sub_bytes)
    monkeypatch.setenv("IPX_JPEG_PAR_STAGE", stage)
    pil = pil_jpeg(picture(1920, 1080, seed=3), subsampling=2, quality=85)
    assert check(ctx, [c.data for c in big] + [pil]) == [0] * (len(big) + 1)


def dqt_to_16bit(data, zig2=None):
    """every DQT segment of a file rewritten with 16-bit entries (the same values; zig 2 set to zig2 when given)"""
    out, i = bytearray(data[:2]), 2
    while i < len(data):
        if data[i] != 0xFF or data[i + 1] == 0xDA:
            return bytes(out + data[i:])
        n = data[i + 2] << 8 | data[i + 3]
        body = data[i + 4:i + 2 + n]
        if data[i + 1] == 0xDB:
            nb, k = b"", 0
            while k < len(body):
                assert body[k] >> 4 == 0
                q = list(body[k + 1:k + 65])
                if zig2 is not None:
                    q[2] = zig2
                nb += bytes([0x10 | body[k] & 15]) + b"".join(int(v).to_bytes(2, "big") for v in q)
                k += 65
            body = nb
        out += data[i:i + 2] + (len(body) + 2).to_bytes(2, "big") + body
        i += 2 + n
    return bytes(out)


def test_progressive_and_multi_scan_files_with_16bit_tables(ctx):
    """the host scan decoder's files share the IDCT kernel: a Pillow progressive file with 16-bit tables (zig 2 at 20000, so that rows
    wrap), its baseline twin, and the corpus's multi-scan files"""
    img = np.full((64, 96, 3), 200, np.uint8)
    img[(np.arange(64) % 8) < 4] = (40, 90, 160)                # horizontal stripes: large terms at natural index 8 (zig 2), none in its row
    prog = dqt_to_16bit(pil_jpeg(img, quality=100, progressive=True), 20000)
    base = dqt_to_16bit(pil_jpeg(img, quality=100), 20000)
    assert check(ctx, [prog, base, prog]) == [0, 0, 0]
    a, b = oracle.jpeg_decode(prog), oracle.jpeg_decode(base)
    assert np.array_equal(a["y"][:64, :96], b["y"][:64, :96])
    assert not np.array_equal(dm.decode(base)["y"], dm.decode(base, shortcut=False)["y"])


def test_compressed_in_compressed_out(ctx):
    """a few edge files through ipx_plan_run_jpeg_jpeg, held to the oracle's decoder + operators + encoder as
    test_jpeg_decode.py::test_compressed_in_compressed_out holds Pillow's"""
    from helpers import DEFAULT_COL, text_glyphs
    from test_sources_gpu import _expect_ycbcr_ops
    import jpeg_writer as jw
    w, h = 320, 200
    rng = np.random.default_rng(11)
    c3 = je.comps3(2, 2)
    fr = jw.Frame(w, h, c3)
    _, ac_s, dc17 = je.tables_short()
    dc_l, ac_l = je.tables_long()
    qw = np.full(64, 2)
    qw[2] = 20000
    files = []
    for k in range(4):
        bl = je._wrap_blocks(fr, rng) if k % 2 == 0 else je.limit(jw.all_blocks(fr, rng, amp=300, ac=900, density=0.1))
        tabs = {(0, 0): dc17, (1, 0): ac_s, (0, 1): dc17, (1, 1): ac_s} if k < 2 else {(0, 0): dc_l, (1, 0): ac_l, (0, 1): dc_l, (1, 1): ac_l}
        files.append(je.file(w, h, c3, bl, tabs, {0: (qw, 1), 1: (np.full(64, 3), 1)}, ri=[0, 1, 7, 1000][k], pad=k % 2))
    files.insert(2, pil_jpeg(picture(w, h, seed=2), quality=90))
    glyphs = text_glyphs(w, h, n=6, width_px=150, height_px=30)
    gs = ctx.glyphset(glyphs, DEFAULT_COL)
    plan = ctx.plan(w, h, resize=(512, 384, True), thumbnail=(100, True), watermark=gs)
    got, st = plan.run_jpeg_jpeg(files)
    assert st == [0] * len(files)
    for k, f in enumerate(files):
        d = oracle.jpeg_decode(f)
        if k != 2:
            m = dm.decode(f)
            assert all(np.array_equal(d[p], m[p]) for p in ("y", "cb", "cr"))
        ch, cw = (h + 1) // 2, (w + 1) // 2
        want = _expect_ycbcr_ops(np.ascontiguousarray(d["y"][:h, :w]), np.ascontiguousarray(d["cb"][:ch, :cw]), np.ascontiguousarray(d["cr"][:ch, :cw]),
                                 2, (512, 384, True), (100, True), glyphs, DEFAULT_COL)
        for key in ("resize", "thumbnail", "watermark"):
            assert got[key][k] == oracle.jpeg_encode_rgba(want[key], 85), (key, k)
    plan.close()
    gs.close()
