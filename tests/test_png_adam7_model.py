"""The Adam7 model (tests/png_adam7_model.py) and writer (tests/png_adam7_corpus.py) on the CPU: the model against the hand-derived
known answers of tests/golden/png_adam7_kats.json, against Pillow's decode of the writer's files, and against
png_decode_model.decode of the non-interlaced twin of every row of the type table; the writer's raw length against the formula.  The GPU
decoder is held to this model in test_png_adam7_gpu.py."""
import io
import json
import os
import zlib

import numpy as np
import pytest

import png_adam7_corpus as ac
import png_adam7_model as am
import png_corpus as pc
import png_decode_model as dm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "png_adam7_kats.json")) as f:
    KATS = json.load(f)


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(k):
    data = bytes.fromhex(k["data"])
    r = am.decode(data)
    assert r["status"] == k["status"], r["why"]
    off = am.decode(data, adam7=False)
    assert off["status"] == k["status_off"] and off["stage"] == "container" and off["pix"] is None
    assert dm.decode(data)["status"] == k["status_off"]
    if k["status"] != dm.OK:
        assert r["pix"] is None
        return
    assert (r["kind"], r["w"], r["h"]) == (k["kind"], k["w"], k["h"])
    assert r["pix"].tobytes().hex() == k["pix"]
    if "palette" in k:
        assert r["palette"].tobytes().hex() == k["palette"]


def test_known_answers_cover_the_rules():
    names = " ".join(k["name"] for k in KATS)
    for word in ("pass order", "1x1", "3x2", "2x5", "gray1 packed", "pal2 packed", "Up row", "Paeth row", "one byte short", "one byte long",
                 "first row of pass 3", "last row of pass 7", "after the Adler-32", "palette without PLTE", "sub-byte gray", "IHDR CRC"):
        assert word in names, word
    assert {k["status"] for k in KATS} == {dm.OK, dm.INVALID, dm.UNSUPPORTED}
    assert {k["status_off"] for k in KATS} == {dm.UNSUPPORTED}


# (ctype, depth, Pillow's mode) of the kinds Pillow decodes to the samples themselves
PIL_TYPES = [(0, 1, "1"), (0, 2, "L"), (0, 4, "L"), (0, 8, "L"), (4, 8, "LA"), (2, 8, "RGB"), (6, 8, "RGBA"), (3, 1, "P"), (3, 2, "P"),
             (3, 4, "P"), (3, 8, "P")]
SIZES = list(range(1, 10)) + [17, 33]
HEIGHTS = list(range(1, 10)) + [65, 130]


@pytest.mark.parametrize("ctype,depth,mode", PIL_TYPES, ids=["%d-%d" % t[:2] for t in PIL_TYPES])
def test_writer_and_model_against_pillow(ctype, depth, mode):
    """the seeded corpus, 11 x 11 sizes per type: Pillow reads the writer's files back to the source samples, the raw length is the
    formula's, and the model's pixels are the samples converted as a non-interlaced file's are"""
    from PIL import Image
    maxv = (1 << depth) - 1
    for k, (h, w) in enumerate((h, w) for h in HEIGHTS for w in SIZES):
        s = pc.samples_of_type(ctype, depth, h, w, seed=k)
        plte = [(3 * i % 256, 5 * i % 256, 7 * i % 256) for i in range(maxv + 1)] if ctype == 3 else None
        data = ac.write(s, ctype, depth, plte=plte, filters=((0, 1, 2, 3, 4), (k % 5,))[k % 2], split=(None, 7)[k % 2])
        st, f = dm.parse(data[:28] + b"\x00" + data[29:])
        raw = zlib.decompress(b"".join(f["idat"]))
        assert len(raw) == ac.raw_length(ctype, depth, w, h) == _formula(ctype, depth, w, h)
        im = Image.open(io.BytesIO(data))
        assert im.info.get("interlace") == 1
        got = np.asarray(im).astype(np.int64)
        if ctype == 0 and depth < 8:
            got = got * 1 if depth == 1 else got // (255 // maxv)      # Pillow scales 2- and 4-bit gray to 8 bits; "1" gives booleans
        np.testing.assert_array_equal(got.reshape(h, w, -1), s, err_msg="%dx%d" % (w, h))
        r = am.decode(data, fast=h > 9)
        assert r["status"] == dm.OK, r["why"]
        want = dm.convert(pc.pack_rows(s, ctype, depth), ctype, depth, w, h, None)
        np.testing.assert_array_equal(r["pix"], want, err_msg="%dx%d" % (w, h))


def _formula(ctype, depth, w, h):
    """the raw length as DESIGN.md section 4.10 states it"""
    bits = dm.CHANNELS[ctype] * depth
    n = 0
    for xf, yf, xo, yo in [(8, 8, 0, 0), (8, 8, 4, 0), (4, 8, 0, 4), (4, 4, 2, 0), (2, 4, 0, 2), (2, 2, 1, 0), (1, 2, 0, 1)]:
        pw, ph = (w - xo + xf - 1) // xf, (h - yo + yf - 1) // yf
        if pw > 0 and ph > 0:
            n += ph * (1 + (bits * pw + 7) // 8)
    return n


def test_raw_length_of_small_frames():
    assert _formula(0, 8, 1, 1) == 2
    assert _formula(0, 8, 8, 8) == 79
    assert _formula(0, 8, 3, 2) == 10 and _formula(0, 8, 2, 5) == 18
    assert _formula(0, 1, 5, 5) == 22 and _formula(3, 2, 5, 5) == 24


@pytest.mark.parametrize("name,ctype,depth,trns", pc.TYPES, ids=[t[0] for t in pc.TYPES])
def test_equals_the_non_interlaced_twin(name, ctype, depth, trns):
    """every row of the type table (16-bit and tRNS rows included): the interlaced file's pix and palette are those png_decode_model
    gives the non-interlaced file of the same samples"""
    for k, (w, h) in enumerate([(1, 1), (1, 9), (9, 1), (13, 7), (37, 29), (70, 67)]):
        kw = dict(seed=100 * k + 3, kind=("photo", "flat")[k % 2], filters=((0, 1, 2, 3, 4), (k % 5,))[k % 2])
        il = ac.of_type(ctype, depth, trns, h, w, **kw)
        twin = ac.of_type(ctype, depth, trns, h, w, interlace=False, **kw)
        assert twin == pc.of_type(ctype, depth, trns, h, w, **kw)
        a, b = am.decode(il, fast=k >= 4), dm.decode(twin, fast=k >= 4)
        assert a["status"] == b["status"] == dm.OK, (a["why"], b["why"])
        assert (a["kind"], a["w"], a["h"]) == (b["kind"], b["w"], b["h"])
        np.testing.assert_array_equal(a["pix"], b["pix"])
        if b["palette"] is None:
            assert a["palette"] is None
        else:
            np.testing.assert_array_equal(a["palette"], b["palette"])
        assert am.decode(il, adam7=False)["status"] == dm.UNSUPPORTED


def test_non_interlaced_files_get_the_plain_models_answer():
    with open(os.path.join(HERE, "golden", "png_dec_kats.json")) as f:
        plain = json.load(f)
    for k in plain:
        data = bytes.fromhex(k["data"])
        for adam7 in (True, False):
            a, b = am.decode(data, adam7=adam7), dm.decode(data)
            if k["name"] == "Adam7" and adam7:
                assert b["status"] == dm.UNSUPPORTED and a["status"] == dm.INVALID     # the one interlaced file there: 5 x 1 with the
                continue                                                                # 6 bytes of a plain row, and its passes take 9
            assert a["status"] == b["status"] == k["status"] and a["stage"] == b["stage"] and a["why"] == b["why"], k["name"]
            assert (a["pix"] is None) == (b["pix"] is None)
            if a["pix"] is not None:
                np.testing.assert_array_equal(a["pix"], b["pix"])
