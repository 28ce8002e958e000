"""ipx_png_encode_mixed_dev and ipx_png_decode_mixed at their record, search and cut edges (tests/mixed_edge_cases.py builds the inputs,
tests/test_mixed_edge_cases.py proves on the CPU that they reach the edges).

Encode: more filter rows than one row of the filter launch's grid holds (2^20), so that gridDim.y > 1, the surplus workgroups and a
row0 beyond 2^20 are reached; a frame of 513 x 4096 pixels, beyond the opacity pass's 512 workgroups, beside 1 x 1 frames.  Streams
byte for byte against the uniform device entry (pinned to tests/png_model.py elsewhere), the model itself, and Pillow's decode.

Decode: the hand-written streams of tests/png_edge_corpus.py, tests/png_par_corpus.py (with its edge cases) and
tests/png_adam7_corpus.py, each at a frame offset and palette slot of its own between neighbours of other sizes."""
import io

import numpy as np
import pytest

import mixed_edge_cases as mx
import png_decode_model as dm
import png_model as pm
import png_par_model as ppm
from test_png_gpu import _frame
from test_png_mixed_gpu import _check_decode, _model, decode_case  # noqa: F401 (decode_case: the shipped call's files, a fixture)
from test_png_par_edges_gpu import file_of
from test_png_par_gpu import File

pytestmark = pytest.mark.gpu

SWITCHES = ("IPX_PNG_ADAM7", "IPX_PNG_PAR", "IPX_PNG_PAR_SUB", "IPX_PNG_DEC_SCRATCH_MB")


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


def setenv(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def upload(ctx, frames):
    """the frames in one device buffer, each at a 256-byte boundary with rows of w * 4 bytes -> (buffer, [(ptr, w, h, stride)])"""
    at, places = 0, []
    for f in frames:
        places.append(at)
        at = (at + f.nbytes + 255) // 256 * 256
    host = np.full(at + 256, 0xA5, np.uint8)
    for f, o in zip(frames, places):
        host[o:o + f.nbytes] = f.reshape(-1)
    d = ctx.alloc(host.nbytes).upload(host)
    return d, [(d.ptr + o, f.shape[1], f.shape[0], f.shape[1] * 4) for f, o in zip(frames, places)]


def pillow_rows(stream):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(stream)))


# ---- C. encode -------------------------------------------------------------------------------------------------------------------

def test_encode_rows_beyond_one_grid_row(ctx):
    """C1.  A 3 x 2 frame, then an opaque 1 x 65535 frame and its twin with one alpha byte 0xfe in the last row described 17 times in
    turn, then a 1 x 1 frame: 1 114 098 filter rows, 65 522 of them in the launch's second grid row; the seventeenth tall frame starts
    at row 1 048 562 and straddles 2^20; the last frame's row0 lies beyond it.  Every stream equals png_encode_batch_dev of that frame
    alone; the two distinct tall streams decode through Pillow to the frame's rows and equal tests/png_model.py's streams (the model
    takes 0.2 s per 262 KB frame)."""
    opaque, alpha = mx.tall_frames()
    first, last = _frame(3, 2, 2, "alpha"), _frame(1, 1, 1, "mixed")
    d, dev = upload(ctx, [first, opaque, alpha, last])
    heights = mx.grid_heights()
    call = [dev[0]] + [dev[1 + k % 2] for k in range(mx.TALL_TIMES)] + [dev[3]]
    assert [h for _, _, h, _ in call] == heights
    alone = [ctx.png_encode_batch_dev(p, w, h, 1, stride=stride, frame_stride=0)[0] for p, w, h, stride in dev]
    got = ctx.png_encode_mixed_dev(call)
    want = [alone[0]] + [alone[1 + k % 2] for k in range(mx.TALL_TIMES)] + [alone[3]]
    assert len(got) == len(want) == 19
    for i in range(19):
        assert got[i] == want[i], "frame %d of 19" % i
    assert [s[25] for s in got] == [6] + [2, 6] * 8 + [2, 2] and alone[1] != alone[2]
    for f, s in ((opaque, got[1]), (alpha, got[2]), (first, got[0])):
        bpp, raw = pm.raw_rows(f)
        np.testing.assert_array_equal(pillow_rows(s).reshape(raw.shape), raw)
        assert s == pm.png_encode(f)
    d.free()


@pytest.mark.parametrize("alpha_at", ["last-pixel", "first-pixel", "first-of-second-sweep", "opaque"])
def test_encode_a_frame_beyond_the_opacity_cap(ctx, alpha_at):
    """C2.  2048 x 1025 pixels ask for 513 workgroups of the opacity pass, which caps a frame at 512 and strides: the pixels from
    512 * 256 on are looked at in a later round of the loop only.  The frame stands between two opaque 1 x 1 frames (one workgroup each
    in a grid sized for the big frame) and a 64 x 48 frame with alpha.  The only byte that is not 0xff in the last pixel, in pixel 0,
    in pixel 512 * 256 (the first one a sweep of 513 workgroups' width would leave to a workgroup that is not there), nowhere: colour
    types 6, 6, 6, 2.  Streams against the uniform device entry, Pillow's decode against the un-premultiplied rows."""
    n = mx.BIG[0] * mx.BIG[1]
    big = mx.big_frame({"last-pixel": n - 1, "first-pixel": 0, "first-of-second-sweep": mx.SECOND_SWEEP, "opaque": None}[alpha_at])
    ones = [np.array([[[9, 8, 7, 255]]], np.uint8), np.array([[[1, 2, 3, 255]]], np.uint8)]
    a64 = _frame(64, 48, 6, "alpha")
    frames = [ones[0], big, ones[1], a64]
    d, dev = upload(ctx, frames)
    got = ctx.png_encode_mixed_dev(dev)
    assert [s[25] for s in got] == [2, 2 if alpha_at == "opaque" else 6, 2, 6]
    for i, (p, w, h, stride) in enumerate(dev):
        assert ctx.png_encode_batch_dev(p, w, h, 1, stride=stride, frame_stride=0) == [got[i]], "frame %d" % i
    for f, s in zip(frames, got):
        bpp, raw = pm.raw_rows(f)
        np.testing.assert_array_equal(pillow_rows(s).reshape(raw.shape), raw)
    # reversed, the big frame is found behind the small ones' records just the same
    assert ctx.png_encode_mixed_dev(dev[::-1]) == got[::-1]
    d.free()


# ---- D. decode -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_mix(decode_case):
    files, n_edge = mx.png_edge_mix(decode_case[0])
    assert n_edge >= 12
    return files, [_model(f) for f in files]


@pytest.mark.parametrize("env", [{}, {"IPX_PNG_PAR": "1"}, {"IPX_PNG_DEC_SCRATCH_MB": "0"}, {"IPX_PNG_PAR": "1", "IPX_PNG_DEC_SCRATCH_MB": "0"}],
                         ids=["plain", "par", "scratch-groups", "par-scratch-groups"])
def test_decode_the_edge_corpus_between_other_sizes(ctx, edge_mix, monkeypatch, env):
    """D1.  tests/png_edge_corpus.py -- far matches, every distance symbol, stored blocks, one-symbol blocks, the unit edges -- between
    the files of the shipped mixed call: the model's status, pixels and palette for every file"""
    files, res = edge_mix
    setenv(monkeypatch, env)
    _check_decode(ctx, files, res)


@pytest.fixture(scope="module")
def par_mix():
    """the files of D2 as test_png_par_gpu.File (the model's answer and the model of the parallel parse).  No switch but IPX_PNG_PAR is
    set, so the corpus's Adam7 files are refused at their header and never enter the inflate."""
    mix, left_out = mx.png_par_mix()
    assert left_out == []          # none of the corpus is left out: the frames of png_edge_corpus.large() are not part of it
    out = []
    for name, data, c in mix:
        if c is not None and not c.adam7:
            out.append(file_of(c))     # shared with tests/test_png_par_edges_gpu.py: the model parses a stream once per process
        else:
            out.append(File(name, data, False, c.tags if c else (), c.damage if c else "", fast=c is None or not c.damage))
    return out


@pytest.mark.parametrize("sub", [ppm.SUB_DEFAULT, ppm.SUB_MIN])
def test_decode_the_par_corpus_in_one_call(ctx, par_mix, monkeypatch, sub):
    """D2.  Every file of tests/png_par_corpus.py with its ring, match-list and redo edge cases, and five small files of other kinds
    (two paletted) between them, in one call under IPX_PNG_PAR=1: status and pixels per file as tests/test_png_par_gpu.py derives
    them; the counters grow by the files that enter the inflate, once -- finished and handed back as the model says, with the token
    counts the model gives the finished files."""
    files = par_mix
    parsed = [f for f in files if f.parsed]
    done = [f for f in parsed if not f.redo]
    runs = [f.counts(sub) for f in done]
    expect = [len(parsed), len(done), len(parsed) - len(done), sum(r[0] for r in runs), sum(r[1] for r in runs)]
    assert len(done) >= 40 and expect[2] >= 6 and len(files) - len(parsed) >= 1
    setenv(monkeypatch, {"IPX_PNG_PAR": 1, "IPX_PNG_PAR_SUB": sub})
    before = ctx.png_decode_counts()
    frames, st = ctx.png_decode_mixed([f.data for f in files])
    grown = [a - b for a, b in zip(ctx.png_decode_counts(), before)]
    missed = []
    for i, f in enumerate(files):
        w = f.want
        if st[i] != w["status"]:
            missed.append("%s: status %d, not %d (%s)" % (f.name, st[i], w["status"], w["why"]))
        elif st[i] != dm.OK:
            assert frames[i] is None, f.name
        else:
            fr = frames[i]
            assert (fr["w"], fr["h"], fr["kind"], fr["stride"]) == (w["w"], w["h"], w["kind"], w["w"] * dm.BPP[w["kind"]]), f.name
            if not np.array_equal(fr["pix"], np.asarray(w["pix"]).reshape(fr["pix"].shape)):
                missed.append("%s: pixels differ" % f.name)
            if w["kind"] == dm.PALETTED:
                np.testing.assert_array_equal(fr["palette"], w["palette"], err_msg=f.name)
            else:
                assert fr["palette"] is None, f.name
    if missed:
        pytest.fail("\n".join(missed))
    assert grown == expect, (grown, expect)


def test_decode_adam7_beside_the_twins(ctx, monkeypatch):
    """D3.  Adam7 files of 33 x 7, 64 x 48 and 5 x 1 (RGB, RGBA, Gray), each before its non-interlaced twin, under IPX_PNG_ADAM7=1:
    every interlaced frame is its twin's, which is the model's; with IPX_PNG_PAR=1 too"""
    pairs = mx.adam7_pairs()
    files = [f for p in pairs for f in p]
    res = [_model(p[1]) for p in pairs]
    for env in ({"IPX_PNG_ADAM7": 1}, {"IPX_PNG_ADAM7": 1, "IPX_PNG_PAR": 1}):
        setenv(monkeypatch, env)
        frames, st = ctx.png_decode_mixed(files)
        assert st == [dm.OK] * 6
        for k, r in enumerate(res):
            il, twin = frames[2 * k], frames[2 * k + 1]
            assert (il["w"], il["h"], il["kind"], il["stride"]) == (twin["w"], twin["h"], twin["kind"], twin["stride"]) == \
                (r["w"], r["h"], r["kind"], r["w"] * dm.BPP[r["kind"]])
            np.testing.assert_array_equal(twin["pix"], r["pix"].reshape(twin["pix"].shape), err_msg="twin %d" % k)
            np.testing.assert_array_equal(il["pix"], twin["pix"], err_msg="pair %d" % k)
    setenv(monkeypatch, {})
    assert ctx.png_decode_mixed(files)[1] == [dm.UNSUPPORTED, dm.OK] * 3
