"""The two mixed-size JPEG entries (ipx_run_jpeg_jpeg_mixed, ipx_jpeg_decode_mixed) on a small table of good and bad calls: the return
code, the ipx_last_error text, the per-file status list and which outputs are set, exactly as recorded in
tests/golden/jpeg_mixed_entry_args.json.  Every output and status word is filled with a sentinel before the call, so the record tells
"left alone" (u) from "cleared to NULL" (0) from "set" (s).  The files are a few pixels: what is pinned is what the entries answer and
where streams and planes are handed out, not the pixels (test_jpeg_mixed_gpu.py and test_jpeg_mixed_edges_gpu.py hold those).  The PNG
entries' twin is test_png_entries_args_gpu.py.

The golden file was recorded once from the library (python tests/test_jpeg_mixed_entry_args_gpu.py writes it anew); the test asserts
equality, it never derives an expectation from the code under test at run time."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_411_corpus as c411
import jpeg_writer as jw

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "jpeg_mixed_entry_args.json")
ENTRIES = ["ipx_jpeg_decode_mixed", "ipx_run_jpeg_jpeg_mixed"]
ENV = ("IPX_JPEG_MIXED_GROUP", "IPX_JPEG_MIXED_CHUNK_MB", "IPX_JPEG_LANE_ARENA", "IPX_DEBUG_J2J", "IPX_JPEG_411", "IPX_JPEG_CMYK",
       "IPX_JPEG_PAR", "IPX_JPEG_PAR_SUB", "IPX_JPEG_PROG_GPU", "IPX_JPEG_HOST_GROUP")
SENTINEL = 0x5A5A00          # what every output pointer holds before a call
UNTOUCHED = 77               # what every status word holds before a call
QUALITY = 85


def _file(w, h, comps, seed):
    fr = jw.Frame(w, h, comps)
    return c411.baseline(fr, c411.blocks(fr, seed))


def _ycc(h0, v0):
    return [(1, h0, v0, 0), (2, 1, 1, 1), (3, 1, 1, 1)]


# the valid call's four files: a 3x2 4:2:0, a 3x2 4:4:4, a 5x1 Gray and a 3x2 4:2:2
F420 = _file(3, 2, _ycc(2, 2), 1)
F444 = _file(3, 2, _ycc(1, 1), 2)
GRAY = _file(5, 1, [(1, 1, 1, 0)], 3)
F422 = _file(3, 2, _ycc(2, 1), 4)
F411 = _file(3, 2, _ycc(4, 1), 5)            # refused while IPX_JPEG_411 is unset
CUT = c411.cut_in_scan(F420)
FOUR = [F420, F444, GRAY, F422]
FILES = {
    "valid": FOUR,
    "truncated": [F420, CUT, F422],
    "unsupported_neighbour": [F420, F411, F444],
    # a thumbnail of 14000 without the crop is 70000 pixels wide for a 5x1 file: past the 65535 a plan takes.  The broken file between
    # the two keeps its own status
    "no_plan": [GRAY, CUT, GRAY],
}


def _cases(name):
    """(case name, what it changes of the valid call) in the order they are run"""
    c = [("valid", {}), ("n_0", dict(n=0)), ("n_negative", dict(n=-1)), ("null_ctx", dict(null="ctx"))]
    if name == "ipx_jpeg_decode_mixed":
        c += [("null_" + p, dict(null=p)) for p in ("files", "frames", "status", "owner")]
        c += [("n_65536", dict(n=65536))]
    else:
        c += [("null_" + p, dict(null=p)) for p in ("ops", "files", "status", "result")]
        c += [("n_65536", dict(n=65536)), ("valid_texts", dict(texts="good")), ("texts_with_ops_glyphs", dict(texts="good", glyphs=True)),
              ("ops_glyphs", dict(glyphs=True)), ("ops_sw_5", dict(sw=5)), ("texts_refused", dict(texts="refused")),
              ("no_plan", dict(files="no_plan"))]
    c += [("truncated", dict(files="truncated")), ("unsupported_neighbour", dict(files="unsupported_neighbour"))]
    return c


def _state(p):
    return "0" if not p else "u" if p == SENTINEL else "s"


GLYPH = {"mask": np.full((2, 2), 255, np.uint8), "dr": (0, 0, 2, 2), "mp": (0, 0)}


def _texts(m, n, refused):
    """one small glyph per file; refused: text 1 carries 257 glyphs, one more than the texts check takes"""
    return m._text_array([([GLYPH] * (257 if refused and i == 1 else 1), (1, 2, 3, 4)) for i in range(n)])


def _call(m, ctx, name, over):
    """one call -> what the golden file holds of it.  Every array handed over has room for max(n, 65536 where the case asks) entries."""
    from imageprocessor_amd import _lib
    L = m.lib()
    files = FILES[over.get("files", "valid")]
    n = over.get("n", len(files))
    room = max(n, len(files), 1)
    null = over.get("null")
    arr = (_lib.Bytes * room)()
    for i, f in enumerate(files):
        arr[i].data, arr[i].len = C.cast(C.c_char_p(f), C.c_void_p), len(f)
    status = (C.c_int * room)(*[UNTOUCHED] * room)
    h = None if null == "ctx" else ctx.handle
    pfiles = None if null == "files" else arr
    pstatus = None if null == "status" else status
    shown = max(0, min(n, len(files)))          # the entries of the arrays a record lists
    rec = {}
    if name == "ipx_jpeg_decode_mixed":
        owner = C.c_void_p(SENTINEL)
        fr = (_lib.JpegFrame * room)()
        for i in range(room):
            fr[i].y, fr[i].cb, fr[i].cr = SENTINEL, SENTINEL, SENTINEL
            fr[i].w, fr[i].h, fr[i].ratio, fr[i].ystride, fr[i].cstride = -1, -1, -1, -1, -1
        rc = L.ipx_jpeg_decode_mixed(h, None, pfiles, n, None if null == "frames" else fr, pstatus, None if null == "owner" else C.byref(owner))
        text = L.ipx_last_error().decode()
        for k in ("y", "cb", "cr"):
            rec[k] = "".join(_state(getattr(fr[i], k)) for i in range(shown))
        rec["whr"] = [[fr[i].w, fr[i].h, fr[i].ratio] for i in range(shown)]
        rec["strides"] = [[fr[i].ystride, fr[i].cstride] for i in range(shown)]
        rec["owner"] = _state(owner.value)
        if rec["owner"] == "s":
            L.ipx_jpeg_planes_free(ctx.handle, owner)
    else:
        outs = [(_lib.Bytes * room)() for _ in range(3)]
        for o in outs:
            for i in range(room):
                o[i].data, o[i].len = SENTINEL, 1
        res = C.c_void_p(SENTINEL)
        tarr, keep = _texts(m, room, over["texts"] == "refused") if over.get("texts") else (None, None)
        ops = _lib.PoolOps()
        ops.do_resize, ops.resize_w, ops.resize_h, ops.keep_aspect = 1, 4, 3, 0
        ops.do_thumbnail, ops.thumb_size, ops.crop_to_fit = 1, 2, 1
        ops.do_watermark = 1
        if over.get("files") == "no_plan":
            ops.do_resize, ops.thumb_size, ops.crop_to_fit = 0, 14000, 0
        ops.sw = over.get("sw", 0)
        garr = gkeep = None
        if over.get("glyphs"):
            garr, gkeep = m._glyph_array([GLYPH])
            ops.glyphs, ops.n_glyphs = garr, 1
            ops.col[0], ops.col[1], ops.col[2], ops.col[3] = 1, 2, 3, 4
        rc = L.ipx_run_jpeg_jpeg_mixed(h, None if null == "ops" else C.byref(ops), n, pfiles, tarr, QUALITY, outs[0], outs[1], outs[2], pstatus,
                                       None if null == "result" else C.byref(res))
        text = L.ipx_last_error().decode()
        del garr, gkeep, keep
        for k, o in zip(("resize", "thumbnail", "watermark"), outs):
            rec[k] = "".join(_state(o[i].data) for i in range(shown))
        rec["result"] = _state(res.value)
        if rec["result"] == "s":
            L.ipx_jpeg_result_free(ctx.handle, res)
    return dict(rc=rc, error=text, status=[status[i] for i in range(shown)], **rec)


def record(m, ctx):
    return {name: {case: _call(m, ctx, name, over) for case, over in _cases(name)} for name in ENTRIES}


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_golden_files(golden):
    assert {n: [c for c, _ in _cases(n)] for n in ENTRIES} == {n: list(golden[n]) for n in golden}


@pytest.mark.parametrize("name", ENTRIES)
def test_what_the_entry_answers(ctx, golden, monkeypatch, name):
    import imageprocessor_amd as m
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for case, over in _cases(name):
        assert _call(m, ctx, name, over) == golden[name][case], "%s, case %s" % (name, case)
    assert golden[name]["valid"]["rc"] == 0 and golden[name]["valid"]["status"] == [0, 0, 0, 0]


if __name__ == "__main__":      # records the golden file from the library as built: run once, on the commit before a change to these entries
    sys.path.insert(0, os.path.dirname(HERE))
    import imageprocessor_amd as m
    for k in ENV:
        os.environ.pop(k, None)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with m.Context(lanes=2) as c:
        got = record(m, c)
        again = record(m, c)
    assert got == again, "two recordings differ"
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=False)
        f.write("\n")
    print("wrote %s: %d entries, %d calls" % (out, len(got), sum(len(v) for v in got.values())))
