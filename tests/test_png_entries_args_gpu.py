"""The five PNG entries that decode uploads (ipx_png_decode_batch, ipx_png_decode_mixed, ipx_plan_run_png_png,
ipx_plan_run_png_png_texts, ipx_run_png_png_mixed) on a small table of good and bad calls: the return code, the ipx_last_error text, the
per-file status list and which outputs are set, exactly as recorded in tests/golden/png_entries_args.json.  Every output is filled with
a sentinel before the call, so the record tells "left alone" (u) from "cleared to NULL" (0) from "set" (s).  The frames are a few pixels:
what is pinned is what the entries answer and where decoded frames and palettes are handed out, not the pixels (test_png_decode_gpu.py,
test_png_mixed_gpu.py and their neighbours hold those).

The golden file was recorded once from the library (python tests/test_png_entries_args_gpu.py writes it anew); the test asserts
equality, it never derives an expectation from the code under test at run time."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import png_adam7_corpus as ac
import png_corpus as pc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden", "png_entries_args.json")
ENTRIES = ["ipx_png_decode_batch", "ipx_png_decode_mixed", "ipx_plan_run_png_png", "ipx_plan_run_png_png_texts", "ipx_run_png_png_mixed"]
ENV = ("IPX_PNG_ADAM7", "IPX_PNG_PAR", "IPX_PNG_PAR_SUB", "IPX_PNG_DEC_SCRATCH_MB", "IPX_PNG_MIXED_CHUNK_MB", "IPX_HOST_CHUNK_PNG_DEC",
       "IPX_HOST_CHUNK_PNG")
SENTINEL = 0x5A5A00          # what every output pointer holds before a call
UNTOUCHED = 77               # what every status word holds before a call
PALETTED = 3

# the valid call's four files: a 3x2 RGB, a 3x2 paletted, a 5x1 gray and a 3x2 RGBA
RGB = pc.of_type(2, 8, False, 2, 3, seed=1)
PAL = pc.of_type(3, 8, True, 2, 3, seed=2)
GRAY = pc.of_type(0, 8, False, 1, 5, seed=3)
RGBA = pc.of_type(6, 8, False, 2, 3, seed=4)
PAL2 = pc.of_type(3, 4, True, 1, 5, seed=5)
FOUR = [RGB, PAL, GRAY, RGBA]
FILES = {
    "valid": FOUR,
    "truncated": [RGB, RGB[:len(RGB) - 20], RGBA],
    "adam7_unset": [RGB, ac.of_type(2, 8, False, 2, 3, seed=6), RGBA],
    "pal_rgb_pal": [PAL, RGB, PAL2],
    # a thumbnail of 14000 without the crop is 70000 pixels wide for a 5x1 file: past the 65535 a plan takes.  The broken file between
    # the two keeps its own status
    "no_plan": [GRAY, RGB[:len(RGB) - 20], GRAY],
}


def _cases(name):
    """(case name, what it changes of the valid call) in the order they are run"""
    c = [("valid", {}), ("n_0", dict(n=0)), ("n_negative", dict(n=-1)), ("null_ctx", dict(null="ctx"))]
    if name == "ipx_png_decode_batch":
        c += [("null_" + p, dict(null=p)) for p in ("files", "w", "h", "kind", "frames", "status", "owner")]
        c += [("w_0_h_5", dict(w=0, h=5)), ("kind_7", dict(kind=7)), ("kind_minus_2", dict(kind=-2)),
              ("paletted_3x2", dict(w=3, h=2, kind=PALETTED)), ("gray_5x1", dict(w=5, h=1))]
    elif name == "ipx_png_decode_mixed":
        c += [("null_" + p, dict(null=p)) for p in ("files", "frames", "status", "owner")]
        c += [("n_65536", dict(n=65536))]
    elif name.startswith("ipx_plan_run"):
        c += [("null_" + p, dict(null=p)) for p in ("plan", "files", "status", "result")]
        if name.endswith("_texts"):
            c += [("null_texts", dict(null="texts")), ("texts_refused", dict(texts="refused"))]
    else:
        c += [("null_" + p, dict(null=p)) for p in ("ops", "files", "status", "result")]
        c += [("valid_texts", dict(texts="good")), ("ops_sw_5", dict(sw=5)), ("ops_glyphs", dict(glyphs=True)),
              ("texts_refused", dict(texts="refused")), ("no_plan", dict(files="no_plan"))]
    c += [("truncated", dict(files="truncated")), ("adam7_unset", dict(files="adam7_unset"))]
    if name in ("ipx_png_decode_mixed", "ipx_run_png_png_mixed"):
        c += [("pal_rgb_pal", dict(files="pal_rgb_pal"))]
    return c


def _state(p):
    return "0" if not p else "u" if p == SENTINEL else "s"


def _texts(m, n, refused):
    """one small glyph per file; refused: text 1 carries 257 glyphs, one more than the texts check takes"""
    g = {"mask": np.full((2, 2), 255, np.uint8), "dr": (0, 0, 2, 2), "mp": (0, 0)}
    return m._text_array([([g] * (257 if refused and i == 1 else 1), (1, 2, 3, 4)) for i in range(n)])


def _call(m, ctx, plan, name, over):
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
    if name.startswith("ipx_png_decode"):
        owner = C.c_void_p(SENTINEL)
        powner = None if null == "owner" else C.byref(owner)
        if name == "ipx_png_decode_batch":
            w, hh, kind = C.c_int(over.get("w", 0)), C.c_int(over.get("h", 0)), C.c_int(over.get("kind", -1))
            b = _lib.PngBatch(SENTINEL, -1, 0, SENTINEL)
            rc = L.ipx_png_decode_batch(h, None, pfiles, n, None if null == "w" else C.byref(w), None if null == "h" else C.byref(hh),
                                        None if null == "kind" else C.byref(kind), None if null == "frames" else C.byref(b), pstatus, powner)
            rec["whk"] = [w.value, hh.value, kind.value]
            rec["pix"], rec["palettes"], rec["stride"] = _state(b.pix), _state(b.palettes), b.stride
        else:
            fr = (_lib.PngFrame * room)()
            for i in range(room):
                fr[i].pix, fr[i].palette = SENTINEL, SENTINEL
            rc = L.ipx_png_decode_mixed(h, None, pfiles, n, None if null == "frames" else fr, pstatus, powner)
            rec["pix"] = "".join(_state(fr[i].pix) for i in range(shown))
            rec["palette"] = "".join(_state(fr[i].palette) for i in range(shown))
            rec["whk"] = [[fr[i].w, fr[i].h, fr[i].kind] for i in range(shown)]
        text = L.ipx_last_error().decode()
        rec["owner"] = _state(owner.value)
        if rec["owner"] == "s":
            L.ipx_png_frames_free(ctx.handle, owner)
    else:
        outs = [(_lib.Bytes * room)() for _ in range(3)]
        for o in outs:
            for i in range(room):
                o[i].data, o[i].len = SENTINEL, 1
        res = C.c_void_p(SENTINEL)
        pres = None if null == "result" else C.byref(res)
        tarr, keep = (None, None)
        if name.endswith("_texts") and null != "texts" or over.get("texts"):
            tarr, keep = _texts(m, room, over.get("texts") == "refused")
        if name == "ipx_run_png_png_mixed":
            ops = _lib.PoolOps()
            ops.do_resize, ops.resize_w, ops.resize_h, ops.keep_aspect = 1, 4, 3, 0
            ops.do_thumbnail, ops.thumb_size, ops.crop_to_fit = 1, 2, 1
            ops.do_watermark = 1
            if over.get("files") == "no_plan":
                ops.do_resize, ops.thumb_size, ops.crop_to_fit = 0, 14000, 0
            ops.sw = over.get("sw", 0)
            garr = gkeep = None
            if over.get("glyphs"):
                garr, gkeep = m._glyph_array([{"mask": np.full((2, 2), 255, np.uint8), "dr": (0, 0, 2, 2), "mp": (0, 0)}])
                ops.glyphs, ops.n_glyphs = garr, 1
            rc = L.ipx_run_png_png_mixed(h, None if null == "ops" else C.byref(ops), n, pfiles, tarr, outs[0], outs[1], outs[2], pstatus, pres)
            del garr, gkeep
        elif name.endswith("_texts"):
            rc = L.ipx_plan_run_png_png_texts(h, None if null == "plan" else plan.handle, n, pfiles, tarr, outs[0], outs[1], outs[2], pstatus, pres)
        else:
            rc = L.ipx_plan_run_png_png(h, None if null == "plan" else plan.handle, n, pfiles, outs[0], outs[1], outs[2], pstatus, pres)
        text = L.ipx_last_error().decode()
        del keep
        for k, o in zip(("resize", "thumbnail", "watermark"), outs):
            rec[k] = "".join(_state(o[i].data) for i in range(shown))
        rec["result"] = _state(res.value)
        if rec["result"] == "s":
            L.ipx_jpeg_result_free(ctx.handle, res)
    return dict(rc=rc, error=text, status=[status[i] for i in range(shown)], **rec)


def record(m, ctx, plan):
    return {name: {case: _call(m, ctx, plan, name, over) for case, over in _cases(name)} for name in ENTRIES}


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as m
    c = m.Context(lanes=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plan(ctx):
    """the uniform legs' plan: 3x2 uploads, copy-only watermark (what the _texts entry asks for)"""
    p = ctx.plan(3, 2, resize=(4, 3, False), thumbnail=(2, True), watermark=True)
    yield p
    p.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_golden_files(golden):
    assert {n: [c for c, _ in _cases(n)] for n in ENTRIES} == {n: list(golden[n]) for n in golden}


@pytest.mark.parametrize("name", ENTRIES)
def test_what_the_entry_answers(ctx, plan, golden, monkeypatch, name):
    import imageprocessor_amd as m
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for case, over in _cases(name):
        assert _call(m, ctx, plan, name, over) == golden[name][case], "%s, case %s" % (name, case)
    assert golden[name]["valid"]["rc"] == 0 and 0 in golden[name]["valid"]["status"]


if __name__ == "__main__":      # records the golden file from the library as built: run once, on the commit before a change to these entries
    sys.path.insert(0, os.path.dirname(HERE))
    import imageprocessor_amd as m
    for k in ENV:
        os.environ.pop(k, None)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with m.Context(lanes=2) as c:
        p = c.plan(3, 2, resize=(4, 3, False), thumbnail=(2, True), watermark=True)
        got = record(m, c, p)
        again = record(m, c, p)
        p.close()
    assert got == again, "two recordings differ"
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=False)
        f.write("\n")
    print("wrote %s: %d entries, %d calls" % (out, len(got), sum(len(v) for v in got.values())))
