"""The model of the parallel GIF code walk (tests/gif_par_model.py, the restatement of csrc/ipx_gif_dec_par.hip) on the CPU: the closed
form of a code's width and bit offset against the serial reader's bookkeeping, and on the edge corpus (tests/gif_edge_corpus.py), the
Pillow corpus and every stream of tests/golden/gif_dec_kats.json the walk either writes the serial walk's records -- which expand to
the frame of tests/gif_decode_model.py -- or raises redo, and it raises redo on exactly the streams the serial walk does not accept at
an EOF code.  Also: the new ABI entries are exported, declared behind a comment, in the ctypes table, and refuse NULL arguments without
a GPU."""
import json
import os
import re

import numpy as np
import pytest

import gif_corpus
import gif_decode_model as dm
import gif_edge_corpus as ge
import gif_par_model as pm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "gif_dec_kats.json")) as f:
    KATS = json.load(f)


@pytest.mark.parametrize("lit", range(2, 9))
def test_closed_form_is_the_serial_readers(lit):
    """compress/lzw's hi / width / overflow, stepped 5001 times without a clear"""
    eof = (1 << lit) + 1
    width, hi, overflow, bit = lit + 1, eof, 1 << (lit + 1), 0
    ts = np.arange(5001)
    vw, vb = pm._v_width(ts, lit), pm._v_bits_before(ts, lit)
    for t in range(5001):
        assert (pm.width(t, lit), pm.bits_before(t, lit)) == (width, bit) == (vw[t], vb[t]), (lit, t)
        assert width == min(12, max(lit + 1, pm.bitlen(eof + t)))
        bit += width
        hi += 1
        if hi >= overflow:
            if width == 12:
                hi -= 1
            else:
                width += 1
                overflow <<= 1


def _check(name, data):
    """-> "skipped" (never reaches the walk), "redo" or "par" """
    want = dm.decode(data)
    if want["stage"] == "container" or dm.entry_status(want) == dm.UNSUPPORTED:
        return "skipped"
    s = pm.stream_of(data)
    ser, par = pm.serial_walk(s), pm.par_walk(s)
    assert (ser.status == 0) == want["ok"], (name, ser.how, want["error"])
    clean = ser.status == 0 and ser.how == "eof"
    assert par.redo == (not clean), (name, ser.how, par.how)
    if par.redo:
        assert par.records == [] and par.status != 0, name
        return "redo"
    assert par.records == ser.records and par.count == ser.count == s.w * s.h, name
    np.testing.assert_array_equal(pm.expand(s, par.records, par.count), want["index"], err_msg=name)
    return "par"


@pytest.fixture(scope="module")
def edge_corpus():
    return ge.corpus()


@pytest.mark.parametrize("part", range(4))
def test_edge_corpus(edge_corpus, part):
    assert len(edge_corpus) > 30
    got = [_check(name, data) for name, data, _, _, _ in edge_corpus[part::4]]
    assert got == ["par"] * len(got)


def test_pillow_corpus():
    got = [_check(name, data) for name, data in gif_corpus.corpus()]
    assert got == ["par"] * len(got) and got


def test_known_answers():
    got = {k["name"]: _check(k["name"], bytes.fromhex(k["data"])) for k in KATS}
    assert sum(1 for v in got.values() if v == "par") >= 10 and sum(1 for v in got.values() if v == "redo") >= 5, got
    for name, v in got.items():
        if "missing EOF" in name or "code above hi" in name:
            assert v == "redo", name                                     # accepted or refused, but by the serial walk
        if "kwkwk" in name or "full dictionary" in name or "clear in mid-stream" in name:
            assert v == "par", name


def test_deep_chains_and_rounds():
    """a one-colour frame: every code is KwKwK of the one before, so the chain inside a round is 63 hops deep; rounds are full"""
    import lzw_writer as lw
    idx = np.zeros((60, 80), np.uint8)
    data, _ = lw.gif(idx, np.zeros((4, 3), np.uint8), lit=2)
    s = pm.stream_of(data)
    par = pm.par_walk(s)
    assert not par.redo and par.records == pm.serial_walk(s).records
    codes = [r[2] & 4095 for r in par.records]
    assert len(codes) > 64 and all(b == a + 1 for a, b in zip(codes[1:64], codes[2:65]))
    assert par.rounds == 1 + -(-(len(codes) + 1) // pm.LANES)             # the leading clear ends round one at lane 0; then the codes and the EOF code
    np.testing.assert_array_equal(pm.expand(s, par.records, par.count), idx)


def test_entries_are_exported_declared_and_refuse_null_arguments_without_a_gpu():
    import ctypes as C
    from imageprocessor_amd import _lib, build
    build.build()
    import imageprocessor_amd as m
    L = m.lib()
    header = open(os.path.join(ROOT, "include", "ipx.h")).read()
    res, args = _lib.SIGNATURES["ipx_gif_decode_counts"]
    assert res is C.c_int and len(args) == 2 and args[1] == C.POINTER(C.c_longlong)
    res, args = _lib.SIGNATURES["ipx_pool_gif_decode_counts"]
    assert res is C.c_int and len(args) == 3 and args[1] is C.c_int and args[2] == C.POINTER(C.c_longlong)
    mt = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ipx_gif_decode_counts\(ipx_ctx \*ctx, long long counts\[4\]\);", header, re.S)
    assert mt, "ipx_gif_decode_counts is not declared behind a comment"
    for word in ("IPX_GIF_PAR=1", "[0]", "[1]", "[2]", "[3]", "redo", "bitlen(eof + t)"):
        assert word in mt.group(1), word
    assert header.index("int ipx_gif_decode_batch(") < mt.start() < header.index("int ipx_plan_run_gif_gif(")
    assert re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ipx_pool_gif_decode_counts\(const ipx_pool \*pool, int slot, long long counts\[4\]\);",
                     header, re.S)
    assert hasattr(L, "ipx_gif_decode_counts") and hasattr(L, "ipx_pool_gif_decode_counts")
    counts = (C.c_longlong * 4)()
    assert L.ipx_gif_decode_counts(None, counts) == dm.INVALID
    assert L.ipx_gif_decode_counts(None, None) == dm.INVALID
    assert L.ipx_pool_gif_decode_counts(None, 0, counts) == dm.INVALID
    assert hasattr(m.Context, "gif_decode_counts") and hasattr(m.Pool, "gif_decode_counts")
