"""GIF files for the parallel code walk (csrc/ipx_gif_dec_par.hip, IPX_GIF_PAR=1): streams of tests/lzw_writer.py taken apart into
their codes, changed code by code and packed again at the widths the reader reads them with, so that a given code lands in a given
lane of a given round of tests/gif_par_model.py.  A helper of the tests only."""
import numpy as np

import gif_decode_model as dm
import gif_par_model as pm
import lzw_writer as lw


def codes_of(data, lit):
    """every code of a valid stream, clear and EOF codes included"""
    clear, eof = 1 << lit, (1 << lit) + 1
    out, bit, t = [], 0, 0
    while True:
        w = pm.width(t, lit)
        assert bit + w <= 8 * len(data)
        v = (int.from_bytes(data[bit >> 3:(bit >> 3) + 3], "little") >> (bit & 7)) & ((1 << w) - 1)
        out.append(v)
        bit += w
        if v == eof:
            return out
        t = 0 if v == clear else t + 1


def pack(codes, lit):
    """the codes LSB first, each at the width of its ordinal (a code that does not fit its width is cut to it)"""
    clear = 1 << lit
    acc, nacc, t = 0, 0, 0
    for v in codes:
        w = pm.width(t, lit)
        acc |= (v & ((1 << w) - 1)) << nacc
        nacc += w
        t = 0 if v == clear else t + 1
    return acc.to_bytes((nacc + 7) // 8, "little")


def container(w, h, pal, lit, data, sub=255, interlace=False, seed=0, tail=b""):
    """lzw_writer.gif's container around these LZW bytes; tail: bytes put between the last sub-block and the block terminator"""
    pal = np.asarray(pal, np.uint8).reshape(-1, 3)
    bits = max(1, (len(pal) - 1).bit_length())
    assert len(pal) == 1 << bits
    out = bytearray(b"GIF89a")
    out += w.to_bytes(2, "little") + h.to_bytes(2, "little") + bytes([0x80 | (bits - 1), 0, 0])
    out += pal.tobytes()
    out += b"\x2c" + bytes(4) + w.to_bytes(2, "little") + h.to_bytes(2, "little") + bytes([0x40 if interlace else 0])
    out.append(lit)
    out += lw.sub_blocks(data, sub, seed)[:-1] + tail + b"\0"
    return bytes(out + b"\x3b")


def palette(n, seed):
    return np.random.default_rng(seed + 500).integers(0, 256, (n, 3)).astype(np.uint8)


def noise(w, h, seed, ncol=256):
    return np.random.default_rng(seed).integers(0, ncol, (h, w)).astype(np.uint8)


def walk(data):
    """(the model's answer, the stream, the parallel walk) of a file whose container parses"""
    s = pm.stream_of(data)
    return dm.decode(data), s, pm.par_walk(s)


def last_round(par):
    """(valid lanes, what ended it) of the round that ended the walk"""
    return par.trace[-1][1], par.trace[-1][2]


def eof_in_lane(lane, seed=11):
    """a one-row noise frame (no leading clear: the code's index is its ordinal) whose EOF code sits in this lane of its round;
    the frame's width by search"""
    for w in range(130, 400):
        idx = noise(w, 1, seed + w)
        data, _ = lw.gif(idx, palette(256, seed), lit=8, clear="never", lead=False)
        want, s, par = walk(data)
        if not par.redo and last_round(par) == (lane, 2) and par.rounds >= 3:
            return data, idx
    raise AssertionError("no frame width puts the EOF code in lane %d" % lane)


def code_above_hi_in_lane(lane, w=160, h=120, seed=21):
    """a noise frame without a leading clear whose code at ordinal 128 + lane is eof + t + 1: one above the KwKwK code"""
    idx = noise(w, h, seed)
    data, _ = lw.lzw(idx, 8, clear="never", lead=False)
    codes = codes_of(data, 8)
    t = 128 + lane
    codes[t] = 257 + t + 1
    return container(w, h, palette(256, seed), 8, pack(codes, 8))


def garbage_behind_a_clear(w=160, h=120):
    """a clear code in mid-round at width 10, so that the lanes behind it read 10-bit codes where 9-bit ones lie, and one of them reads
    a code above its hi; the seed by search"""
    for seed in range(40):
        idx = noise(w, h, 300 + seed)
        data, _ = lw.gif(idx, palette(256, seed), lit=8, clear="every", every=300 + seed, lead=False)
        want, s, par = walk(data)
        if not par.redo and any(stop == 1 and 0 < nv < 60 and (kind[nv + 1:] == 4).any() for _, nv, stop, kind in par.trace):
            return data, idx
    raise AssertionError("no seed puts an invalid-looking code behind a clear")


def redo_cases(w=160, h=120, seed=31):
    """[(name, file, status of the model)]: streams the parallel walk leaves to the serial walk"""
    pal = palette(256, seed)
    idx = noise(w, h, seed)
    good, _ = lw.gif(idx, pal, lit=8)
    lzw, _ = lw.lzw(idx, 8)
    codes = codes_of(lzw, 8)
    more, _ = lw.lzw(np.append(idx.ravel(), 7), 8)
    short_pal = np.minimum(noise(w, h, seed + 1, 4), 3)
    short_pal[h // 2, w // 2] = 5                                      # a literal below clear = 8, past the four colours
    out = [("truncated data", good[:len(good) * 2 // 3]),
           ("EOF before the frame is full", container(w, h, pal, 8, pack(codes[:len(codes) // 2] + [257], 8))),
           ("one byte too many", container(w, h, pal, 8, more)),
           ("code above hi in lane 0", code_above_hi_in_lane(0, w, h)),
           ("code above hi in lane 63", code_above_hi_in_lane(63, w, h)),
           ("literal past a short palette", container(w, h, palette(4, seed), 3, lw.lzw(short_pal, 3)[0])),
           ("extra sub-block behind the EOF code", container(w, h, pal, 8, lzw, tail=b"\x02ab")),
           ("missing EOF code, complete frame", container(w, h, pal, 8, pack(codes[:-1], 8)))]
    return [(name, data, dm.entry_status(dm.decode(data), (w, h))) for name, data in out]
