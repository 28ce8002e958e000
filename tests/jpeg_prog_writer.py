"""A progressive JPEG writer at the coefficient level, for the corpus of the GPU scan walk (tests/test_jpeg_prog_gpu.py).

Built on tests/jpeg_writer.py's segments, Huff and BitWriter.  libjpeg writes one scan script per colour space, one EOB run policy and
one table id per class; Go's reader takes every script T.81 allows.  This writer lays down the script it is given:

  progressive(frame, blocks, script, q=None, ...)   the whole file: SOF2, then per scan its DHT, SOS and entropy-coded data (T.81 G.1.2)
  script                                            [(components, Ss, Se, Ah, Al)] or [(components, Ss, Se, Ah, Al, options)]
  options of a scan                                 "max_eobrun": the longest EOB run to emit (default 32767; 1: a plain EOB per block)
                                                    "overrun": announce that many blocks more than the scan has in its LAST EOB run, so
                                                               the decoder's run is still pending when the next scan starts (Go does
                                                               not reset it); the next band scan's first blocks are then covered by it
                                                    "raw": the scan's symbols and bits as given, [("sym", s) | ("bits", value, n)], in
                                                           place of the coding of the blocks (damaged scans, made by hand)
                                                    "tid": the table id (0 - 3) the scan's table is defined under (default: ids cycle
                                                           when ids="cycle", else 0 -- the same id redefined before every scan)
  baseline(frame, blocks, q=None)                   the same coefficients as ONE interleaved sequential scan (jpeg_writer.scan)
  corpus()                                          the named cases of the GPU tests: (name, frame, progressive file, baseline file)

blocks[c] is (rows, cols, 64) int in ZIG-ZAG order, as for jpeg_writer.scan.  Every scan's table holds exactly the symbols the scan
uses, most frequent first, with one code per length from 1 on (jpeg_writer.spread): short codes for the first-level table, codes up to
16 bits for the bit-serial path.  A helper of the tests only."""
import functools

import numpy as np

import jpeg_writer as jw


def _sos(frame, comps, tids, ss, se, ah, al):
    out = bytes([len(comps)])
    for c in comps:
        out += bytes([frame.comps[c][0], tids[0] << 4 | tids[1]])
    return jw.seg(0xDA, out + bytes([ss, se, ah << 4 | al]))


def _table(symbols):
    """a Huffman table for the symbols used, most frequent first: lengths 1, 2, 3 ... as far as the rest still fits at 16"""
    freq = {}
    for s in symbols:
        freq[s] = freq.get(s, 0) + 1
    order = sorted(freq, key=lambda s: (-freq[s], s)) or [0]
    return jw.Huff(jw.spread(len(order), 1, 16), order)


class _Scan:
    """the symbols of one scan first (the table is built from them), the bits second"""

    def __init__(self):
        self.items = []          # ("sym", s) | ("bits", value, n)

    def sym(self, s):
        self.items.append(("sym", s))

    def bits(self, v, n):
        if n:
            self.items.append(("bits", v, n))

    def write(self, table):
        bw = jw.BitWriter(1)
        for it in self.items:
            if it[0] == "sym":
                c, ln = table.code[it[1]]
                bw.put(c, ln)
            else:
                bw.put(it[1], it[2])
        return bw.flush()


def _scan_tokens(frame, blocks, comps, ss, se, ah, al, opts, carry):
    """-> (_Scan, the decoder's pending EOB run after the scan).  carry: the run pending from the scan before."""
    S = _Scan()
    order = frame.order([(c, 0, 0) for c in comps])
    if ss == 0:
        assert se == 0
        pred = {}
        for _, c, by, bx in order:
            dc = int(blocks[c][by, bx, 0])
            if ah == 0:
                v = dc >> al
                d = v - pred.get(c, 0)
                pred[c] = v
                s = jw.size_of(d)
                S.sym(s)
                S.bits(jw.magnitude_bits(d, s), s)
            else:
                S.bits(dc >> al & 1, 1)
        return S, carry
    assert len(comps) == 1
    max_run = int(opts.get("max_eobrun", 0x7FFF))
    eobrun, be = 0, []           # the encoder's run and the correction bits buffered for its blocks

    def flush(extra=0):
        nonlocal eobrun, be
        if eobrun:
            n = eobrun + extra
            nb = n.bit_length() - 1
            S.sym(nb << 4)
            S.bits(n - (1 << nb), nb)
            eobrun = 0
        for b in be:
            S.bits(b, 1)
        be = []

    for _, c, by, bx in order:
        zz = [int(v) for v in blocks[c][by, bx]]
        t = [abs(v) >> al for v in zz]
        if carry:                # the decoder is still inside the run the scan before announced: no symbol, only corrections
            carry -= 1
            if ah == 0:
                assert not any(t[ss:se + 1]), "a block under a carried EOB run must be empty in the band"
            else:
                assert 1 not in t[ss:se + 1], "a block under a carried EOB run takes no new coefficient"
                for k in range(ss, se + 1):
                    if t[k] > 1:
                        S.bits(t[k] & 1, 1)
            continue
        if ah == 0:
            run = 0
            for k in range(ss, se + 1):
                if t[k] == 0:
                    run += 1
                    continue
                flush()
                while run > 15:
                    S.sym(jw.ZRL)
                    run -= 16
                v = t[k] if zz[k] > 0 else -t[k]
                s = jw.size_of(v)
                S.sym(run << 4 | s)
                S.bits(jw.magnitude_bits(v, s), s)
                run = 0
            if run:
                eobrun += 1
                if eobrun == max_run:
                    flush()
            continue
        # refinement (T.81 G.1.2.3, as libjpeg's encode_mcu_AC_refine orders it)
        eob = max([k for k in range(ss, se + 1) if t[k] == 1], default=-1)
        run, br = 0, []
        for k in range(ss, se + 1):
            if t[k] == 0:
                run += 1
                continue
            while run > 15 and k <= eob:
                flush()
                S.sym(jw.ZRL)
                run -= 16
                for b in br:
                    S.bits(b, 1)
                br = []
            if t[k] > 1:
                br.append(t[k] & 1)
                continue
            flush()
            S.sym(run << 4 | 1)
            S.bits(0 if zz[k] < 0 else 1, 1)
            for b in br:
                S.bits(b, 1)
            br = []
            run = 0
        if run or br:
            eobrun += 1
            be += br
            if eobrun == max_run:
                flush()
    over = int(opts.get("overrun", 0))
    if over:
        assert eobrun, "an overrun needs a run that is still open at the scan's end"
    flush(over)
    return S, over


def _quant(q):
    return list(q) if q is not None else [1 + (k >> 2) for k in range(64)]


def unused_tables(n):
    """DHT segments that define n tables no scan decodes with (ids 0 - 3 of both classes in turn, one code each): a file may carry any
    number of them, and every later DHT of the file redefines them"""
    out, seg = b"", b""
    for k in range(n):
        seg += bytes([(k >> 2 & 1) << 4 | (k & 3)]) + bytes([1] + [0] * 15) + bytes([k % 251])
        if len(seg) > 60000 or k == n - 1:
            out += jw.seg(0xC4, seg)
            seg = b""
    return out


def progressive(frame, blocks, script, q=None, ids="cycle", dri=0, extra=b""):
    """the progressive file of `blocks` by `script`; dri > 0 writes a DRI segment (and no restart markers: for the route tests only);
    extra: segments put behind the frame header"""
    comps = frame.comps
    out = jw.soi() + jw.app0_jfif() + jw.dqt([(tq, _quant(q), 0) for tq in sorted({c[3] for c in comps})]) + jw.sof(frame.w, frame.h, comps, 0xC2)
    if dri:
        out += jw.dri(dri)
    out += extra
    carry = 0
    for n, entry in enumerate(script):
        sel, ss, se, ah, al = entry[:5]
        opts = entry[5] if len(entry) > 5 else {}
        if "raw" in opts:
            S = _Scan()
            S.items = list(opts["raw"])
        else:
            S, carry = _scan_tokens(frame, blocks, list(sel), ss, se, ah, al, opts, carry)
        tid = int(opts.get("tid", n % 4 if ids == "cycle" else 0))
        syms = [it[1] for it in S.items if it[0] == "sym"]
        tids = (0, 0)
        table = None
        if syms:
            table = _table(syms)
            tc = 0 if ss == 0 else 1
            out += jw.dht([(tc, tid, table)])
            tids = (tid, 0) if tc == 0 else (0, tid)
        out += _sos(frame, list(sel), tids, ss, se, ah, al) + S.write(table)
    return out + jw.eoi()


def baseline(frame, blocks, q=None):
    """the same coefficients in one interleaved sequential scan, every block coded in full"""
    comps = frame.comps
    dct = jw.Huff(jw.spread(16, 2, 9), list(range(16)))
    act = jw.Huff(jw.spread(256, 3, 12), sorted(range(256), key=lambda s: (s & 15, s >> 4)))
    sel = [(c, 0, 0) for c in range(len(comps))]
    return (jw.soi() + jw.app0_jfif() + jw.dqt([(tq, _quant(q), 0) for tq in sorted({c[3] for c in comps})]) + jw.sof(frame.w, frame.h, comps, 0xC0) +
            jw.dht([(0, 0, dct), (1, 0, act)]) + jw.sos(comps, sel) + jw.scan(frame, sel, blocks, ({0: dct}, {0: act})) + jw.eoi())


# ---- the corpus --------------------------------------------------------------------------------------------------------------------
def colour_frame(w, h, h0=1, v0=1):
    return jw.Frame(w, h, [(1, h0, v0, 0), (2, 1, 1, 1), (3, 1, 1, 1)])


def gray_frame(w, h):
    return jw.Frame(w, h, [(1, 1, 1, 0)])


def _blocks(frame, seed, amp=200, ac=40, density=0.2):
    return jw.all_blocks(frame, np.random.default_rng(seed), amp=amp, ac=ac, density=density)


def _all(frame):
    return list(range(len(frame.comps)))


def libjpeg_script(frame):
    """the script libjpeg writes for a three-component file (jcparam.c, jpeg_simple_progression)"""
    if len(frame.comps) == 1:
        return [([0], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1), ([0], 0, 0, 1, 0), ([0], 1, 63, 1, 0)]
    return [([0, 1, 2], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([2], 1, 63, 0, 1), ([1], 1, 63, 0, 1), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1),
            ([0, 1, 2], 0, 0, 1, 0), ([2], 1, 63, 1, 0), ([1], 1, 63, 1, 0), ([0], 1, 63, 1, 0)]


def _per_component(frame, bands):
    return [([c], ss, se, ah, al) for ss, se, ah, al in bands for c in _all(frame)]


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, frame, progressive file, baseline file of the same coefficients)]"""
    out = []

    def case(name, frame, blocks, script, **kw):
        out.append((name, frame, progressive(frame, blocks, script, **kw), baseline(frame, blocks)))

    f420, f444, f422 = colour_frame(48, 40, 2, 2), colour_frame(48, 40), colour_frame(48, 40, 2, 1)
    case("libjpeg script 4:2:0", f420, _blocks(f420, 1), libjpeg_script(f420))
    case("libjpeg script 4:4:4", f444, _blocks(f444, 2), libjpeg_script(f444))
    case("no successive approximation", f422, _blocks(f422, 3),
         [(_all(f422), 0, 0, 0, 0)] + _per_component(f422, [(1, 9, 0, 0), (10, 63, 0, 0)]))
    case("bands one coefficient wide", f444, _blocks(f444, 4, density=0.5),
         [(_all(f444), 0, 0, 0, 0)] + _per_component(f444, [(1, 1, 0, 0), (2, 2, 0, 0), (3, 62, 0, 0), (63, 63, 0, 0)]))
    case("Al = 3 refined down to 0", f420, _blocks(f420, 5, amp=900, ac=120),
         [(_all(f420), 0, 0, 0, 3)] + _per_component(f420, [(1, 63, 0, 3)]) + [(_all(f420), 0, 0, 3, 2)] + _per_component(f420, [(1, 63, 3, 2)]) +
         [(_all(f420), 0, 0, 2, 1)] + _per_component(f420, [(1, 63, 2, 1)]) + [(_all(f420), 0, 0, 1, 0)] + _per_component(f420, [(1, 63, 1, 0)]))
    # a refinement whose new coefficients lie more than 16 zeros apart, with already non-zero coefficients among those zeros (ZRL across
    # them), and whose last new coefficient comes early: the EOB run starts mid-block with coefficients still to correct
    fz = colour_frame(48, 40)
    bz = _blocks(fz, 6, density=0.0)
    for c in range(3):
        b = bz[c]
        b[..., 3] = 9          # non-zero before the refinement
        b[..., 12] = -6
        b[..., 30] = 1         # new in the last pass, 26 zeros behind position 3
        b[..., 40] = 7
        b[..., 58] = -11       # still to correct when the run starts
        b[::2, ::3, 30] = 0    # some blocks have no new coefficient at all: runs of several blocks with corrections
        b[1::2, 1::2, 62] = -1
    case("ZRL across non-zero coefficients, run from mid-block", fz, bz,
         [(_all(fz), 0, 0, 0, 0)] + _per_component(fz, [(1, 63, 0, 1), (1, 63, 1, 0)]))
    case("plain EOBs only (max run 1) and runs of at most 3", f420, _blocks(f420, 7, density=0.05),
         [(_all(f420), 0, 0, 0, 0)] + [([c], 1, 63, 0, 1, {"max_eobrun": 1 + 2 * (c & 1)}) for c in range(3)] +
         [([c], 1, 63, 1, 0, {"max_eobrun": 3 - 2 * (c & 1)}) for c in range(3)])
    case("tables redefined under the same id", f444, _blocks(f444, 8), libjpeg_script(f444), ids="same")
    case("table ids 2 and 3", f444, _blocks(f444, 9),
         [(_all(f444), 0, 0, 0, 0, {"tid": 3})] + [([c], 1, 63, 0, 0, {"tid": 2 + (c & 1)}) for c in range(3)])
    case("interleaved DC scan out of frame order", f420, _blocks(f420, 10),
         [([2, 0, 1], 0, 0, 0, 1), ([1, 0], 0, 0, 1, 0), ([2], 0, 0, 1, 0)] + _per_component(f420, [(1, 63, 0, 0)]))
    # the last blocks of Y's scan are empty and its run announces 5 blocks more than there are; a DC scan goes by, then Cb's first 5
    # blocks -- empty in the band -- are still under that run
    fp = colour_frame(48, 40)
    bp = _blocks(fp, 11)
    bp[0][-1, -3:, 1:] = 0
    bp[1][0, :5, 1:] = 0
    bp[2][0, :2, 1:5] = 0
    case("an EOB run pending across scans", fp, bp,
         [(_all(fp), 0, 0, 0, 0), ([0], 1, 63, 0, 1, {"overrun": 5}), ([0], 0, 0, 0, 0), ([1], 1, 63, 0, 1), ([0], 1, 63, 1, 0, {"overrun": 2}),
          ([2], 1, 4, 0, 0), ([2], 5, 63, 0, 0), ([1], 1, 63, 1, 0)])
    # magnitudes of all ones: the scans hold many 0xff bytes, every one followed by a stuffed zero
    fs = colour_frame(48, 40)
    bs = _blocks(fs, 12, density=0.0)
    for c in range(3):
        bs[c][..., 0] = 255
        bs[c][..., 1:9] = 255
    case("stuffed 0xff bytes", fs, bs, [(_all(fs), 0, 0, 0, 0)] + _per_component(fs, [(1, 63, 0, 0)]))
    f179 = colour_frame(17, 9, 2, 2)
    case("17x9 4:2:0: luma blocks only the interleaved scan carries", f179, _blocks(f179, 13, density=0.4), libjpeg_script(f179))
    fg = gray_frame(1024, 1024)
    bg = _blocks(fg, 14, density=0.0)
    case("one EOB run of 16384 blocks", fg, bg, [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)])
    return out


def scan_data_has_stuffing(f):
    """whether any scan of the file holds 0xff 0x00"""
    i = f.find(b"\xff\xda")
    return i >= 0 and b"\xff\x00" in f[i:]
