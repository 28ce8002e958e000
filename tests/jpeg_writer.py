"""A JPEG writer that works at the coefficient level, for the JPEG decoder's edge corpus (tests/jpeg_edge_corpus.py).

libjpeg (Pillow) and the project's encoder write one kind of stream: 8-bit DQT, two Annex K or optimised tables per class, SOF0,
components 1/2/3 in frame order, a single interleaved scan, EOB after the last non-zero coefficient, padding with 1s.  Go's reader
takes much more.  This writer lays down exactly what it is told:

  huff(counts, vals)                     a Huffman table from code-length counts (BITS) and symbols (HUFFVAL), canonical codes
  spread(n, lo, hi)                      code-length counts for n symbols: one code per length from lo on, the rest at hi
  complete(ln)                           the counts of a complete table: every code of length ln
  Segments: soi(), eoi(), app0_jfif(), app14_adobe(transform), app(n, data), com(data), dqt([(tq, q, pq)]),
            dht([(tc, th, table)]), sof(w, h, comps, marker), dri(n), sos(sel)
  Frame(w, h, comps)                     comps: [(id, h, v, tq)]; the MCU grid and each component's block grid as Go sees them
  scan(frame, sel, blocks, tables, ri=0, pad=1, tokens=None)
                                         the entropy-coded segment(s) of one scan: blocks[c] is (rows, cols, 64) int in ZIG-ZAG order;
                                         sel = [(component index, td, ta)]; restart markers every ri MCUs, RSTn numbered mod 8
  tokens                                 per (component, block row, block col): a symbol list that replaces the block's own coding:
                                           ("dc", diff)                      DC size category and magnitude bits of diff
                                           ("dcs", size, bits)               a DC symbol of that size with those raw magnitude bits
                                           ("ac", run, value)                run / size symbol and magnitude bits
                                           ("sym", symbol)                   an AC symbol with no magnitude bits (EOB, ZRL, or a run
                                                                             that passes zig 63, whose bits Go never reads)

Coefficients in ZIG-ZAG order throughout; ZIG maps zig-zag index to natural index.  A helper of the tests only."""
import struct

import numpy as np

ZIG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                62, 63])
EOB, ZRL = 0x00, 0xF0


def size_of(v):
    """the magnitude category of v (T.81 F.1.2.1): 0 for 0, else the bit length of |v|"""
    return int(abs(int(v))).bit_length()


def magnitude_bits(v, t):
    """the t low-order bits that follow a symbol of size t for the value v (negative values: v - 1 in t bits)"""
    v = int(v)
    return v if v >= 0 else v + (1 << t) - 1


class Huff:
    def __init__(self, counts, vals):
        counts, vals = list(counts), list(vals)
        assert len(counts) == 16 and sum(counts) == len(vals) and 0 < len(vals) <= 256
        self.counts, self.vals = counts, vals
        self.code = {}
        code, k = 0, 0
        for ln in range(1, 17):
            for _ in range(counts[ln - 1]):
                assert code < 1 << ln, "over-subscribed table"
                self.code.setdefault(vals[k], (code, ln))
                code += 1
                k += 1
            code <<= 1


def huff(counts, vals):
    return Huff(counts, vals)


def spread(n, lo=1, hi=16):
    """code-length counts for n symbols: one code at each length lo, lo + 1, ... as long as the rest still fit at length hi, then all
    the rest at hi (an incomplete table unless the capacity is used exactly)"""
    counts = [0] * 16
    room = 1 << hi                                      # capacity in codes of length hi
    left = n
    for ln in range(lo, hi):
        cost = 1 << (hi - ln)
        if left > 1 and room - cost >= left - 1:
            counts[ln - 1] += 1
            room -= cost
            left -= 1
    assert left <= room, "too many symbols for the lengths"
    counts[hi - 1] += left
    return counts


def complete(ln):
    """counts of a complete table: every code of length ln (2 ** ln symbols, the all-ones code among them)"""
    counts = [0] * 16
    counts[ln - 1] = 1 << ln
    return counts


# ---- segments --------------------------------------------------------------------------------------------------------------------
def seg(marker, payload):
    assert len(payload) + 2 <= 0xFFFF
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def soi():
    return b"\xff\xd8"


def eoi():
    return b"\xff\xd9"


def app0_jfif():
    return seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")


def app14_adobe(transform):
    return seg(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform))


def app(n, data):
    return seg(0xE0 + n, data)


def com(data):
    return seg(0xFE, data)


def dqt(tables):
    """tables: [(tq, q (64 values, zig-zag order), pq)]; pq 1 writes 16-bit entries"""
    out = b""
    for tq, q, pq in tables:
        q = [int(x) for x in q]
        assert len(q) == 64
        out += bytes([pq << 4 | tq]) + (struct.pack(">64H", *q) if pq else bytes(q))
    return seg(0xDB, out)


def dht(tables):
    """tables: [(tc, th, Huff)]"""
    out = b""
    for tc, th, t in tables:
        out += bytes([tc << 4 | th]) + bytes(t.counts) + bytes(t.vals)
    return seg(0xC4, out)


def sof(w, h, comps, marker=0xC0):
    """comps: [(id, h, v, tq)]"""
    out = struct.pack(">BHHB", 8, h, w, len(comps))
    for cid, ch, cv, tq in comps:
        out += bytes([cid, ch << 4 | cv, tq])
    return seg(marker, out)


def dri(n):
    return seg(0xDD, struct.pack(">H", n))


def sos(comps, sel):
    """sel: [(component index, td, ta)]; comps as for sof (the ids are taken from there); Ss = 0, Se = 63, Ah = Al = 0"""
    out = bytes([len(sel)])
    for ci, td, ta in sel:
        out += bytes([comps[ci][0], td << 4 | ta])
    return seg(0xDA, out + b"\x00\x3f\x00")


# ---- entropy coding ------------------------------------------------------------------------------------------------------------
class Frame:
    """Go's view of a frame: the MCU grid (mxx, myy) from the first component's sampling, each component's (h, v) -- (1, 1) for a
    single-component frame -- and block grid (rows, cols) = (myy * v, mxx * h)"""

    def __init__(self, w, h, comps):
        self.w, self.h, self.comps = w, h, list(comps)
        self.hv = [(1, 1)] if len(comps) == 1 else [(c[1], c[2]) for c in comps]
        h0, v0 = self.hv[0]
        self.mxx, self.myy = (w + 8 * h0 - 1) // (8 * h0), (h + 8 * v0 - 1) // (8 * v0)

    def grid(self, c):
        hi, vi = self.hv[c]
        return self.myy * vi, self.mxx * hi

    def order(self, sel):
        """[(mcu index, component index, block row, block col)] in scan order, as processSOS walks them (a non-interleaved scan goes
        row by row over the component's grid and skips the blocks wholly outside the image)"""
        out = []
        if len(sel) == 1:
            c = sel[0][0]
            hi, vi = self.hv[c]
            q = self.mxx * hi
            n = 0
            for m in range(self.mxx * self.myy):
                for _ in range(hi * vi):
                    bx, by = n % q, n // q
                    n += 1
                    if bx * 8 >= self.w or by * 8 >= self.h:
                        continue
                    out.append((m, c, by, bx))
            return out
        for my in range(self.myy):
            for mx in range(self.mxx):
                for c, _, _ in sel:
                    hi, vi = self.hv[c]
                    for j in range(hi * vi):
                        out.append((my * self.mxx + mx, c, vi * my + j // hi, hi * mx + j % hi))
        return out


class BitWriter:
    def __init__(self, pad=1):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.pad = pad

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.acc = (self.acc << n) | v
        self.n += n
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(((1 << (8 - self.n)) - 1) if self.pad else 0, 8 - self.n)
        return bytes(self.out)


def block_tokens(zz, prev_dc):
    """the symbols libjpeg would write for one block (zig-zag coefficients zz): DC difference, run / size pairs with ZRL, EOB"""
    toks = [("dc", int(zz[0]) - prev_dc)]
    run = 0
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            toks.append(("sym", ZRL))
            run -= 16
        toks.append(("ac", run, int(zz[k])))
        run = 0
    if last < 63:
        toks.append(("sym", EOB))
    return toks


def emit(bw, toks, dct, act):
    for t in toks:
        if t[0] == "dc":
            s = size_of(t[1])
            c, ln = dct.code[s]
            bw.put(c, ln)
            bw.put(magnitude_bits(t[1], s), s)
        elif t[0] == "dcs":
            c, ln = dct.code[t[1]]
            bw.put(c, ln)
            bw.put(t[2], t[1])
        elif t[0] == "ac":
            s = size_of(t[2])
            assert 1 <= s <= 15 and 0 <= t[1] <= 15
            c, ln = act.code[t[1] << 4 | s]
            bw.put(c, ln)
            bw.put(magnitude_bits(t[2], s), s)
        else:
            c, ln = act.code[t[1]]
            bw.put(c, ln)


def scan(frame, sel, blocks, tables, ri=0, pad=1, tokens=None, rst_start=0):
    """the entropy-coded data of one scan, restart markers included.  tables = (dc tables by id, ac tables by id).  The DC
    prediction restarts at every restart marker, as in Go's processSOS.  tokens: {(c, by, bx): [...]} overrides; such a block's
    DC difference is the one its tokens say, and the next block's prediction follows from the coefficients given in `blocks`."""
    dcs, acs = tables
    tokens = tokens or {}
    bw = BitWriter(pad)
    out = b""
    pred = {}
    k = rst_start
    last_m = 0
    nmcu = frame.mxx * frame.myy
    td = {c: d for c, d, _ in sel}
    ta = {c: a for c, _, a in sel}

    def restarts(upto):
        """the markers due before MCU `upto` (Go expects one after every ri-th MCU but the last, blocks or not)"""
        nonlocal bw, pred, k, out, last_m
        for mm in range(last_m + 1, upto + 1):
            if ri and mm % ri == 0 and mm < nmcu:
                out += bw.flush() + bytes([0xFF, 0xD0 + (k & 7)])
                k += 1
                bw = BitWriter(pad)
                pred = {}
        last_m = max(last_m, upto)

    for m, c, by, bx in frame.order(sel):
        restarts(m)
        zz = blocks[c][by, bx]
        toks = tokens.get((c, by, bx)) or block_tokens(zz, pred.get(c, 0))
        emit(bw, toks, dcs[td[c]], acs[ta[c]])
        pred[c] = int(zz[0])
    restarts(nmcu - 1)
    return out + bw.flush()


def all_blocks(frame, rng, amp=40, ac=6, density=0.15):
    """random zig-zag blocks for every component: DC in +-amp, a few small AC values (|v| <= ac) at random positions"""
    out = []
    for c in range(len(frame.comps)):
        rows, cols = frame.grid(c)
        b = np.zeros((rows, cols, 64), np.int64)
        b[..., 0] = rng.integers(-amp, amp + 1, (rows, cols))
        mask = rng.random((rows, cols, 63)) < density
        b[..., 1:] = np.where(mask, rng.integers(-ac, ac + 1, (rows, cols, 63)), 0)
        out.append(b)
    return out
