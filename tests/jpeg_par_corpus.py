"""JPEG files engineered for the decoder that is parallel inside a scan (csrc/ipx_jpeg_dec_par.hip), written with tests/jpeg_writer.py
and the table sets of tests/jpeg_edge_corpus.py.  Every file has one baseline scan of all its components, no DRI, and (but for the ones
that say otherwise) 4 KiB of entropy-coded data or more, which is what routes it to par_count / par_unstuff / par_sync / par_write / par_dc.

  Lay                 plans a Gray scan token by token with the stuffed and the unstuffed position known as it goes, so that a byte or a
                      symbol can be put on a chosen offset; the file itself is then written by jpeg_writer.scan(tokens=...)
  trace(...)          jpeg_writer.scan restated with the unstuffed bit offset of every block (tests check it gives scan()'s bytes)
  scan_of, unstuffed  what the host plan calls the scan (up to the first marker that is neither 0xff00 nor RSTn) and what the
                      unstuff pass makes of it
  SpecModel           the passes in plain Python: speculative decode of every sub-sequence, then rounds in which each wave of 64
                      reaches its fixed point from what the wave before it left in the round before

corpus() -> [Case]; each case carries its file, the coefficients it codes, the status image.Decode has to give, and the properties it
claims (tests/test_jpeg_par_corpus.py proves them from the bytes)."""
from dataclasses import dataclass, field

import numpy as np

import jpeg_edge_corpus as je
import jpeg_writer as jw

SUBS = (128, 256, 512, 1024)
ROUTE_BYTES = 4096                      # jpeg_plan_batch: scan_len >= 4 * the largest sub-sequence goes to the parallel decoder
END = (0xFFFFFFFF, 0, 0)
GW, GH = 328, 200                       # the Gray geometry of the engineered files: 41 x 25 = 1025 blocks
G1 = [(1, 1, 1, 0)]
SHARED_SEED = 5                         # see test_jpeg_par_corpus.py::test_shared_tables_need_a_round_per_wave


@dataclass
class Case:
    name: str
    data: bytes
    w: int
    h: int
    ratio: int
    coefs: list                         # per component (rows, cols, 64) zig-zag coefficients, None where the file is not decodable
    status: int = 0                     # 0, -1 (malformed), -4 (a DC value beyond int16)
    props: dict = field(default_factory=dict)
    par: bool = True                    # the scan is long enough for the parallel route
    tables: tuple = None                # (dc tables by id, ac tables by id), sel
    sel: list = None
    scan_args: tuple = None             # (frame, sel, blocks, tables, tokens) as given to jpeg_writer.scan
    starts: list = None                 # see block_starts()


# ---- the scan as the product sees it ---------------------------------------------------------------------------------------------
def scan_of(data):
    """(offset, length) of the entropy-coded data as jpeg_parse takes it: from the end of the SOS header to the first 0xff that is
    followed by neither 0x00 nor RSTn (the last byte of the file is never looked at)"""
    i = 2
    while data[i + 1] != 0xDA:
        assert data[i] == 0xFF
        i += 2 + (data[i + 2] << 8 | data[i + 3])
    off = i + 2 + (data[i + 2] << 8 | data[i + 3])
    k = off
    while k + 1 < len(data):
        if data[k] == 0xFF and not (data[k + 1] == 0 or 0xD0 <= data[k + 1] <= 0xD7):
            return off, k - off
        k += 2 if data[k] == 0xFF else 1
    return off, len(data) - off


def unstuffed(scan):
    """the scan without its stuffed zeros, cut at its first marker (a lone 0xff at the very end counts as one): par_unstuff_kernel"""
    out = bytearray()
    k = 0
    while k < len(scan):
        c = scan[k]
        if c == 0xFF:
            if k + 1 >= len(scan) or scan[k + 1] != 0:
                break
            k += 1
        out.append(c)
        k += 1
    return bytes(out)


def stuffed_pairs(scan):
    """offsets of the 0xff of every 0xff 0x00 pair before the first marker"""
    out, k = [], 0
    while k + 1 < len(scan):
        if scan[k] == 0xFF:
            if scan[k + 1] != 0:
                break
            out.append(k)
            k += 2
        else:
            k += 1
    return out


# ---- writing with offsets ----------------------------------------------------------------------------------------------------------
class CountingWriter(jw.BitWriter):
    def __init__(self, pad=1):
        super().__init__(pad)
        self.ubits = 0

    def put(self, v, n):
        self.ubits += n
        super().put(v, n)

    def sbits(self):
        """the stuffed position in bits"""
        return len(self.out) * 8 + self.n


def trace(frame, sel, blocks, tables, tokens=None, pad=1):
    """jpeg_writer.scan for a scan without restart intervals -> (bytes, unstuffed bit offset of every block + the end of the last)"""
    dcs, acs = tables
    tokens = tokens or {}
    bw = CountingWriter(pad)
    pred, starts = {}, []
    td = {c: d for c, d, _ in sel}
    ta = {c: a for c, _, a in sel}
    for m, c, by, bx in frame.order(sel):
        starts.append(bw.ubits)
        zz = blocks[c][by, bx]
        toks = tokens.get((c, by, bx)) or jw.block_tokens(zz, pred.get(c, 0))
        jw.emit(bw, toks, dcs[td[c]], acs[ta[c]])
        pred[c] = int(zz[0])
    starts.append(bw.ubits)
    n = bw.ubits
    out = bw.flush()
    bw.ubits = n
    return out, starts


def block_starts(case):
    """the writer's unstuffed bit offset of every block of a case, and of the end of the last one"""
    if case.starts is None:
        _, case.starts = trace(*case.scan_args)
    return case.starts


def coefs_of(toks, prev_dc):
    """the zig-zag coefficients a token list codes, as Go reads it"""
    zz = np.zeros(64, np.int64)
    zig = 1
    for t in toks:
        if t[0] == "dc":
            zz[0] = prev_dc + t[1]
        elif t[0] == "dcs":
            v = t[2]
            if t[1] and v < 1 << (t[1] - 1):
                v += (-1 << t[1]) + 1
            zz[0] = prev_dc + v
        elif t[0] == "ac":
            zig += t[1]
            assert zig <= 63
            zz[zig] = t[2]
            zig += 1
        elif t[1] == jw.ZRL:
            zig += 16
        elif t[1] & 15:
            zig += t[1] >> 4                # a run that passes zig 63: nothing is stored, no bits are read
            assert zig > 63
        else:
            break
    return zz


def token_bits(toks, dct, act):
    n = 0
    for t in toks:
        if t[0] == "dc":
            s = jw.size_of(t[1])
            n += dct.code[s][1] + s
        elif t[0] == "dcs":
            n += dct.code[t[1]][1] + t[1]
        elif t[0] == "ac":
            s = jw.size_of(t[2])
            n += act.code[t[1] << 4 | s][1] + s
        else:
            n += act.code[t[1]][1]
    return n


class Lay:
    """A Gray scan planned block by block.  fill() pads with blocks of two filler tokens whose lengths are coprime and which never
    make a 0xff byte, up to a chosen position (stuffed or unstuffed bits); block() lays a block of given tokens."""

    def __init__(self, dct, act, fillers):
        self.dct, self.act = dct, act
        self.bw = CountingWriter(1)
        self.toks = []                  # per block
        self.dc = 0
        self.zz = []
        self.starts = []
        self.f = [(t, token_bits([t], dct, act), 1 + t[1]) for t in fillers]      # (token, bits, zig positions)
        self.base = token_bits([("dc", 0), ("sym", jw.EOB)], dct, act)
        # extras (bits beyond an empty block) a block of fillers can have, and how
        self.how = {}
        (t1, l1, z1), (t2, l2, z2) = self.f
        for a in range(63):
            for b in range(63):
                if a * z1 + b * z2 <= 62:
                    self.how.setdefault(a * l1 + b * l2, (a, b))
        self.emax = max(e for e in self.how if all(x in self.how for x in range(e - 100, e)))
        self.dense = next(e for e in sorted(self.how) if all(x in self.how for x in range(e, self.emax)))   # every extra in [dense, emax] works

    def block(self, toks):
        self.starts.append(self.bw.ubits)
        jw.emit(self.bw, toks, self.dct, self.act)
        zz = coefs_of(toks, self.dc)
        self.dc = int(zz[0])
        self.toks.append(list(toks))
        self.zz.append(zz)

    def filler(self, extra):
        a, b = self.how[extra]
        toks = [("dc", 0)]
        # the two kinds interleaved, so that long blocks are not one token repeated
        ka, kb = a, b
        while ka or kb:
            if ka:
                toks.append(self.f[0][0])
                ka -= 1
            if kb:
                toks.append(self.f[1][0])
                kb -= 1
        before = len(self.bw.out), self.bw.ubits
        self.block(toks + [("sym", jw.EOB)])
        # fillers add no stuffing: as many new stuffed bytes as unstuffed ones (to the byte the writer has completed)
        assert (len(self.bw.out) - before[0]) == (self.bw.ubits // 8 - before[1] // 8), "a filler made a 0xff"

    def can(self, e, k):
        """e bits of extra can be split over k filler blocks"""
        if e > k * self.emax:
            return False
        return e in self.how or e >= self.dense + (k > 1) * self.dense or (k > 1 and any(e - a in self.how for a in self.how if a <= e and a < self.dense))

    def pos(self, stuffed):
        return self.bw.sbits() if stuffed else self.bw.ubits

    def fill(self, target, stuffed=False, m=None):
        """filler blocks up to bit `target` exactly (a block boundary), m of them if given"""
        r = target - self.pos(stuffed)
        if m is None:
            assert r >= self.base, (target, r)
            m = r // (self.base + self.emax) + 1
            if r - m * self.base < self.dense and r - m * self.base not in self.how:
                m += 1
        e = r - m * self.base
        assert 0 <= e <= m * self.emax, (r, m, e)
        for left in range(m, 0, -1):
            # spread evenly: the extra nearest the mean that leaves the blocks behind it a sum they can have
            x = e if left == 1 else next(a for d in range(self.emax) for a in (min(self.emax, -(-e // left)) + d, min(self.emax, -(-e // left)) - d)
                                         if a in self.how and a <= e and self.can(e - a, left - 1))
            assert x in self.how, (e, x)
            self.filler(x)
            e -= x
        assert e == 0 and self.pos(stuffed) == target

    def tokens(self, cols):
        return {(0, k // cols, k % cols): t for k, t in enumerate(self.toks)}

    def blocks(self, rows, cols):
        z = np.stack(self.zz)
        return [z[:rows * cols].reshape(rows, cols, 64)]


def complete_lay():
    """under tables_complete: DC size 0 is 0000, EOB 0000000, ZRL 0000001, symbol 0xff (run 15, size 15) is the byte 0xff"""
    dct, act = je.tables_complete()
    return Lay(dct, act, [("ac", 0, 1), ("ac", 0, 4)])                   # 7 + 1 and 8 + 3 bits


def short_lay():
    """under tables_short with 17 DC sizes: DC size 0 and EOB take 2 bits, size 16 a 16-bit code; AC size 15 a 16-bit code"""
    _, act, dct = je.tables_short()
    return Lay(dct, act, [("ac", 0, 1), ("ac", 1, 1)])                   # 4 + 1 and 5 + 1 bits


Q2 = {0: (je.flat_q(2), 0)}
ROWS, COLS = GH // 8, GW // 8
NB = ROWS * COLS


def gray_case(name, lay, props, total_bytes=None, nblocks=NB, status=0, par=True, tail=b"", extra_blocks=0):
    """finishes a planned scan with filler blocks to nblocks + extra_blocks and, if given, to a stuffed length of total_bytes"""
    left = nblocks + extra_blocks - len(lay.toks)
    assert left >= 1, (name, left)
    if total_bytes is None:
        lay.fill(lay.bw.sbits() + left * lay.base, stuffed=True, m=left)
    else:
        lay.fill(total_bytes * 8, stuffed=True, m=left)
    return gray_from_tokens(name, lay, lay.toks, props, status=status, par=par, tail=tail, nblocks=nblocks)


def gray_from_tokens(name, lay, toks, props, status=0, par=True, tail=b"", nblocks=NB):
    fr = jw.Frame(GW, GH, G1)
    # the frame's blocks by the writer's token override; blocks beyond the frame are written behind the scan by hand below
    zz, dc = [], 0
    for t in toks:
        zz.append(coefs_of(t, dc))
        dc = int(zz[-1][0])
    blocks = [np.stack(zz[:nblocks]).reshape(ROWS, COLS, 64)]
    tokens = {(0, k // COLS, k % COLS): t for k, t in enumerate(toks[:nblocks])}
    tables = {(0, 0): lay.dct, (1, 0): lay.act}
    args = (fr, [(0, 0, 0)], blocks, ({0: lay.dct}, {0: lay.act}), tokens)
    data = je.file(GW, GH, G1, blocks, tables, Q2, tokens=tokens, tail=tail)
    if len(toks) > nblocks:
        # more coded blocks than the frame has: the scan of a taller frame under this frame's header
        rows2 = -(-len(toks) // COLS)
        toks = toks + [[("dc", 0), ("sym", jw.EOB)]] * (rows2 * COLS - len(toks))
        args = (jw.Frame(GW, rows2 * 8, G1), [(0, 0, 0)], [np.zeros((rows2, COLS, 64), np.int64)], args[3],
                {(0, k // COLS, k % COLS): t for k, t in enumerate(toks)})
        off, n = scan_of(data)
        data = data[:off] + jw.scan(*args[:4], tokens=args[4]) + tail + jw.eoi()
    return Case(name, data, GW, GH, 4, blocks, status, props, par, args[3], [(0, 0, 0)], args)


# ---- unstuffing ------------------------------------------------------------------------------------------------------------------------
# 0xff bytes of pairs, by stuffed offset: the last byte of a sub-sequence at every size (3071, 8191 = the last of the first wave at
# 128, 16383 = at 256), the last of sub-sequence 64 at 128 and at 256 (8319, 16639), and inside a sub-sequence astride a 4-byte word
# (3091) and a 16-byte group (3135)
PAIRS_AT = (3071, 3091, 3135, 8191, 8319, 16383, 16639)


def pairs_case():
    lay = complete_lay()
    for p in PAIRS_AT:
        lay.fill(p * 8 - 4, stuffed=True)
        lay.block([("dc", 0), ("ac", 15, -21846), ("sym", jw.EOB)])        # 0000 11111111 then 010101010101001
    return gray_case("unstuff_pairs", lay, {"pairs_at": PAIRS_AT})


def dense_case(seed=2):
    """runs of all-ones magnitudes: about every other byte of 9 KiB is 0xff (the seed: test_jpeg_par_corpus.py asserts the residues)"""
    rng = np.random.default_rng(seed)
    lay = complete_lay()
    while lay.bw.sbits() < 9000 * 8:
        toks = [("dc", 0)]
        for _ in range(63):
            s = int(rng.choice([15, 14, 13, 11, 9, 15, 15]))
            toks.append(("ac", 0, (1 << s) - 1))
        lay.block(toks)                                                    # zig 63 reached: no EOB
    return gray_case("unstuff_dense", lay, {"dense": True})


LENGTHS = (4096, 4097, 8064, 8191, 8192, 8193, 16383, 16384, 16385)       # 8064 = 63 * 128; 64, 65, 128, 129 sub-sequences of 128 follow


def length_cases():
    """the scan's stuffed length on and around multiples of every sub-sequence size and the routing threshold.  4095, 4096 and 4097
    code the same coefficients: the last block carries 0, 1 or 2 ZRLs before its EOB (7 bits each), so the three give equal planes"""
    out = []
    lay = complete_lay()
    lay.fill(700 * 8 - 4, stuffed=True)
    lay.block([("dc", 0), ("ac", 15, 20000), ("sym", jw.EOB)])                # one pair early on, so that the lengths are stuffed lengths
    left = NB - len(lay.toks)
    lay.fill(4095 * 8 - lay.base, stuffed=True, m=left - 1)
    lay.block([("dc", 0), ("sym", jw.EOB)])                                # ends on the last bit of byte 4095
    assert lay.bw.sbits() == 4095 * 8
    for k in range(3):
        toks = lay.toks[:-1] + [[("dc", 0)] + [("sym", jw.ZRL)] * k + [("sym", jw.EOB)]]
        out.append(gray_from_tokens("len_%d" % (4095 + k), lay, toks, {"scan_len": 4095 + k, "trio": True}, par=k > 0))
    for n in LENGTHS[2:]:
        lay = complete_lay()
        lay.fill(n * 8 - 64 * 8 - 4, stuffed=True, m=NB - 21)
        lay.block([("dc", 0), ("ac", 15, -17000), ("sym", jw.EOB)])         # and a pair 64 bytes before the end
        out.append(gray_case("len_%d" % n, lay, {"scan_len": n}, total_bytes=n))
    return out


def noise(rng, n, pairs):
    """n bytes without markers: values below 0xff with 0xff 0x00 pairs sprinkled in"""
    b = bytearray(rng.integers(0, 255, n, dtype=np.uint8).tobytes())
    for k in rng.choice(n // 2 - 1, pairs, replace=False):
        b[2 * k], b[2 * k + 1] = 0xFF, 0x00
    return bytes(b)


def tail_and_cut_cases(seed=2):
    rng = np.random.default_rng(seed)
    out = []

    def body():
        lay = complete_lay()
        lay.fill(2047 * 8 - 4, stuffed=True)
        lay.block([("dc", 0), ("ac", 15, -30000), ("sym", jw.EOB)])
        return lay
    base = gray_case("tail_none", body(), {"scan_len": 6000}, total_bytes=6000)
    out.append(base)
    off, n = scan_of(base.data)
    assert n == 6000
    junk = noise(rng, 1500, 200)
    # bytes behind EOI: Go never reads them, and the host plan cuts the scan at the marker
    out.append(Case("tail_after_eoi", base.data + junk, GW, GH, 4, base.coefs, 0, {"scan_len": 6000, "after_eoi": len(junk)},
                    True, base.tables, base.sel, base.scan_args))
    # bytes between the scan and EOI behind an RSTn: a file without DRI keeps RSTn inside what the plan calls the scan, so these
    # bytes reach the kernels, which have to stop at the marker; Go's marker loop skips RSTn and the bytes that follow
    d = base.data[:off + n] + b"\xff\xd0" + junk + jw.eoi()
    out.append(Case("tail_behind_rst", d, GW, GH, 4, base.coefs, 0, {"scan_len": 6000 + 2 + len(junk), "marker_at": 6000},
                    True, base.tables, base.sel, base.scan_args))
    # entropy-coded noise straight behind the last block: part of the scan for every decoder, never reached by Go
    d = base.data[:off + n] + junk + jw.eoi()
    out.append(Case("tail_noise_in_scan", d, GW, GH, 4, base.coefs, 0, {"scan_len": 6000 + len(junk)}, True, base.tables, base.sel,
                    base.scan_args))
    # cut on the 0xff of the pair at 2047 (no EOI: the host refuses the file), the same with EOI behind it (the parser takes the 0xff
    # for a fill byte: the scan ends one byte earlier, short of its blocks), and cut inside a symbol with EOI behind it
    lay = body()
    big = gray_case("cut_source", lay, {}, total_bytes=9000)
    off, n = scan_of(big.data)
    pair = 2047
    assert big.data[off + pair] == 0xFF
    out.append(Case("cut_on_ff_no_eoi", big.data[:off + pair + 1], GW, GH, 4, None, -1, {"cut": pair + 1, "host_verdict": True}, False))
    lay2 = complete_lay()
    lay2.fill(5000 * 8 - 4, stuffed=True)
    lay2.block([("dc", 0), ("ac", 15, -30000), ("sym", jw.EOB)])
    big2 = gray_case("cut_source2", lay2, {}, total_bytes=9000)
    off, n = scan_of(big2.data)
    assert big2.data[off + 5000] == 0xFF
    out.append(Case("cut_on_ff", big2.data[:off + 5001] + jw.eoi(), GW, GH, 4, None, -1, {"scan_len": 5000, "cut": 5000}, True))
    out.append(Case("cut_mid_symbol", big2.data[:off + 5003] + jw.eoi(), GW, GH, 4, None, -1, {"scan_len": 5003, "cut": 5003}, True))
    return out


# ---- synchronisation ---------------------------------------------------------------------------------------------------------------------
AC15 = ("ac", 0, 21845)                 # a 16-bit code and 101010101010101
DC16 = ("dcs", 16, 0x7FFF)              # a 16-bit code and sixteen bits: the difference -32768, the only one of size 16 within int16
# (unstuffed byte offset of a boundary, the symbol laid across it, the symbol's bit that sits on the boundary): boundaries of every
# size at 4096 .. 7168, of 128 alone at 3200 .. 3456; 8192 and 16384 end the first wave at 128 and 256, 8208 and 16400 end its
# staged window (64 rows + 16 bytes), where the reader changes from LDS to global words
STRADDLES = ((3200, "ac15", 8), (3328, "ac15", 24), (3456, "dc16", 8), (3584, "dc16", 24),
             (4096, "ac15", 24), (5120, "dc16", 24), (6144, "ac15", 8), (7168, "dc16", 8),
             (8192, "dc16", 24), (8208, "ac15", 24), (16384, "ac15", 8), (16400, "dc16", 8))
LONG_BLOCK_AT = 12288                   # unstuffed byte: a block of 63 size-15 coefficients (244 bytes) starts just before it


def sync_edges_case():
    lay = short_lay()
    plan = sorted(STRADDLES + ((LONG_BLOCK_AT, "long", 10),))
    for at, kind, bit in plan:
        if kind == "long":
            lay.fill(at * 8 - bit)
            lay.block([("dc", 0)] + [AC15] * 63)
            continue
        # the block's DC symbol comes first: 2 bits for size 0, so an AC symbol starts 2 bits into its block
        if kind == "ac15":
            lay.fill(at * 8 - bit - 2)
            lay.block([("dc", 0), AC15, ("sym", jw.EOB)])
        else:
            lay.fill(at * 8 - bit)
            assert lay.dc == 0
            lay.block([DC16, ("sym", jw.EOB)])
            lay.block([("dc", 32767), ("sym", jw.EOB)])
            lay.block([("dc", 1), ("sym", jw.EOB)])
    return gray_case("sync_straddles", lay, {"straddles": STRADDLES, "long_block_at": LONG_BLOCK_AT})


def sync_symbols_case():
    """ZRL runs to and before zig 63, runs that pass zig 63 (no magnitude bits follow), EOB straight after the DC -- the symbol
    choices of jpeg_edge_corpus.py, over 6 KiB"""
    lay = short_lay()
    specs = [
        [("ac", 0, 5), ("sym", 0xF0), ("sym", 0xF0), ("sym", 0x00)],
        [("ac", 15, 3), ("ac", 15, -2), ("ac", 14, 7), ("sym", 0xF0)],
        [("sym", 0xF0), ("sym", 0xF0), ("ac", 14, -9), ("ac", 0, 4), ("ac", 14, 6)],
        [("ac", 3, 2), ("ac", 15, 1), ("ac", 15, 1), ("ac", 15, 1), ("sym", 13 << 4 | 1)],
        [("sym", 0x00)],
        [("sym", 0xF0), ("sym", 0xF0), ("sym", 0xF0), ("sym", 15 << 4 | 3)],
    ]
    k = 0
    while lay.bw.ubits < 6000 * 8:
        lay.block([("dc", (k % 7) - 3)] + specs[k % len(specs)])
        k += 1
    return gray_case("sync_symbols", lay, {"zrl": True, "run_past_63": True})


def extra_blocks_case():
    """300 coded blocks more than the frame has, all of them long: CoefSink::end_block stops the lane that reaches the last block of
    the frame, and the lanes behind it start at g >= nblk"""
    lay = complete_lay()
    lay.fill(5000 * 8, stuffed=True, m=NB - 1)
    lay.block([("dc", 5), ("ac", 0, -7), ("sym", jw.EOB)])
    for k in range(299):
        lay.block([("dc", 1 - 2 * (k & 1))] + [("ac", 0, 100 + k)] * 20 + [("sym", jw.EOB)])
    return gray_case("sync_extra_blocks", lay, {"extra_blocks": 300}, extra_blocks=300)


T444 = (328, 256)                       # 41 x 32 MCUs of three blocks


def shared_tables_case(seed=SHARED_SEED, shared=True, w=T444[0], h=T444[1]):
    """4:4:4 with one DC and one AC table for the three components: a decoder in step with the symbols still does not know which block
    of the MCU it is in, so the block-in-MCU index of a speculative exit is right by luck only"""
    rng = np.random.default_rng(seed)
    c3 = je.comps3(1, 1)
    fr = jw.Frame(w, h, c3)
    dc_s, ac_s, _ = je.tables_short()
    bl = je.limit(jw.all_blocks(fr, rng, amp=40, ac=6, density=0.12))
    sel = [(c, 0, 0) for c in range(3)] if shared else None
    dc_l, ac_l = je.tables_long()
    tabs = {(0, 0): dc_s, (1, 0): ac_s} if shared else {(0, 0): dc_s, (1, 0): ac_s, (0, 1): dc_l, (1, 1): ac_l}
    q = {0: (je.flat_q(3), 0), 1: (je.flat_q(5), 0)}
    data = je.file(w, h, c3, bl, tabs, q, sel=sel)
    sel = sel or [(0, 0, 0), (1, 1, 1), (2, 1, 1)]
    tables = ({0: dc_s, 1: dc_s if shared else dc_l}, {0: ac_s, 1: ac_s if shared else ac_l})
    return Case("shared_tables_444" if shared else "own_tables_444", data, w, h, 0, bl, 0, {"shared_tables": shared}, True, tables, sel, (fr, sel, bl, tables, None))


# ---- the DC pass -------------------------------------------------------------------------------------------------------------------------
MCU_GRIDS = {1023: (33, 31), 1024: (32, 32), 1025: (41, 25), 2047: (89, 23), 2048: (64, 32), 2049: (683, 3)}
SAMPLINGS = {1: None, 3: (1, 1), 4: (2, 1), 6: (2, 2)}       # blocks per MCU -> the first component's sampling factors (4: 4:2:2)


def comps_of(bpm):
    return G1 if bpm == 1 else je.comps3(*SAMPLINGS[bpm])


def dc_tile_cases(seed=3):
    """MCU counts on and around par_dc_kernel's tiles of 1024, for 1, 3, 4 and 6 blocks per MCU; DC differences large enough for the
    running values to roam over a few thousand, sparse AC so that the scans stay at a few tens of KiB"""
    rng = np.random.default_rng(seed)
    dc_s, ac_s, _ = je.tables_short()
    std = {(0, 0): dc_s, (1, 0): ac_s, (0, 1): dc_s, (1, 1): ac_s}
    q = {0: (je.flat_q(1), 0), 1: (je.flat_q(2), 0)}
    out = []
    for bpm in SAMPLINGS:
        comps = comps_of(bpm)
        h0, v0 = (1, 1) if bpm == 1 else SAMPLINGS[bpm]
        for nmcu, (mx, my) in MCU_GRIDS.items():
            w, h = mx * 8 * h0 - 3, my * 8 * v0 - 5              # ragged: the last MCU column and row are partial
            fr = jw.Frame(w, h, comps)
            assert fr.mxx * fr.myy == nmcu
            dens = min(0.12, 0.12 * 1500 / (nmcu * bpm))
            bl = je.limit(jw.all_blocks(fr, rng, amp=900, ac=5, density=max(dens, 0.05 if bpm == 1 else 0.0)))
            c = je.case("dc_tile_%d_bpm%d" % (nmcu, bpm), w, h, comps, bl, std, q, set())
            sel = [(k, min(k, 1), min(k, 1)) for k in range(len(comps))]
            tables = ({0: dc_s, 1: dc_s}, {0: ac_s, 1: ac_s})
            out.append(Case(c.name, c.data, w, h, c.ratio, bl, 0, {"nmcu": nmcu, "bpm": bpm}, True, tables, sel, (fr, sel, bl, tables, None)))
    return out


DC_LIMIT_GRID = 2048                    # MCUs of the DC-limit files: two tiles


def dc_limit_cases():
    """running DC values that reach exactly 32767 and -32768 in MCUs of the second tile (accepted), and that go one step past either
    (a DC value beyond int16: IPX_ERR_UNSUPPORTED); every DIFFERENCE stays within int16, the one of size 16 (-32768) included.  Gray,
    and 4:4:4 where the second and the third component carry the values; the first excursion peaks in MCU 1024, the first of the
    second tile"""
    _, ac_s, dc17 = je.tables_short()
    std = {(0, 0): dc17, (1, 0): ac_s, (0, 1): dc17, (1, 1): ac_s}
    q = {0: (je.flat_q(1), 0), 1: (je.flat_q(1), 0)}
    out = []
    mx, my = MCU_GRIDS[DC_LIMIT_GRID]
    for bpm in (1, 3):
        comps = comps_of(bpm)
        w, h = mx * 8, my * 8
        fr = jw.Frame(w, h, comps)
        for nm, hi, lo, status in (("reach", 32767, -32768, 0), ("past_hi", 32768, -32768, -4), ("past_lo", 32767, -32769, -4)):
            rng = np.random.default_rng(7)
            bl = je.limit(jw.all_blocks(fr, rng, amp=300, ac=5, density=0.08))
            peaks = {}
            for c in range(len(comps)):
                if bpm == 3 and c == 0:
                    continue
                flat = bl[c].reshape(-1, 64)                    # Gray and 4:4:4: block k of a component belongs to MCU k
                m0 = 1023 + 300 * (c % 2)
                # ... 0, 16000, hi, 0, -16000, lo, -16000, 0 ...: steps of at most 32768 downwards and 32767 upwards
                for k, v in enumerate((0, 16000, hi, 0, -16000, lo, -16000, 0)):
                    flat[m0 - 1 + k, 0] = v
                peaks[c] = (m0 + 1, m0 + 4)
            c0 = je.case("dc_%s_bpm%d" % (nm, bpm), w, h, comps, bl, std, q, set())
            sel = [(k, min(k, 1), min(k, 1)) for k in range(len(comps))]
            tables = ({0: dc17, 1: dc17}, {0: ac_s, 1: ac_s})
            out.append(Case(c0.name, c0.data, w, h, c0.ratio, bl, status, {"dc_hi": hi, "dc_lo": lo, "bpm": bpm, "peaks": peaks},
                            True, tables, sel, (fr, sel, bl, tables, None)))
    return out


def dc_wide_step_case():
    """NOT part of corpus(): the running DC value goes from 32767 straight to -32768 in the second tile, a difference of -65535 (size
    16) between values that both fit.  Go and the piece kernels decode it; the in-scan route keeps DC differences in int16 and hands the
    file back"""
    _, ac_s, dc17 = je.tables_short()
    mx, my = MCU_GRIDS[DC_LIMIT_GRID]
    fr = jw.Frame(mx * 8, my * 8, G1)
    bl = je.limit(jw.all_blocks(fr, np.random.default_rng(1), amp=300, ac=5, density=0.08))
    flat = bl[0].reshape(-1, 64)
    for k, v in enumerate((0, 16000, 32767, -32768, -16000, 0)):
        flat[1500 + k, 0] = v
    data = je.file(mx * 8, my * 8, G1, bl, {(0, 0): dc17, (1, 0): ac_s}, {0: (je.flat_q(1), 0)})
    tables = ({0: dc17}, {0: ac_s})
    return Case("dc_wide_step", data, mx * 8, my * 8, 4, bl, 0, {"dc_step": -65535}, True, tables, [(0, 0, 0)], (fr, [(0, 0, 0)], bl, tables, None))


_CORPUS = None


def corpus():
    """built once per process: the tests share it and leave it unchanged"""
    global _CORPUS
    if _CORPUS is None:
        out = [pairs_case(), dense_case()] + length_cases() + [c for c in tail_and_cut_cases() if not c.name.startswith("cut_source")]
        out += [sync_edges_case(), sync_symbols_case(), extra_blocks_case(), shared_tables_case(), shared_tables_case(shared=False)]
        out += dc_tile_cases() + dc_limit_cases()
        _CORPUS = out
    return _CORPUS


# ---- the passes in plain Python ----------------------------------------------------------------------------------------------------------
def _lut(h):
    """16-bit window -> code length << 8 | symbol, -1 where no code matches"""
    t = np.full(65536, -1, np.int32)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(h.counts[ln - 1]):
            lo = code << (16 - ln)
            t[lo:lo + (1 << (16 - ln))] = ln << 8 | h.vals[k]
            code += 1
            k += 1
        code <<= 1
    return t.tolist()


class SpecModel:
    """run() of ipx_jpeg_dec_par.hip and the rounds of par_sync_kernel restated.  A state is (unstuffed bit position, block in MCU,
    next zig-zag index; 0 = DC expected); END when the data is used up."""

    def __init__(self, case, sub):
        off, n = scan_of(case.data)
        self.u = unstuffed(case.data[off:off + n])
        self.ubits = len(self.u) * 8
        self.pad = self.u + bytes(8)
        self.sub = sub
        self.nsub = -(-n // sub)                                  # by the STUFFED length, as jpeg_plan_batch counts them
        ncomp = 1 if case.ratio == 4 else 3
        hv = {4: (1, 1), 0: (1, 1), 1: (2, 1), 2: (2, 2), 3: (1, 2)}[case.ratio]
        self.ybl = hv[0] * hv[1]
        self.bpm = self.ybl + (2 if ncomp == 3 else 0)
        dcs, acs = case.tables
        luts = {}
        self.dc = [luts.setdefault(id(dcs[d]), _lut(dcs[d])) for _, d, _ in case.sel]
        self.ac = [luts.setdefault(id(acs[a]), _lut(acs[a])) for _, _, a in case.sel]

    def peek32(self, p):
        b = p >> 3
        return (int.from_bytes(self.pad[b:b + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF

    def run(self, p, c, z, uend):
        """-> (exit state, blocks ended)"""
        ends = 0
        ubits, bpm, ybl = self.ubits, self.bpm, self.ybl
        while True:
            if p >= uend:
                return (END if p >= ubits else (p, c, z)), ends
            dcs = z == 0
            comp = 0 if c < ybl else c - ybl + 1
            bits = self.peek32(p) if p < ubits else 0
            e = (self.dc if dcs else self.ac)[comp][bits >> 16]
            if e < 0:
                p += 1                                             # no such code: one bit on, the state as it is
                if p > ubits:
                    return END, ends
                continue
            ln, sym = e >> 8, e & 255
            run_, sz = sym >> 4, sym & 15
            if dcs:
                nbits = sym if sym <= 16 else 0
            else:
                nbits = sz if sz and z + run_ <= 63 else 0
            p += ln + nbits
            if p > ubits:
                return END, ends
            if dcs:
                if sym <= 16:
                    z = 1
                continue
            zz = z + (run_ if sz else (16 if run_ == 15 else 64))
            z = zz + (1 if sz else 0)
            if z > 63:
                ends += 1
                c = 0 if c + 1 == bpm else c + 1
                z = 0

    def decode(self, entry, t):
        p = entry[0]
        uend = min((t + 1) * self.sub * 8, self.ubits)
        if entry == END or p >= uend:
            return (END if p >= self.ubits else entry), 0
        return self.run(p, entry[1], entry[2], uend)

    def solve(self):
        """-> the number of rounds that change an entry; leaves entry, exit and ends per sub-sequence"""
        n, sub = self.nsub, self.sub
        self.entry = [(t * sub * 8, 0, 0) if t * sub * 8 < self.ubits else END for t in range(n)]
        self.wrong_exits = None
        res = [self.decode(self.entry[t], t) for t in range(n)]
        self.exit, self.ends = [r[0] for r in res], [r[1] for r in res]
        self.spec_exit = list(self.exit)
        rounds = 0
        while True:
            prev = list(self.exit)
            changed = 0
            for w0 in range(0, n, 64):
                for t in range(max(w0, 1), min(w0 + 64, n)):
                    want = prev[t - 1] if t == w0 else self.exit[t - 1]
                    if want != self.entry[t]:
                        self.entry[t] = want
                        self.exit[t], self.ends[t] = self.decode(want, t)
                        changed += 1
            if not changed:
                return rounds
            rounds += 1
