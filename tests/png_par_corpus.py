"""PNG files for the parallel inflate (csrc/ipx_png_dec_par.hip, IPX_PNG_PAR=1): streams written with tests/deflate_writer.py, token
by token and code length by code length, and with zlib, aimed at that kernel's own edges -- sub-sequence boundaries inside every part
of a token, end-of-block symbols at and beside a boundary, blocks shorter than a sub-sequence, codes on which a speculative lane never
falls into step, sub-sequences whose output alone exceeds a flush unit, rounds that end at, below and above the unit, matches over
literals of the same round, a distance of 32768 into bytes flushed rounds before -- and damaged twins.  tests/png_par_model.py says
which edge a stream reaches (tests/test_png_par_corpus.py asserts it).

Frames are small: raw lengths from a few bytes to about 100 KB.  A stream laid down token by token is wrapped as a file of one row
(filter byte 0 first), so the tokens need not know about rows.

corpus() -> [Case]; a Case carries the file, its zlib stream, the filtered bytes (clean files), what it aims at (`tags`) and, for a
damaged twin, `damage`.

corpus(edges=True) has, behind those clean files, the cases of EDGE_TAGS, which run at the sizes EDGE_SUBS: a literal that a 32 KiB ring
would put on a byte a match of its round still reads, output byte 65536 (the 64 KiB ring's slot 0) crossed by matches, literals and a
stored block, a round that fills the match list, matches over matches of their round, 48-bit tokens at every bit of a word.
trailing_twins(): every clean file with a byte (three: with an IDAT chunk) behind its Adler-32, which only a serial walk of the whole
stream answers rightly.  mixed_launch(): files of one frame size that take very different paths, for one launch."""
import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

import deflate_writer as dw
import png_adam7_corpus as a7
import png_corpus as pc
import png_decode_model as dm
import png_edge_corpus as ec
import png_par_model as pm

SUBS = (pm.SUB_DEFAULT, 48, 509)       # the default, the smallest, one that is no multiple of 8
EDGE_SUBS = (pm.SUB_DEFAULT, pm.SUB_MIN, 254, pm.SUB_MAX)      # the edge cases' sizes: 254 fills the match list, 1000 the staging
EDGE_TAGS = ("alias", "wrap", "wrap-stored", "list", "chain", "long-token")
RING = 65536                           # the kernel's window ring: output byte 65536 lands on slot 0
EIGHT_BIT = [8] * 255 + [9, 9] + [0] * 29          # 255 literals of 8 bits; literal 255 and the end-of-block symbol at 9


@dataclass
class Case:
    name: str
    data: bytes
    stream: bytes
    raw: bytes = b""
    tags: tuple = ()
    damage: str = ""          # "" for a clean file
    adam7: bool = False


def one_row(n):
    """(w, ctype) of an 8-bit file of one row whose filtered bytes are n long"""
    for ctype, ch in ((0, 1), (4, 2), (2, 3), (6, 4)):
        if (n - 1) % ch == 0 and 0 < (n - 1) // ch <= 65535:
            return (n - 1) // ch, ctype
    raise AssertionError("no one-row file of %d bytes" % n)


def row_case(name, blocks, tags=(), length=None):
    """the one-row file of these blocks (the first byte they write must be 0: filter None); literals are added in a last fixed block
    until a row of that length exists, or, with `length`, up to a raw length of exactly that (a one-row file of it must exist)"""
    raw = b""
    for b in blocks:
        raw += bytes(b["data"]) if b["kind"] == "stored" else b["tokens"].expand(raw)
    assert raw[0] == 0
    if length is not None:
        assert len(raw) <= length, (name, len(raw), length)
        w, ctype = one_row(length)
        if length > len(raw):
            tail = bytes((11 * k + 1) % 256 for k in range(length - len(raw)))
            blocks = blocks + [{"kind": "fixed", "tokens": dw.literals(tail)}]
            raw += tail
        c = ec.case(name, raw, w, 1, ctype, 8, blocks)
        return Case(name, c.data, c.stream, raw, tuple(tags))
    pad = 0
    while True:
        try:
            w, ctype = one_row(len(raw) + pad)
            break
        except AssertionError:
            pad += 1
    if pad:
        blocks = blocks + [{"kind": "fixed", "tokens": dw.literals(bytes(range(1, pad + 1)))}]
        raw += bytes(range(1, pad + 1))
    c = ec.case(name, raw, w, 1, ctype, 8, blocks)
    return Case(name, c.data, c.stream, raw, tuple(tags))


def toks(items):
    """Tokens of [(literal byte,) or (length, distance)]"""
    lit = [t[0] if len(t) == 1 else 0 for t in items]
    length = [0 if len(t) == 1 else t[0] for t in items]
    dist = [0 if len(t) == 1 else t[1] for t in items]
    return dw.Tokens(lit, length, dist)


def lits(values):
    return [(int(v),) for v in values]


def shifter(offset, first=0):
    """a fixed block of literals behind a byte-aligned point that leaves the next header at bit `offset` of its byte: 3 + 8 a + 9 b + 7
    bits (ec.stored_case's trick)"""
    for b in range(8):
        if (2 + b) % 8 == offset:
            return {"kind": "fixed", "tokens": toks(lits([first, 1] + [200] * b))}


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def split_parts(seed):
    """matches with extra bits on length and distance, so that boundaries fall inside each of a token's four parts"""
    rng = np.random.default_rng(seed)
    items, n = lits([0] + rng.integers(0, 256, 300).tolist()), 301
    for _ in range(1500):
        if rng.random() < 0.3:
            k = int(rng.integers(1, 4))
            items += lits(rng.integers(0, 256, k).tolist())
            n += k
        length = int(rng.integers(11, 60))
        items.append((length, int(rng.integers(5, min(n, 32768)))))
        n += length
    return row_case("boundaries inside every part of a token", [ec.dynamic(toks(items))], ("parts",))


def eob_cases():
    """one fixed block of literals whose end-of-block symbol ends k sub-sequences and -1, 0, +1 bits behind the block's first token"""
    out = []
    for sub in SUBS:
        for delta in (-1, 0, 1):
            want = 3 * sub + delta - 7                       # bits of literals: 8 a + 9 b
            b = next(b for b in range(8) if (want - 9 * b) % 8 == 0)
            a = (want - 9 * b) // 8
            items = lits([0] + [(7 * k) % 144 for k in range(a - 1)] + [150 + k for k in range(b)])
            out.append(row_case("EOB ends %+d bits from a boundary of %d" % (delta, sub), [{"kind": "fixed", "tokens": toks(items)}],
                                ("eob", sub, delta)))
    return out


def short_block(length=None):
    return row_case("a block shorter than one sub-sequence", [{"kind": "fixed", "tokens": toks(lits([0, 7, 9]))}], ("short",), length)


def stored_between(seed):
    """stored blocks between Huffman blocks, their headers at all eight bit offsets"""
    rng = np.random.default_rng(seed)
    blocks = [{"kind": "fixed", "tokens": toks(lits([0, 5, 200]))}]
    for off in range(8):
        blocks.append({"kind": "stored", "data": rng.integers(0, 256, 3 + off).astype(np.uint8).tobytes()})      # ends byte-aligned
        blocks.append(shifter(off))
        blocks.append({"kind": "stored", "data": rng.integers(0, 256, 40 + 37 * off).astype(np.uint8).tobytes()})
        blocks.append(ec.dynamic(toks(lits(rng.integers(0, 64, 700).tolist()) + [(30, 500), (258, 1), (9, 3)])))
    return row_case("stored blocks between Huffman blocks at every bit offset", blocks, ("stored",))


def never_in_step(seed, length=None):
    """The 8-bit code: every token a lane reads is 8 bits at any alignment (literals below 128 never put eight 1 bits in a row), so a
    lane that starts out of phase stays out of phase.  The sub-sequence boundaries of a size that is a multiple of 8 are all in one
    phase, so the block opens with ONE literal 255 (9 bits), inside lane 0's own stretch: behind it the true chain is one bit off every
    boundary, no lane but lane 0 starts in step, and the fixed point takes a pass per lane.  (Without that literal the boundaries of such
    a size are token starts and one pass is enough; with a size that is no multiple of 8 every eighth lane starts in phase.)  One
    such block behind an empty stored block and a shifter for each of the 8 bit offsets of its first token."""
    rng = np.random.default_rng(seed)
    blocks = [{"kind": "fixed", "tokens": toks(lits([0]))}]
    for off in range(8):
        blocks.append({"kind": "stored", "data": b""})                  # the shifter starts byte-aligned
        blocks.append(shifter(off))
        body = lits([255] + rng.integers(0, 128, pm.LANES * max(SUBS) // 8 + 100).tolist())
        blocks.append(ec.dynamic(toks(body), lit=EIGHT_BIT))
    return row_case("8-bit code, never in step", blocks, ("never", "literal-only"), length)


def late_in_step(seed, length=None):
    """the same code with literal 255 (and every other byte) in the data: lanes fall into step late, or at once"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, 9000)
    v[rng.integers(0, 9000, 600)] = 255
    return row_case("8-bit code with literal 255", [shifter(3), ec.dynamic(toks(lits(v.tolist())), lit=EIGHT_BIT)], ("late", "literal-only"),
                    length)


def budget_lone(matches=400, length=None):
    """runs of (258, 1) matches on 1-bit length and distance codes: a default sub-sequence of 256 bits writes 33 KB"""
    items = lits([0]) + [(258, 1)] * matches
    return row_case("one sub-sequence exceeds the budget", [ec.dynamic(toks(items))], ("budget-lone",), length)


def budget_edges(length=None):
    """a fixed block whose first k default sub-sequences end at a token boundary and write 16383, 16384 and 16385 bytes: 8-bit and 9-bit
    literals and (258, 1) matches of 13 bits"""
    out = []
    for target in (pm.BUDGET - 1, pm.BUDGET, pm.BUDGET + 1):
        found = None
        for m in range(40, 64):
            for n9 in range(0, 512):
                n8 = target - 258 * m - n9
                bits = 8 * n8 + 9 * n9 + 13 * m
                if n8 >= 1 and bits % pm.SUB_DEFAULT == 0 and bits // pm.SUB_DEFAULT <= pm.LANES:
                    found = (m, n8, n9)
                    break
            if found:
                break
        m, n8, n9 = found
        items = lits([0] + [(5 * k) % 144 for k in range(n8 - 1)]) + [(258, 1)] * m + lits([160] * n9) + lits([(3 * k) % 144 for k in range(900)])
        out.append(row_case("a round ends at %d bytes" % target, [{"kind": "fixed", "tokens": toks(items)}], ("budget-edge", target), length))
    return out


def same_round_sources(seed, length=None):
    """matches, overlapping ones too, whose source is a literal an earlier lane of the same round wrote"""
    rng = np.random.default_rng(seed)
    items = lits([0])
    for _ in range(12):
        items += lits(rng.integers(0, 256, 200).tolist())
        items += [(100, 150), (50, 7), (258, 1), (40, 190), (17, 2)]
        items += lits(rng.integers(0, 256, 200).tolist())
        items += [(258, 199), (30, 29)]                                  # overlapping, from literals some lanes back
    return row_case("matches over literals of the same round", [ec.dynamic(toks(items))], ("same-round",), length)


def far_flushed(seed):
    """distance 32768 into bytes that were flushed rounds before"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 256, 32768).astype(np.uint8)
    r[0] = 0
    raw = r.tobytes() + r[:5000].tobytes()
    return row_case("distance 32768 into flushed output", [ec.dynamic(dw.match(raw, [32768]))], ("far",))


# ---- the ring, the match list, chains, the longest token (tests/test_png_par_corpus.py proves each from the model) ----------------------
class _Lay:
    """tokens laid down with the output position known: .n is the next output byte"""
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.items, self.n = lits([0]), 1

    def lit(self, k):
        self.items += lits(self.rng.integers(0, 256, k).tolist())
        self.n += k

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= min(self.n, 32768), (length, dist, self.n)
        self.items.append((length, dist))
        self.n += length

    def fill(self, pos):
        """to output byte pos: literals with a match now and then, and nothing but literals over the last 600 bytes"""
        while self.n < pos - 1200:
            self.lit(150)
            self.match(int(self.rng.integers(3, 259)), int(self.rng.integers(100, min(self.n, 30000))))
        self.lit(pos - self.n)

    def block(self):
        return ec.dynamic(toks(self.items))


def ring_alias(seed):
    """A literal written ahead of a match of its round that reads more than 16 KiB back: in a 32 KiB ring the literal's slot would be
    one the match still reads.  40 000 literals, then matches at distances of 16 500 .. 32 767 (every fourth within 168 of 32 768, so
    that the 384-byte rounds of the smallest size reach the aliased slot too) between runs of 100 .. 600 literals, to past 66 000."""
    lay = _Lay(seed)
    lay.lit(39999)
    k = 0
    while lay.n <= 66000:
        lo = 32600 if k % 4 == 3 else 16500
        lay.match(int(lay.rng.integers(3, 259)), int(lay.rng.integers(lo, 32768)))
        lay.lit(int(lay.rng.integers(100, 601)))
        k += 1
    return row_case("literals ahead of matches more than 16 KiB back", [lay.block()], ("alias",))


def ring_wrap(seed):
    """four files around output byte 65536, slot 0 of the ring: a match whose destination straddles it and one whose source does; an
    overlapping match whose destination straddles it; a match of distance 32768 that begins exactly there; literals of several lanes
    of one round on both sides"""
    out = []
    lay = _Lay(seed)
    lay.fill(RING - 100)
    lay.match(200, 5000)                                                 # writes 65436 .. 65635
    lay.lit(50)
    lay.match(150, lay.n - (RING - 70))                                  # reads 65466 .. 65615, distance 220
    lay.lit(300)
    out.append(row_case("matches to and from both sides of byte 65536", [lay.block()], ("wrap", "dst", "src")))
    lay = _Lay(seed + 1)
    lay.fill(RING - 100)
    lay.match(250, 7)                                                    # overlapping, writes 65436 .. 65685
    lay.lit(40)
    lay.match(258, 1)
    lay.lit(300)
    out.append(row_case("an overlapping match across byte 65536", [lay.block()], ("wrap", "overlap")))
    lay = _Lay(seed + 2)
    lay.fill(RING)
    lay.match(258, 32768)                                                # begins at byte 65536, reads from 32768 on
    lay.lit(30)
    lay.match(100, 32768)
    lay.lit(300)
    out.append(row_case("distance 32768 from byte 65536", [lay.block()], ("wrap", "far")))
    lay = _Lay(seed + 3)
    lay.fill(RING + 500)                                                 # literals from 64936 to 66035
    lay.match(30, 400)
    lay.lit(200)
    out.append(row_case("literals of one round across byte 65536", [lay.block()], ("wrap", "literals")))
    return out


def ring_wrap_stored(seed):
    """a Huffman block of 30 000 bytes, a stored block of 65 535 bytes that carries the output across byte 65536 (every piece of the copy
    loop is cut by the staging), then a dynamic block whose first tokens are matches into the stored bytes before, across and behind
    that byte"""
    lay = _Lay(seed)
    lay.fill(30000)
    stored = lay.rng.integers(0, 256, 65535).astype(np.uint8).tobytes()
    n = 30000 + 65535
    items = [(200, n - 63000)]
    n += 200
    items.append((258, n - (RING - 60)))                                 # reads 65476 .. 65733
    n += 258
    items.append((120, n - 70000))
    n += 120
    items += lits(lay.rng.integers(0, 256, 400).tolist())
    return row_case("a stored block across byte 65536", [lay.block(), {"kind": "stored", "data": stored}, ec.dynamic(toks(items))],
                    ("wrap-stored",))


LIST_LIT = [2] + [0] * 255 + [2, 1]                # literal 0 and the end-of-block symbol on 2 bits, length symbol 257 on 1 bit
LIST_DIST = [1] + [0] * 29                         # distance 1 on 1 bit


def match_list(matches=12000, length=None):
    """(3, 1) matches of 2 bits behind one literal 0: at 254 bits a lane holds 127 of them and 43 lanes' 5461 matches are 16 383 bytes,
    the most a round can hold -- the match list's last entry but one and the largest offset of its 16-bit column"""
    items = lits([0]) + [(3, 1)] * matches
    return row_case("a round of 5461 three-byte matches", [ec.dynamic(toks(items), lit=LIST_LIT, dist=LIST_DIST)], ("list",), length)


def chains(seed, length=None):
    """matches that read what earlier matches of the same round wrote, three deep (40 from literals, 30 from those 40, 20 from those 30),
    an overlapping match that reads an overlapping match's bytes, and two matches that neither read nor write each other's bytes"""
    lay = _Lay(seed)
    lay.lit(700)
    for k in range(40):
        lay.lit(20 + 7 * (k % 9))
        lay.match(40, 50)
        lay.match(30, 35)
        lay.match(20, 25)
        lay.match(50, 3)                                                 # overlapping
        lay.match(40, 7)                                                 # overlapping, over the bytes of the one before
        lay.lit(10)
        lay.match(30, 400)                                               # independent of each other: both read literals
        lay.match(30, 600)                                               # written before the round's matches
    return row_case("matches over matches of the same round", [lay.block()], ("chain",), length)


def long_tokens(seed, per=64, length=None):
    """48-bit matches (a 15-bit length code with 5 extra bits, a 15-bit distance code with 13) behind 0 .. 31 one-bit literals each, so
    that one starts at every bit of a 32-bit word; a second such run behind a shifter"""
    rng = np.random.default_rng(seed)
    lit = dw.complete_lengths([256] + list(range(1, 40)), {0: 1, 281: 15}, 286)       # lengths 131 .. 162
    dist = dw.complete_lengths(list(range(29)), {29: 15}, 30)
    blocks = [{"kind": "fixed", "tokens": toks(lits([0]))},
              {"kind": "stored", "data": rng.integers(0, 256, 25000).astype(np.uint8).tobytes()}]
    n = 25001
    for off in (0, 3):
        if off:
            blocks += [{"kind": "stored", "data": b""}, shifter(off)]
            n += len(blocks[-1]["tokens"].lit)
        items, rel = [], 0
        for k in range(per):
            fill = (k - rel) % 32                                        # token k starts k bits (mod 32) behind the block's first
            m = (131 + int(rng.integers(0, 32)), 24577 + int(rng.integers(0, min(n + fill, 32768) - 24576)))
            items += lits([0] * fill) + [m]
            rel += fill + 48
            n += fill + m[0]
        blocks.append(ec.dynamic(toks(items), lit=lit, dist=dist))
    return row_case("48-bit tokens at every bit of a word", blocks, ("long-token",), length)


def tiny_row(seed, length=None):
    """ec.tiny_blocks_case as a file of one row: 400 one-symbol blocks, dynamic and fixed in turn"""
    raw = ec.source(2560, 2560, seed, ec.NEAR)
    tok = dw.match(raw, ec.NEAR)
    blocks = []
    for k in range(400):
        t = dw.Tokens(tok.lit[k:k + 1], tok.length[k:k + 1], tok.dist[k:k + 1])
        blocks.append(ec.dynamic(t, ("go", "zlib")[k % 3 == 0]) if k % 2 == 0 else {"kind": "fixed", "tokens": t})
    blocks.append({"kind": "fixed", "tokens": dw.Tokens(tok.lit[400:], tok.length[400:], tok.dist[400:])})
    return row_case("hundreds of one-symbol blocks in one row", blocks, ("tiny",), length)


def _zlib_case(name, samples, ctype, tags=(), **kw):
    f = pc.write(samples, ctype, 8, **kw)
    st, fields = dm.parse(f)
    assert st == dm.OK
    stream = b"".join(fields["idat"])
    return Case(name, f, stream, zlib.decompress(stream), tuple(tags))


def zlib_cases(seed):
    out = []
    for k, (w, h) in enumerate(ec.UNIT_EDGES):                                   # raw lengths k * 16384 and one either side
        out.append(_zlib_case("raw %d zlib 6" % ((w + 1) * h), pc.photo(h, w, 1, seed + k)[..., 0], 0, ("unit",), filters=(1, 4), level=6))
    for level in (1, 6, 9):
        out.append(_zlib_case("zlib level %d rgb 192x170" % level, pc.photo(170, 192, 3, seed + 10), 2, ("level",), filters=(4, 1, 2), level=level))
    for sname, strat in (("huffman-only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("fixed", zlib.Z_FIXED)):
        for cname, fn in (("photo", pc.photo), ("flat", pc.flat)):
            tags = ("strategy",) + (("literal-only",) if strat == zlib.Z_HUFFMAN_ONLY else ())
            out.append(_zlib_case("zlib %s %s rgb 120x100" % (sname, cname), fn(100, 120, 3, seed + 20), 2, tags, filters=(4, 2), strategy=strat))
    return out


def adam7_case(seed):
    f = a7.of_type(2, 8, False, 40, 50, seed, filters=(4,))
    stream = idat_of(f)
    return Case("Adam7 rgb 50x40", f, stream, zlib.decompress(stream), ("adam7",), adam7=True)


def idat_of(data):
    out, i = b"", 8
    while i < len(data):
        n = struct.unpack(">I", data[i:i + 4])[0]
        if data[i + 4:i + 8] == b"IDAT":
            out += data[i + 8:i + 8 + n]
        i += 12 + n
    return out


def rewrap(data, stream):
    """the file with its IDAT chunks replaced by one chunk of this stream"""
    out, i, done = data[:8], 8, False
    while i < len(data):
        n = struct.unpack(">I", data[i:i + 4])[0]
        if data[i + 4:i + 8] == b"IDAT":
            if not done:
                out += pc.chunk(b"IDAT", stream)
                done = True
        else:
            out += data[i:i + 12 + n]
        i += 12 + n
    return out


def damaged(clean, seed):
    """twins of a dozen clean files: the stream cut short, a bit of the body flipped, the Adler-32 wrong"""
    rng = np.random.default_rng(seed)
    out = []
    for k, c in enumerate(clean):
        s = bytearray(c.stream)
        kind = ("truncated", "bit flipped", "wrong adler")[k % 3]
        if kind == "truncated":
            s = s[:max(3, int(len(s) * (0.3 + 0.05 * (k % 7))))]
        elif kind == "bit flipped":
            at = int(rng.integers(len(s) // 4, len(s) - 4))
            s[at] ^= 1 << int(rng.integers(0, 8))
        else:
            s[-1] ^= 0x55
        out.append(Case(c.name + " / " + kind, rewrap(c.data, bytes(s)), bytes(s), b"", c.tags, kind, c.adam7))
    return out


def two_idat(data, stream, tail):
    """the file with its IDAT chunks replaced by two: the stream, and `tail` behind it"""
    one = pc.chunk(b"IDAT", stream)
    f = rewrap(data, stream)
    at = f.index(one) + len(one)
    return f[:at] + pc.chunk(b"IDAT", tail) + f[at:]


def trailing_twins(seed=31):
    """Streams in order with something behind the Adler-32: IPX_ERR_UNSUPPORTED, and only from a serial walk that got every token, every
    flush and the checksum right.  Every clean file of the corpus with one zero byte behind its stream ("trailing byte"), and three of
    them (more than 64 KiB, stored blocks, Adam7) with a second IDAT chunk of 4 bytes behind the whole stream ("trailing idat")."""
    key = ("trailing", seed)
    if key not in _CACHE:
        clean = [c for c in corpus(seed, edges=True) if not c.damage]
        out = [Case(c.name + " / trailing byte", rewrap(c.data, c.stream + b"\0"), c.stream + b"\0", c.raw, c.tags, "trailing byte", c.adam7)
               for c in clean]
        for tag in ("alias", "stored", "adam7"):
            c = next(c for c in clean if c.tags[0] == tag)
            out.append(Case(c.name + " / trailing idat", two_idat(c.data, c.stream, b"\0\1\2\3"), c.stream + b"\0\1\2\3", c.raw, c.tags,
                            "trailing idat", c.adam7))
        _CACHE[key] = out
    return _CACHE[key]


MIXED_LENGTH = 40001                   # a gray row of 40 000 samples: every file of mixed_launch has this frame


def mixed_launch(seed=31, length=MIXED_LENGTH):
    """One launch whose files take very different paths through the kernel, all of one frame size: 64 passes a window, a full match
    list, the uniform loop, a block of three tokens, hundreds of blocks, literals only, matches over literals and over matches, 48-bit
    tokens, rounds that end at and beside the unit -- and, next to their clean files, twins with a byte behind the Adler-32 (redone, in
    order) and damaged twins (redone, broken)."""
    key = ("mixed", seed, length)
    if key not in _CACHE:
        clean = [never_in_step(seed + 2, length), match_list(12000, length), budget_lone(140, length), short_block(length),
                 tiny_row(seed + 6, length), late_in_step(seed + 3, length), same_round_sources(seed + 4, length), chains(seed + 13, length),
                 long_tokens(seed + 14, 32, length)] + budget_edges(length)
        clean = [Case(c.name + " / %d bytes" % length, c.data, c.stream, c.raw, c.tags) for c in clean]
        assert all(len(c.raw) == length for c in clean)
        broken = damaged(clean, seed + 60)
        out = []
        for k, c in enumerate(clean):
            out.append(c)
            out.append(Case(c.name + " / trailing byte", rewrap(c.data, c.stream + b"\0"), c.stream + b"\0", c.raw, c.tags, "trailing byte"))
            if k % 4 != 3:
                out.append(broken[k])
        out += clean[:4]                                                 # the same files once more, behind the twins
        _CACHE[key] = out
    return _CACHE[key]


_CACHE = {}


def corpus(seed=31, edges=False):
    """the corpus the tests of the three sizes SUBS run over; edges: with the cases of EDGE_SUBS (EDGE_TAGS) behind its clean files"""
    if seed not in _CACHE:
        clean = [split_parts(seed)] + eob_cases() + [short_block(), stored_between(seed + 1), never_in_step(seed + 2), late_in_step(seed + 3),
                                                      budget_lone()] + budget_edges() + [same_round_sources(seed + 4), far_flushed(seed + 5)]
        t = ec.tiny_blocks_case("hundreds of one-symbol blocks", seed + 6)
        clean.append(Case(t.name, t.data, t.stream, t.raw, ("tiny",)))
        t = ec.far_case("fixed behind dynamic and the reverse", 300, 100, 0, 8, seed + 7, nblocks=6)
        clean.append(Case(t.name, t.data, t.stream, t.raw, ("mixed",)))
        clean += zlib_cases(seed + 8) + [adam7_case(seed + 9)]
        picks = [c for c in clean if c.tags[0] in ("parts", "stored", "late", "budget-lone", "same-round", "far", "tiny", "mixed", "adam7")]
        picks += [c for c in clean if c.tags[0] in ("level", "budget-edge")][:4]
        _CACHE[seed] = clean + damaged(picks, seed + 50)
    if not edges:
        return _CACHE[seed]
    if ("edges", seed) not in _CACHE:
        new = [ring_alias(seed + 10)] + ring_wrap(seed + 20) + [ring_wrap_stored(seed + 11), match_list(), chains(seed + 13), long_tokens(seed + 14)]
        assert {c.tags[0] for c in new} == set(EDGE_TAGS)
        old = _CACHE[seed]
        _CACHE["edges", seed] = [c for c in old if not c.damage] + new + [c for c in old if c.damage]
    return _CACHE["edges", seed]


_RUNS = {}


def run(case, sub):
    """png_par_model's Result for the case's stream at this sub-sequence size, computed once"""
    key = (case.name, sub)
    if key not in _RUNS:
        m = _RUNS.setdefault((case.name, None), pm.Model(case.stream))
        _RUNS[key] = m.run(sub)
    return _RUNS[key]
