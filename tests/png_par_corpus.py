"""PNG files for the parallel inflate (csrc/ipx_png_dec_par.hip, IPX_PNG_PAR=1): streams written with tests/deflate_writer.py, token
by token and code length by code length, and with zlib, aimed at that kernel's own edges -- sub-sequence boundaries inside every part
of a token, end-of-block symbols at and beside a boundary, blocks shorter than a sub-sequence, codes on which a speculative lane never
falls into step, sub-sequences whose output alone exceeds a flush unit, rounds that end at, below and above the unit, matches over
literals of the same round, a distance of 32768 into bytes flushed rounds before -- and damaged twins.  tests/png_par_model.py says
which edge a stream reaches (tests/test_png_par_corpus.py asserts it).

Frames are small: raw lengths from a few bytes to about 100 KB.  A stream laid down token by token is wrapped as a file of one row
(filter byte 0 first), so the tokens need not know about rows.

corpus() -> [Case]; a Case carries the file, its zlib stream, the filtered bytes (clean files), what it aims at (`tags`) and, for a
damaged twin, `damage`."""
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


def row_case(name, blocks, tags=()):
    """the one-row file of these blocks (the first byte they write must be 0: filter None); literals are added in a last fixed block
    until a row of that length exists"""
    raw = b""
    for b in blocks:
        raw += bytes(b["data"]) if b["kind"] == "stored" else b["tokens"].expand(raw)
    assert raw[0] == 0
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


def short_block():
    return row_case("a block shorter than one sub-sequence", [{"kind": "fixed", "tokens": toks(lits([0, 7, 9]))}], ("short",))


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


def never_in_step(seed):
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
    return row_case("8-bit code, never in step", blocks, ("never", "literal-only"))


def late_in_step(seed):
    """the same code with literal 255 (and every other byte) in the data: lanes fall into step late, or at once"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, 9000)
    v[rng.integers(0, 9000, 600)] = 255
    return row_case("8-bit code with literal 255", [shifter(3), ec.dynamic(toks(lits(v.tolist())), lit=EIGHT_BIT)], ("late", "literal-only"))


def budget_lone():
    """runs of (258, 1) matches on 1-bit length and distance codes: a default sub-sequence of 256 bits writes 33 KB"""
    items = lits([0]) + [(258, 1)] * 400
    return row_case("one sub-sequence exceeds the budget", [ec.dynamic(toks(items))], ("budget-lone",))


def budget_edges():
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
        out.append(row_case("a round ends at %d bytes" % target, [{"kind": "fixed", "tokens": toks(items)}], ("budget-edge", target)))
    return out


def same_round_sources(seed):
    """matches, overlapping ones too, whose source is a literal an earlier lane of the same round wrote"""
    rng = np.random.default_rng(seed)
    items = lits([0])
    for _ in range(12):
        items += lits(rng.integers(0, 256, 200).tolist())
        items += [(100, 150), (50, 7), (258, 1), (40, 190), (17, 2)]
        items += lits(rng.integers(0, 256, 200).tolist())
        items += [(258, 199), (30, 29)]                                  # overlapping, from literals some lanes back
    return row_case("matches over literals of the same round", [ec.dynamic(toks(items))], ("same-round",))


def far_flushed(seed):
    """distance 32768 into bytes that were flushed rounds before"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 256, 32768).astype(np.uint8)
    r[0] = 0
    raw = r.tobytes() + r[:5000].tobytes()
    return row_case("distance 32768 into flushed output", [ec.dynamic(dw.match(raw, [32768]))], ("far",))


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


_CACHE = {}


def corpus(seed=31):
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
    return _CACHE[seed]


_RUNS = {}


def run(case, sub):
    """png_par_model's Result for the case's stream at this sub-sequence size, computed once"""
    key = (case.name, sub)
    if key not in _RUNS:
        m = _RUNS.setdefault((case.name, None), pm.Model(case.stream))
        _RUNS[key] = m.run(sub)
    return _RUNS[key]
