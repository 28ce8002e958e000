"""The parallel parse of a Huffman block's body (csrc/ipx_png_dec_par.hip, IPX_PNG_PAR=1) as plain Python, over png_decode_model's
inflater: its tables (canonical, go_huffman_ok), its header rules and its errors; only the token loop is replaced by the scheme.

  Model(stream).run(sub) -> Result
    the bits behind a block's next token are cut into LANES sub-sequences of `sub` bits; lane k decodes from its boundary as if a
    literal / length code began there, up to the first token that starts at or past the next boundary (its exit); then passes: lane k
    restarts from lane k - 1's exit, until no lane's start changes.  A lane that meets the end-of-block symbol, a code outside the
    alphabet or the stream's end keeps that as its state and the lanes behind it are dead.  In step, the lanes up to the first
    end-of-block whose bytes together are at most BUDGET are taken and the next window starts behind the last of them; when lane 0's
    bytes alone exceed BUDGET its stretch goes to the uniform (serial) loop.

  Result: redo (the kernel would leave the file: any rule of Go's reader broken, the Adler-32, bytes behind it), data (the bytes),
  tokens [Tok] in stream order (literals, matches and end-of-block symbols), lane_tokens / uniform_tokens (how many of them the lanes
  and the uniform loop decoded), blocks [(kind, first token bit or None)], windows [Window] and stored [(block, first output byte,
  bytes)], the stored blocks.

The token at a bit position does not depend on `sub`, so a Model keeps what it decoded across run() calls."""
import struct
import zlib
from dataclasses import dataclass, field

import png_decode_model as dm

LANES = 64
BUDGET = 16384
SUB_DEFAULT = 256
SUB_MIN, SUB_MAX = 48, 1000
CONT, EOB, ERR, DEAD = range(4)


@dataclass
class Tok:
    bit: int             # where the token starts in the stream
    kind: str            # "lit", "match", "eob"
    nbits: int
    length: int = 0      # bytes it writes (a literal: 1)
    dist: int = 0
    value: int = 0       # the literal byte
    parts: tuple = ()    # a match: bits of (length code, length extra, distance code, distance extra)
    out: int = 0         # its first output byte
    block: int = 0
    window: int = -1     # the window of its block that took it (index into Result.windows), and the lane; lane -1: the uniform loop
    lane: int = -1


@dataclass
class Window:
    block: int
    first_bit: int       # the window's first token
    sub: int
    passes: int          # decode passes to the fixed point, the first one included
    last_valid: int      # the first lane in order that is not CONT (or LANES - 1)
    cum: list = field(default_factory=list)     # inclusive byte sums of lanes 0 .. last_valid
    taken: int = 0       # lanes taken (0: lane 0's stretch went to the uniform loop)
    out_first: int = 0   # the round's first output byte
    nbytes: int = 0      # the bytes the window wrote (uniform: the stretch's)


@dataclass
class Result:
    redo: bool
    why: str = ""
    data: bytes = b""
    tokens: list = field(default_factory=list)
    lane_tokens: int = 0
    uniform_tokens: int = 0
    blocks: list = field(default_factory=list)
    windows: list = field(default_factory=list)
    stored: list = field(default_factory=list)      # (block, first output byte, bytes) of every stored block


class _Code:
    """a canonical code with a 10-bit root table over LSB-first stream bits"""
    def __init__(self, lengths):
        self.table = dm.canonical(lengths)
        self.root = [None] * 1024
        for (L, code), s in self.table.items():
            if L <= 10:
                r = int("{:0{}b}".format(code, L)[::-1], 2)
                for e in range(r, 1024, 1 << L):
                    self.root[e] = (s, L)

    def decode(self, w):
        e = self.root[w & 1023]
        if e is not None:
            return e
        code = 0
        for L in range(1, 16):
            code = (code << 1) | ((w >> (L - 1)) & 1)
            s = self.table.get((L, code))
            if s is not None:
                return s, L
        return -1, 0


_FIXED = None


class _Redo(Exception):
    pass


class Model:
    def __init__(self, stream, limit=None):
        self.d = bytes(stream)
        self.pad = self.d + b"\0" * 16                  # input past the end reads as zero bits
        self.zbits = 8 * len(self.d)
        self.limit = limit
        self.memo = {}                                  # (block, bit) -> Tok or None (a code outside the alphabet)

    # ---- the serial parts: headers, as png_decode_model.inflate reads them ---------------------------------------------------------
    def _head(self, br):
        """the block header at br: (final, kind, codes or None, stored bytes or None)"""
        global _FIXED
        final = br.bits(1)
        t = br.bits(2)
        if t == 0:
            br.pos = (br.pos + 7) & ~7
            p = br.pos >> 3
            if p + 4 > len(self.d):
                raise dm.FlateError("unexpected EOF")
            n, nn = self.d[p] | self.d[p + 1] << 8, self.d[p + 2] | self.d[p + 3] << 8
            if n != (~nn & 0xFFFF):
                raise dm.FlateError("stored length")
            if p + 4 + n > len(self.d):
                raise dm.FlateError("unexpected EOF")
            br.pos = 8 * (p + 4 + n)
            return final, "stored", None, self.d[p + 4:p + 4 + n]
        if t == 3:
            raise dm.FlateError("block type 3")
        if t == 1:
            if _FIXED is None:
                _FIXED = (_Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _Code([5] * 32))
            return final, "fixed", _FIXED, None
        hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
        if hlit > 286 or hdist > 30:
            raise dm.FlateError("HLIT / HDIST")
        cl = [0] * 19
        for k in range(hclen):
            cl[dm.CLEN_ORDER[k]] = br.bits(3)
        if not dm.go_huffman_ok(cl):
            raise dm.FlateError("code length code")
        ct = dm.canonical(cl)
        lens = []
        n = hlit + hdist
        while len(lens) < n:
            s = br.sym(ct)
            if s < 16:
                lens.append(s)
                continue
            if s == 16:
                if not lens:
                    raise dm.FlateError("repeat at the first position")
                rep, val = 3 + br.bits(2), lens[-1]
            elif s == 17:
                rep, val = 3 + br.bits(3), 0
            else:
                rep, val = 11 + br.bits(7), 0
            if len(lens) + rep > n:
                raise dm.FlateError("repeat past HLIT + HDIST")
            lens += [val] * rep
        if not dm.go_huffman_ok(lens[:hlit]) or not dm.go_huffman_ok(lens[hlit:]):
            raise dm.FlateError("incomplete code")
        return final, "dynamic", (_Code(lens[:hlit]), _Code(lens[hlit:])), None

    # ---- one token at a bit position -----------------------------------------------------------------------------------------------
    def token(self, block, codes, p):
        """the token a lane reads at bit p (None: no such code, symbol 286 / 287, distance code 30 / 31)"""
        key = (block, p)
        if key in self.memo:
            return self.memo[key]
        w = int.from_bytes(self.pad[p >> 3:(p >> 3) + 8], "little") >> (p & 7) if (p >> 3) + 8 <= len(self.pad) else 0
        s, L = codes[0].decode(w)
        t = None
        if 0 <= s < 256:
            t = Tok(p, "lit", L, 1, value=s)
        elif s == 256:
            t = Tok(p, "eob", L)
        elif 256 < s <= 285:
            le = dm.LEN_EXTRA[s - 257]
            length = dm.LEN_BASE[s - 257] + ((w >> L) & ((1 << le) - 1))
            ds, DL = codes[1].decode(w >> (L + le))
            if 0 <= ds < 30:
                de = dm.DIST_EXTRA[ds]
                dist = dm.DIST_BASE[ds] + ((w >> (L + le + DL)) & ((1 << de) - 1))
                t = Tok(p, "match", L + le + DL + de, length, dist, parts=(L, le, DL, de))
        self.memo[key] = t
        return t

    def _stretch(self, block, codes, p, lim):
        """a lane's stretch: the tokens from p that start before lim -> (exit, state, tokens, bytes)"""
        toks, nby = [], 0
        while p < lim:
            t = self.token(block, codes, p)
            if t is None:
                return p, ERR, toks, nby
            p += t.nbits
            toks.append(t)
            if p > self.zbits:
                return p, ERR, toks, nby
            if t.kind == "eob":
                return p, EOB, toks, nby
            nby += t.length
        return p, CONT, toks, nby

    # ---- the scheme ----------------------------------------------------------------------------------------------------------------
    def run(self, sub=SUB_DEFAULT):
        sub = min(SUB_MAX, max(SUB_MIN, sub))
        res = Result(False)
        out = bytearray()
        try:
            self._run(sub, res, out)
        except (dm.FlateError, _Redo) as e:
            return Result(True, str(e))
        res.data = bytes(out)
        return res

    def _emit(self, res, out, t, b, w, lane):
        t = Tok(**{**t.__dict__, "out": len(out), "block": b, "window": w, "lane": lane})
        res.tokens.append(t)
        if t.kind == "lit":
            out.append(t.value)
        elif t.kind == "match":
            if t.dist > len(out):
                raise _Redo("distance too far back")
            for _ in range(t.length):
                out.append(out[-t.dist])
        if self.limit is not None and len(out) > self.limit:
            raise _Redo("too much pixel data")

    def _run(self, sub, res, out):
        d = self.d
        if len(d) < 2:
            raise _Redo("zlib: unexpected EOF")
        cmf, flg = d[0], d[1]
        if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
            raise _Redo("zlib: invalid header")
        br = dm.Bits(d)
        br.pos = 16
        final, b = False, -1
        while not final:
            b += 1
            final, kind, codes, stored = self._head(br)
            if kind == "stored":
                res.blocks.append((kind, None))
                res.stored.append((b, len(out), len(stored)))
                out += stored
                if self.limit is not None and len(out) > self.limit:
                    raise _Redo("too much pixel data")
                continue
            P = br.pos
            res.blocks.append((kind, P))
            while True:                                              # windows
                if P > self.zbits:
                    raise _Redo("unexpected EOF")
                start = [P + k * sub for k in range(LANES)]
                lim = [P + (k + 1) * sub for k in range(LANES)]
                r = [self._stretch(b, codes, start[k], lim[k]) for k in range(LANES)]
                passes = 1
                while True:
                    ns = [start[0]] + [r[k - 1][0] if r[k - 1][1] == CONT else None for k in range(1, LANES)]
                    ch = [k for k in range(LANES) if ns[k] != start[k]]
                    if not ch:
                        break
                    passes += 1
                    for k in ch:
                        start[k] = ns[k]
                        r[k] = (None, DEAD, [], 0) if ns[k] is None else self._stretch(b, codes, ns[k], lim[k])
                last = next((k for k in range(LANES) if r[k][1] != CONT), LANES - 1)
                if r[last][1] == ERR:
                    raise _Redo("a rule broken on the chain in step")
                cum, c = [], 0
                for k in range(last + 1):
                    c += r[k][3]
                    cum.append(c)
                taken = sum(1 for c in cum if c <= BUDGET)
                win = Window(b, P, sub, passes, last, cum, taken, len(out))
                wi = len(res.windows)
                res.windows.append(win)
                if taken == 0:                                       # the uniform loop: the tokens that start before P + sub
                    p, eob = P, False
                    while p < P + sub and not eob:
                        t = self.token(b, codes, p)
                        if t is None:
                            raise _Redo("invalid code")
                        p += t.nbits
                        if p > self.zbits:
                            raise _Redo("unexpected EOF")
                        self._emit(res, out, t, b, wi, -1)
                        res.uniform_tokens += 1
                        eob = t.kind == "eob"
                    win.nbytes = len(out) - win.out_first
                    P = p
                    if eob:
                        break
                    continue
                for k in range(taken):
                    for t in r[k][2]:
                        self._emit(res, out, t, b, wi, k)
                    res.lane_tokens += len(r[k][2])
                win.nbytes = len(out) - win.out_first
                assert win.nbytes == cum[taken - 1]
                P = r[taken - 1][0]
                if r[taken - 1][1] == EOB:
                    break
            br.pos = P
        if self.limit is not None and len(out) != self.limit:
            raise _Redo("not enough pixel data")
        p = (br.pos + 7) >> 3
        if p + 4 > len(d):
            raise _Redo("unexpected EOF")
        if struct.unpack(">I", d[p:p + 4])[0] != zlib.adler32(bytes(out)):
            raise _Redo("zlib: invalid checksum")
        if p + 4 != len(d):
            raise _Redo("bytes after the Adler-32")
