"""A raw-deflate writer under the tests' control, for the PNG decoder's edge corpus (tests/png_edge_corpus.py).

zlib never writes distances above 32506, sends the literal / length and distance code lengths as two separate run-length sequences and
puts long codes only where its statistics happen to.  Go's compress/flate, libdeflate and zopfli do other valid things; this writer can do
them on purpose:

  write(blocks, raw) -> the zlib stream (header, blocks, Adler-32 of raw); each block is a dict:
    {"kind": "stored", "data": bytes}                                  any length up to 65535, 0 included
    {"kind": "fixed", "tokens": Tokens}
    {"kind": "dynamic", "tokens": Tokens, "lit": lengths or None, "dist": lengths or None, "codegen": "zlib" | "go"}
       lengths None: computed from the block's frequencies with a limit of 15; given: any complete code over the symbols used
  match(raw, dists) -> Tokens: a fixed-candidate matcher (numpy): at each position the longest match at the first distance of `dists`
    that gives >= 3 bytes, else a literal
  stats(stream) -> what a stream reaches: largest distance, distances above 32506, code lengths used per alphabet, codegen repeats that
    cross HLIT, block kinds and their bit offsets, stored lengths (a table-driven inflater of its own, which also returns the bytes)

Only streams valid for both Go and zlib are written: complete codes (or the single distance code of length 1), HLIT <= 286,
HDIST <= 30, no symbols 286 / 287, no distance codes 30 / 31.  A helper of the tests only."""
import heapq
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 - 1 for k in range(4, 30)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
ZLIB_MAX_DIST = 32768 - 262
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30

# symbol of every match length 3 .. 258 and of every distance 1 .. 32768
_LSYM = np.zeros(259, np.int64)
for _s in range(29):
    _LSYM[LEN_BASE[_s]:LEN_BASE[_s] + (1 << LEN_EXTRA[_s])] = 257 + _s
_LSYM[258] = 285
_DSYM = np.zeros(32769, np.int64)
for _s in range(30):
    _DSYM[DIST_BASE[_s]:DIST_BASE[_s] + (1 << DIST_EXTRA[_s])] = _s
_LBASE, _LEXTRA = np.array(LEN_BASE + [0, 0], np.int64), np.array(LEN_EXTRA + [0, 0], np.int64)
_DBASE, _DEXTRA = np.array(DIST_BASE, np.int64), np.array(DIST_EXTRA, np.int64)


class Tokens:
    """a block's symbols: per token a literal byte (length 0) or a match (length 3 .. 258, distance 1 .. 32768)"""
    def __init__(self, lit, length, dist):
        self.lit = np.asarray(lit, np.int64)
        self.length = np.asarray(length, np.int64)
        self.dist = np.asarray(dist, np.int64)

    def nbytes(self):
        return int(np.where(self.length > 0, self.length, 1).sum())

    def split(self, k):
        """the tokens cut into k runs of about equal count"""
        cuts = np.linspace(0, len(self.lit), k + 1).astype(int)
        return [Tokens(self.lit[a:b], self.length[a:b], self.dist[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]

    def expand(self, prefix=b""):
        out = bytearray(prefix)
        for c, n, d in zip(self.lit.tolist(), self.length.tolist(), self.dist.tolist()):
            if n == 0:
                out.append(c)
            else:
                for _ in range(n):
                    out.append(out[-d])
        return bytes(out[len(prefix):])

    def symbols(self):
        """(lit / length symbol, distance symbol or -1) per token"""
        m = self.length > 0
        ls = np.where(m, _LSYM[np.minimum(self.length, 258)], self.lit)
        ds = np.where(m, _DSYM[np.minimum(self.dist, 32768)], -1)
        return ls, ds


def literals(raw):
    raw = np.frombuffer(bytes(raw), np.uint8)
    z = np.zeros(len(raw), np.int64)
    return Tokens(raw, z, z)


def match(raw, dists, start=0, end=None):
    """tokens of raw[start:end] (matches may reach back before start): at each position, the longest match (<= 258, inside raw[:end])
    at the first distance of `dists` that gives >= 3 bytes, else a literal"""
    a = np.frombuffer(bytes(raw), np.uint8)
    end = len(a) if end is None else end
    n = end - start
    best_len = np.zeros(n, np.int64)
    best_dist = np.zeros(n, np.int64)
    for d in dists:
        if d > end - 1:
            continue
        eq = np.zeros(end, bool)
        eq[d:end] = a[d:end] == a[:end - d]
        pos = np.arange(end)
        nf = np.where(eq, end, pos)
        run = np.minimum.accumulate(nf[::-1])[::-1] - pos               # equal bytes from here on (the stream end stops a run)
        run = np.minimum(run[start:end], 258)
        take = (best_len == 0) & (run >= 3)
        best_len[take] = run[take]
        best_dist[take] = d
    lit, length, dist = [], [], []
    has = best_len >= 3
    nxt = np.where(has, np.arange(n), n)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]                          # the next position that starts a match
    i = 0
    while i < n:
        j = int(nxt[i])
        if j > i:
            lit.append(a[start + i:start + j].astype(np.int64))
            length.append(np.zeros(j - i, np.int64))
            dist.append(np.zeros(j - i, np.int64))
            i = j
            if i >= n:
                break
        L = int(best_len[i])
        lit.append(np.zeros(1, np.int64))
        length.append(np.array([L], np.int64))
        dist.append(np.array([best_dist[i]], np.int64))
        i += L
    if not lit:
        return Tokens([], [], [])
    return Tokens(np.concatenate(lit), np.concatenate(length), np.concatenate(dist))


# ---- code lengths ----------------------------------------------------------------------------------------------------------------
def huffman_lengths(freq, limit=15):
    """code lengths of a Huffman code over the symbols with freq > 0, at most `limit` bits (frequencies halved until it fits);
    a lone symbol gets length 1 and a partner of length 1 (the code stays complete)"""
    freq = [int(f) for f in freq]
    used = [s for s, f in enumerate(freq) if f > 0]
    if len(used) == 0:
        used = [0, 1]
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    f = {s: max(freq[s], 1) for s in used}
    while True:
        heap = [(f[s], k, [s]) for k, s in enumerate(used)]
        heapq.heapify(heap)
        depth = {s: 0 for s in used}
        k = len(heap)
        while len(heap) > 1:
            fa, _, sa = heapq.heappop(heap)
            fb, _, sb = heapq.heappop(heap)
            for s in sa + sb:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, k, sa + sb))
            k += 1
        if max(depth.values()) <= limit:
            break
        f = {s: max(1, v >> 1) for s, v in f.items()}
    out = [0] * len(freq)
    for s in used:
        out[s] = depth[s]
    return out


def complete_lengths(order, fixed, n):
    """an explicit complete code over `order` (symbols, most frequent first) and `fixed` ({symbol: length}, or a list of symbols that
    get 15 bits): the symbols of `fixed` get their lengths, the others share the rest of the Kraft sum (shorter codes first);
    a list of n lengths"""
    if not isinstance(fixed, dict):
        fixed = {s: 15 for s in fixed}
    rest = [s for s in dict.fromkeys(order) if s not in fixed]
    budget = (1 << 15) - sum(1 << (15 - L) for L in fixed.values())   # in units of 2^-15
    terms = [1 << b for b in range(15, -1, -1) if budget >> b & 1]
    assert len(terms) <= len(rest), "too few symbols to complete the code"
    while len(terms) < len(rest) or terms[0] > 1 << 14:
        t = terms.pop(0)
        terms[:0] = [t >> 1, t >> 1]
        terms.sort(reverse=True)
    assert len(terms) == len(rest)
    out = [0] * n
    for s, L in fixed.items():
        out[s] = L
    for s, t in zip(rest, terms):
        out[s] = 15 - (t.bit_length() - 1)
    return out


def kraft_ok(lengths):
    nz = [n for n in lengths if n]
    if len(nz) == 1:
        return nz[0] == 1
    return sum(1 << (15 - n) for n in nz) == 1 << 15 and max(nz) <= 15


def canonical_codes(lengths):
    """code per symbol, bit-reversed for LSB-first output"""
    count = [0] * 16
    for n in lengths:
        if n:
            count[n] += 1
    nxt, code = [0] * 16, 0
    for L in range(1, 16):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    out = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            c = nxt[n]
            nxt[n] += 1
            out[s] = int("{:0{}b}".format(c, n)[::-1], 2)
    return out


# ---- code-length (codegen) emitters ----------------------------------------------------------------------------------------------
def _rle(seq):
    """[(symbol, extra value, extra bits)] of one run-length sequence, the rules Go's generateCodegen and zlib's send_tree share"""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        n = 1
        while i + n < len(seq) and seq[i + n] == v:
            n += 1
        i += n
        if v == 0:
            while n >= 11:
                k = min(n, 138)
                out.append((18, k - 11, 7))
                n -= k
            if n >= 3:
                out.append((17, n - 3, 3))
                n = 0
        else:
            out.append((v, 0, 0))
            n -= 1
            while n >= 3:
                k = min(n, 6)
                out.append((16, k - 3, 2))
                n -= k
        out += [(v, 0, 0)] * n
    return out


def codegen(lit, dist, style):
    """zlib: the two sequences run-length coded apart; go: one sequence over HLIT + HDIST (a repeat may cross the boundary)"""
    if style == "go":
        return _rle(list(lit) + list(dist))
    return _rle(list(lit)) + _rle(list(dist))


# ---- the bit writer --------------------------------------------------------------------------------------------------------------
class BitWriter:
    """fields (value, bit count) LSB first, packed once with numpy"""
    def __init__(self):
        self.vals, self.nbits, self.pos = [], [], 0

    def put(self, vals, nbits):
        vals = np.atleast_1d(np.asarray(vals, np.int64))
        nbits = np.broadcast_to(np.asarray(nbits, np.int64), vals.shape).copy()
        keep = nbits > 0
        vals, nbits = vals[keep], nbits[keep]
        self.vals.append(vals)
        self.nbits.append(nbits)
        self.pos += int(nbits.sum())

    def align(self):
        self.put(0, (-self.pos) % 8)

    def tobytes(self):
        bits = []
        for vv, nn in zip(self.vals, self.nbits):
            for c in range(0, len(vv), 1 << 19):                      # bounded temporaries on multi-megabyte frames
                v, n = vv[c:c + (1 << 19)], nn[c:c + (1 << 19)]
                start = np.concatenate([[0], np.cumsum(n)[:-1]])
                rep = np.repeat(np.arange(len(v)), n)
                off = np.arange(int(n.sum())) - start[rep]
                bits.append(((v[rep] >> off) & 1).astype(np.uint8))
        b = np.concatenate(bits) if bits else np.zeros(0, np.uint8)
        return np.packbits(b, bitorder="little").tobytes()


def _put_tokens(bw, tok, lit_len, dist_len):
    lc, dc = np.array(canonical_codes(lit_len), np.int64), np.array(canonical_codes(dist_len), np.int64)
    ll, dl = np.array(lit_len, np.int64), np.array(dist_len, np.int64)
    ls, ds = tok.symbols()
    m = tok.length > 0
    assert (ll[ls] > 0).all() and (dl[ds[m]] > 0).all(), "a symbol without a code"
    li = np.maximum(ls - 257, 0)
    di = np.maximum(ds, 0)
    # per token: the symbol, the length's extra bits, the distance symbol, its extra bits
    vals = np.stack([lc[ls], np.where(m, tok.length - _LBASE[li], 0), np.where(m, dc[di], 0), np.where(m, tok.dist - _DBASE[di], 0)], 1)
    nb = np.stack([ll[ls], np.where(m, _LEXTRA[li], 0), np.where(m, dl[di], 0), np.where(m, _DEXTRA[di], 0)], 1)
    bw.put(vals.ravel(), nb.ravel())
    bw.put(lc[256], ll[256])


def _freqs(tok):
    ls, ds = tok.symbols()
    lf = np.bincount(ls, minlength=286)[:286].copy()
    lf[256] += 1
    df = np.bincount(ds[ds >= 0], minlength=30)[:30]
    return lf, df


def dynamic_lengths(tok):
    """Huffman lengths (limit 15) of a block's symbols; no distances: the single distance code of length 1"""
    lf, df = _freqs(tok)
    lit = huffman_lengths(lf)
    dist = huffman_lengths(df) if df.any() else [1] + [0] * 29
    if df.any() and np.count_nonzero(df) == 1:
        dist = [0] * 30
        dist[int(np.flatnonzero(df)[0])] = 1                            # a lone distance symbol: the single code of length 1
    return lit, dist


def write_block(bw, blk, final):
    kind = blk["kind"]
    if kind == "stored":
        data = bytes(blk["data"])
        assert len(data) <= 65535
        bw.put(final | 0 << 1, 3)
        bw.align()
        bw.put([len(data), len(data) ^ 0xFFFF], 16)
        bw.put(np.frombuffer(data, np.uint8), 8)
        return
    tok = blk["tokens"]
    assert ((tok.length == 0) | ((tok.length >= 3) & (tok.length <= 258))).all() and (tok.dist <= 32768).all()
    if kind == "fixed":
        bw.put(final | 1 << 1, 3)
        _put_tokens(bw, tok, FIXED_LIT, FIXED_DIST)
        return
    lit, dist = dynamic_lengths(tok)
    lit = list(blk.get("lit") or lit)
    dist = list(blk.get("dist") or dist)
    lit += [0] * (286 - len(lit))
    dist += [0] * (30 - len(dist))
    assert kraft_ok(lit) and (kraft_ok(dist) or dist.count(0) == 29 and 1 in dist) and lit[256] > 0
    hlit = max(257, max(s for s in range(286) if lit[s]) + 1)
    hdist = max(1, max((s for s in range(30) if dist[s]), default=0) + 1)
    lit, dist = lit[:hlit], dist[:hdist]
    cg = codegen(lit, dist, blk.get("codegen", "zlib"))
    cf = np.bincount([s for s, _, _ in cg], minlength=19)
    cl = huffman_lengths(cf, limit=7)
    hclen = max(4, max(k for k in range(19) if cl[CLEN_ORDER[k]]) + 1)
    bw.put(final | 2 << 1, 3)
    bw.put([hlit - 257, hdist - 1, hclen - 4], [5, 5, 4])
    bw.put([cl[CLEN_ORDER[k]] for k in range(hclen)], 3)
    cc = canonical_codes(cl)
    v, n = [], []
    for s, ev, eb in cg:
        v += [cc[s], ev]
        n += [cl[s], eb]
    bw.put(v, n)
    _put_tokens(bw, tok, lit + [0] * (286 - hlit), dist + [0] * (30 - hdist))


def write(blocks, raw):
    """the zlib stream of the blocks (the last one final); raw is what they decode to (for the Adler-32)"""
    bw = BitWriter()
    bw.put([0x78, 0x9C], 8)                                             # 32 KiB window, default level: what zlib's header says
    for k, blk in enumerate(blocks):
        write_block(bw, blk, int(k == len(blocks) - 1))
    bw.align()
    return bw.tobytes() + struct.pack(">I", zlib.adler32(bytes(raw)))


# ---- stats: a table-driven inflater of its own ----------------------------------------------------------------------------------
def _table(lengths):
    """15-bit LSB-first window -> (symbol, length); (-1, 0) where no code matches"""
    t = [(-1, 0)] * (1 << 15)
    codes = canonical_codes(lengths)
    for s, n in enumerate(lengths):
        if n:
            for hi in range(1 << (15 - n)):
                t[codes[s] | hi << n] = (s, n)
    return t


_FIXED_TABLES = None


def stats(stream):
    """(what the stream reaches, its bytes): dict of max_dist, far (distances > 32506), lit_lens / len_lens / dist_lens (Counter
    of code length -> symbols decoded at it), cross (codegen repeats crossing HLIT), blocks [(kind, bit offset of the header)],
    stored [lengths], stored_offsets {bit offset mod 8 of stored headers}"""
    global _FIXED_TABLES
    from collections import Counter
    d = bytes(stream) + b"\0" * 8
    pos = 16
    out = bytearray()
    st = {"max_dist": 0, "far": 0, "lit_lens": Counter(), "len_lens": Counter(), "dist_lens": Counter(), "cross": 0, "at_hlit": 0, "blocks": [],
          "stored": [], "stored_offsets": set()}

    def bits(n):
        nonlocal pos
        v = (int.from_bytes(d[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def sym(t):
        nonlocal pos
        s, n = t[(int.from_bytes(d[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & 0x7FFF]
        assert n, "invalid code"
        pos += n
        return s, n

    final = 0
    while not final:
        hdr_at = pos
        final, kind = bits(1), bits(2)
        if kind == 0:
            st["blocks"].append(("stored", hdr_at))
            st["stored_offsets"].add(hdr_at % 8)
            pos = (pos + 7) & ~7
            n = bits(16)
            assert bits(16) == n ^ 0xFFFF
            out += d[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            st["stored"].append(n)
            continue
        assert kind != 3
        if kind == 1:
            if _FIXED_TABLES is None:
                _FIXED_TABLES = (_table(FIXED_LIT), _table(FIXED_DIST + [5, 5]))
            lt, dt = _FIXED_TABLES
            ll, dl = FIXED_LIT, FIXED_DIST
            st["blocks"].append(("fixed", hdr_at))
        else:
            st["blocks"].append(("dynamic", hdr_at))
            hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
            assert hlit <= 286 and hdist <= 30
            cl = [0] * 19
            for k in range(hclen):
                cl[CLEN_ORDER[k]] = bits(3)
            ct = _table(cl)
            lens = []
            while len(lens) < hlit + hdist:
                s, _ = sym(ct)
                if s < 16:
                    lens.append(s)
                    continue
                rep, val = (3 + bits(2), lens[-1]) if s == 16 else (3 + bits(3), 0) if s == 17 else (11 + bits(7), 0)
                if len(lens) < hlit < len(lens) + rep:
                    st["cross"] += 1
                if s == 16 and len(lens) == hlit:
                    st["at_hlit"] += 1
                lens += [val] * rep
            assert len(lens) == hlit + hdist
            ll, dl = lens[:hlit], lens[hlit:]
            lt, dt = _table(ll), _table(dl)
        while True:
            s, n = sym(lt)
            if s < 256:
                st["lit_lens"][n] += 1
                out.append(s)
                continue
            if s == 256:
                st["lit_lens"][n] += 1
                break
            assert s <= 285
            st["len_lens"][n] += 1
            L = LEN_BASE[s - 257] + bits(LEN_EXTRA[s - 257])
            ds, n = sym(dt)
            assert ds < 30
            st["dist_lens"][(ds, n)] += 1
            D = DIST_BASE[ds] + bits(DIST_EXTRA[ds])
            assert D <= len(out)
            st["max_dist"] = max(st["max_dist"], D)
            st["far"] += D > ZLIB_MAX_DIST
            if D >= L:
                out += out[len(out) - D:len(out) - D + L]
            else:
                for _ in range(L):
                    out.append(out[-D])
    return st, bytes(out)
