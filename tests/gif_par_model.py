"""The parallel code walk of a GIF's LZW data (csrc/ipx_gif_dec_par.hip, IPX_GIF_PAR=1) as numpy, round by round, beside a plain
restatement of the serial walk (gif_walk_kernel) and of the expansion (gif_expand_kernel) over the records both write.

Between two clear codes the reader's code width depends only on how many codes it has read since the clear: at ordinal t of a segment
(t = 0: the first code after the clear, or the first code of the data) hi = eof + t, so the code is min(12, bitlen(eof + t)) bits wide
and its bit offset inside the segment is a closed form of t and lit (bits_before).  A round reads LANES consecutive ordinals at once;
the first lane, in lane order, that holds a clear code, the EOF code, a code whose bits run past the data or a broken rule ends the
round's valid prefix.  A code eof + j (1 <= j <= t; j == t is KwKwK) is the string of ordinal j - 1 plus one byte: L[t] = L[j - 1] + 1,
first[t] = first[j - 1]; a literal has L = 1 and first = its value.  Ordinals before the round are looked up, the others resolved by six
pointer-jumping steps; a prefix sum of L gives the offsets.  Once eof + t > 4095 the table is full: no entry is added, every 12-bit
code is valid, and the recurrence reads ordinals <= 4094 - eof only.

The parallel walk accepts a file only at an EOF code with count == w * h and blockReader.close's rule; everything else is `redo`
(the serial walk's).  A helper of the tests only."""
import numpy as np

import gif_decode_model as dm

LANES = 64
STEPS = 6          # pointer-jumping steps: 2 ** 6 - 1 = 63 hops, the longest chain 64 lanes hold


def bitlen(x):
    return int(x).bit_length()


def width(t, lit):
    return min(12, max(lit + 1, bitlen((1 << lit) + 1 + t)))


def bits_before(t, lit):
    """the bits of ordinals 0 .. t - 1: width lit + 1 serves the first clear - 1 ordinals, a width x above it the 1 << (x - 1) ordinals
    from (1 << (x - 1)) - eof on, width 12 every one from 2048 - eof on; sum of x << (x - 1) over x <= b is ((b - 1) << b) + 1"""
    clear = 1 << lit
    eof = clear + 1
    w = width(t, lit)
    if w == lit + 1:
        return w * t
    below = (lit + 1) * (clear - 1) + (((w - 2) << (w - 1)) + 1) - ((lit << (lit + 1)) + 1)
    return below + w * (t - ((1 << (w - 1)) - eof))


def _v_width(t, lit):
    x = ((1 << lit) + 1 + t).astype(np.int64)
    return np.minimum(12, np.floor(np.log2(x)).astype(np.int64) + 1)


def _v_bits_before(t, lit):
    clear, eof = 1 << lit, (1 << lit) + 1
    w = _v_width(t, lit)
    below = (lit + 1) * (clear - 1) + (((w - 2) << (w - 1)) + 1) - ((lit << (lit + 1)) + 1)
    return np.where(w == lit + 1, w * t, below + w * (t - ((1 << (w - 1)) - eof)))


class Stream:
    """what the host hands the walk for one file (GifDecDesc): the LZW bytes, their sub-block framing, the frame"""
    def __init__(self, data, lit, w, h, pal_len, sizes, terminated, interlaced=False):
        self.data, self.lit, self.w, self.h, self.pal_len = bytes(data), lit, w, h, min(pal_len, 256)
        self.terminated, self.interlaced = terminated, interlaced
        self.last_start = sum(sizes[:-1]) if sizes else 0
        self.last_is_one = bool(sizes) and sizes[-1] == 1
        self.code_cap = min(8 * len(self.data) // (lit + 1), w * h) + 1

    def close_ok(self, used):
        return self.terminated and (used > self.last_start or (used == self.last_start and self.last_is_one))


def stream_of(file):
    """the Stream of a file whose container parses (dm.decode(file)["stage"] != "container"), as gif_parse and gif_gather cut it"""
    d = bytes(file)
    p = 13
    glen = 0
    if d[10] & 0x80:
        glen = 1 << (1 + (d[10] & 7))
        p += 3 * glen
    trans = None
    while d[p] != 0x2C:
        label = d[p + 1]
        p += 2
        if label == 0xF9:
            if d[p + 1] & 1:
                trans = d[p + 4]
            p += 6
            continue
        if label == 0x01:
            p += 13
        elif label == 0xFF:
            p += 1 + d[p]
        while d[p]:
            p += 1 + d[p]
        p += 1
    w, h, fields = d[p + 5] | d[p + 6] << 8, d[p + 7] | d[p + 8] << 8, d[p + 9]
    p += 10
    pal_len = glen
    if fields & 0x80:
        pal_len = 1 << (1 + (fields & 7))
        p += 3 * pal_len
    if trans is not None:
        pal_len = max(pal_len, trans + 1)
    lit = d[p]
    r = dm._Reader(d)
    r.p = p + 1
    data, sizes, terminated = dm.read_sub_blocks(r)
    return Stream(data, lit, w, h, pal_len, sizes, terminated, bool(fields & 0x40))


class Walk:
    """status 0 (accepted), 1 (Go's reader fails) or 2 (scratch); how: "eof", "end" (accepted without an EOF code) or why not;
    records [(off, segb, packed)], count; for the parallel walk redo / why and the rounds it took.  A lane's kind: 0 a code that
    outputs bytes, 1 a clear code, 2 the EOF code, 3 bits past the data, 4 a broken rule."""
    def __init__(self):
        self.status, self.how, self.records, self.count = 1, "", [], 0
        self.redo, self.rounds, self.trace = False, 0, []      # trace: per round (t0, valid lanes, what ended it, every lane's kind)


def serial_walk(s):
    """gif_walk_kernel, line by line"""
    out = Walk()
    lit, data = s.lit, s.data
    clear, eof, npix, nbits = 1 << lit, (1 << lit) + 1, s.w * s.h, 8 * len(s.data)
    s_len, s_first = [0] * 4096, [0] * 4096
    bit, wd, hi, overflow = 0, lit + 1, eof, 1 << (lit + 1)
    have_last, last, last_len, last_first, count, k, segb = False, 0, 0, 0, 0, 0, 0
    rec = out.records

    def end(st, how):
        out.status, out.how, out.count = st, how, count
        return out

    while True:
        if bit + wd > nbits:
            return end(0 if s.terminated and count == npix else 1, "end")
        v = (int.from_bytes(data[bit >> 3:(bit >> 3) + 3], "little") >> (bit & 7)) & ((1 << wd) - 1)
        bit += wd
        if v == clear:
            wd, hi, overflow, have_last, segb = lit + 1, eof, 1 << (lit + 1), False, k
            continue
        if v == eof:
            return end(0 if count == npix and s.close_ok((bit + 7) >> 3) else 1, "eof")
        if v < clear:
            if v >= s.pal_len:
                return end(1, "pixel value")
            L, f = 1, v
        elif v < hi or (v == hi and not have_last):
            L, f = s_len[v], s_first[v]
        elif v == hi:
            L, f = last_len + 1, last_first
        else:
            return end(1, "invalid code")
        if L > npix - count:
            return end(1, "too much")
        if k + 1 >= s.code_cap:
            return end(2, "scratch")
        rec.append((count, segb, v | (last if have_last else 0) << 12 | f << 24))
        if have_last:
            s_len[hi], s_first[hi] = last_len + 1, last_first
        count += L
        k += 1
        have_last, last, last_len, last_first = True, v, L, f
        hi += 1
        if hi >= overflow:
            if wd == 12:
                have_last = False
                hi -= 1
            else:
                wd += 1
                overflow <<= 1


def par_walk(s):
    """gif_walk_par_kernel, round by round"""
    out = Walk()
    lit = s.lit
    clear, eof, npix, nbits = 1 << lit, (1 << lit) + 1, s.w * s.h, 8 * len(s.data)
    keep = 4095 - eof
    buf = np.frombuffer(s.data + bytes(8), np.uint8).astype(np.int64)
    s_len, s_first = np.zeros(4096, np.int64), np.zeros(4096, np.int64)
    bit0, t0, k, segb, count, prev_v = 0, 0, 0, 0, 0, 0
    lanes = np.arange(LANES)

    def redo(why):
        out.redo, out.how, out.records, out.count = True, why, [], 0
        return out

    for _ in range(nbits // (lit + 1) + 2):
        out.rounds += 1
        t = t0 + lanes
        w = _v_width(t, lit)
        pos = bit0 + _v_bits_before(t, lit)
        fits = pos + w <= nbits
        o = np.minimum(pos >> 3, len(buf) - 3)                   # (lanes past the data read nothing they decide on)
        v = ((buf[o] | buf[o + 1] << 8 | buf[o + 2] << 16) >> (pos & 7)) & ((1 << w) - 1)
        frozen = eof + t > 4095
        bad = np.where(v < clear, v >= s.pal_len, ~frozen & (v - eof > t))
        kind = np.where(~fits, 3, np.where(v == clear, 1, np.where(v == eof, 2, np.where(bad, 4, 0))))
        stops = np.nonzero(kind)[0]
        nvalid = int(stops[0]) if len(stops) else LANES
        stop = int(kind[nvalid]) if nvalid < LANES else 0
        valid = lanes < nvalid
        out.trace.append((t0, nvalid, stop, kind))
        L, F, ptr = np.where(valid, 1, 0), v & 255, lanes.copy()
        ref = valid & (v > eof)
        dep = np.where(ref, v - eof - 1, 0)
        old = ref & (dep < t0)
        L[old], F[old] = s_len[dep[old]] + 1, s_first[dep[old]]
        ptr[ref & ~old] = dep[ref & ~old] - t0
        assert (ptr <= lanes).all() and (ptr[ref & ~old] < lanes[ref & ~old]).all()
        for _ in range(STEPS):
            pl, pf, pp = L[ptr], F[ptr], ptr[ptr]
            un = ptr != lanes
            L = np.where(un, L + pl, L)
            hit = un & (pp == ptr)
            F = np.where(hit, pf, F)
            ptr = np.where(hit, lanes, np.where(un, pp, ptr))
        assert (ptr == lanes).all()
        incl = np.cumsum(L)
        if (valid & (incl > npix - count)).any():
            return redo("too much")
        if nvalid and k + nvalid >= s.code_cap:
            return redo("scratch")
        tv = t[valid]
        s_len[tv[tv < keep]], s_first[tv[tv < keep]] = L[valid][tv < keep], F[valid][tv < keep]
        for i in range(nvalid):
            prev = 0 if t[i] == 0 or frozen[i] else (prev_v if i == 0 else int(v[i - 1]))
            out.records.append((count + int(incl[i] - L[i]), segb, int(v[i]) | prev << 12 | int(F[i]) << 24))
        if nvalid:
            prev_v = int(v[nvalid - 1])
        count += int(incl[-1])
        k += nvalid
        t0 += nvalid
        if stop == 0:
            continue
        end_bit = bit0 + bits_before(t0, lit) + width(t0, lit)
        if stop == 1:
            bit0, t0, segb = end_bit, 0, k
            continue
        if stop == 2:
            if count == npix and s.close_ok((end_bit + 7) >> 3):
                out.status, out.how, out.count = 0, "eof", count
                return out
            return redo("early or unclosed EOF code")
        return redo("data end" if stop == 3 else "invalid code or pixel value")
    return redo("round bound")


def expand(s, records, count):
    """gif_expand_kernel: every record's string written backwards along the entry -> ordinal map of its segment -> h x w frame"""
    clear, eof, npix = 1 << s.lit, (1 << s.lit) + 1, s.w * s.h
    pix = np.zeros(npix, np.uint8)
    offs = [r[0] for r in records] + [count]
    for k, (off, segb, packed) in enumerate(records):
        pos, v = offs[k + 1] - 1, packed & 4095
        while True:
            if v < clear:
                pix[pos] = v
                break
            p = records[segb + (v - eof)][2]
            pix[pos] = p >> 24
            if pos == off:
                break
            pos, v = pos - 1, (p >> 12) & 4095
    return dm.uninterlace(pix, s.w, s.h) if s.interlaced else pix.reshape(s.h, s.w)
