"""png.Decode restated (image/png reader.go, compress/zlib, compress/flate), the model the GPU decoder (csrc/ipx_png_dec.hip) is
held to byte for byte.  PARITY UNPINNED: Go cannot run here, so the rules are restated from memory; every case whose Go behaviour is
not restated with confidence answers UNSUPPORTED (the worker then decodes the file with Go), and the list is in DESIGN.md section 4.10.

decode(data) -> dict(status, stage, kind, w, h, pix, palette, why):
  status  OK / INVALID / UNSUPPORTED for the file on its own
  stage   "container" when the chunk headers decide the status (the host parse), "data" when the CRCs, the zlib stream or the rows do
  pix     Go's Pix for the type Go returns, h x (w * bytes per pixel) uint8 (OK only)
  palette 256 x 4 uint8 (R, G, B, A) for PALETTED: tRNS entries non-premultiplied, entries past PLTE opaque black
inflate(data, limit) is the pure-Python inflater; decode(..., fast=True) takes zlib.decompress for the stream instead (valid streams
only: the large frames of the GPU tests)."""
import struct
import zlib

import numpy as np

OK, INVALID, UNSUPPORTED = 0, -1, -4
GRAY, NRGBA, RGBA, PALETTED, GRAY16, RGBA64, NRGBA64 = range(7)
BPP = (1, 4, 4, 1, 2, 8, 8)
SIG = b"\x89PNG\r\n\x1a\n"
LEGAL = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
MAX_SPAN = 0x7FFF0000


class FlateError(Exception):
    pass


# ---- compress/flate ------------------------------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k // 2 - 1 for k in range(4, 30)]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def go_huffman_ok(lengths):
    """huffmanDecoder.init's verdict: complete, or empty, or exactly one code of length 1"""
    nz = [n for n in lengths if n]
    if not nz:
        return True
    mn, mx = min(nz), max(nz)
    code = 0
    for L in range(mn, mx + 1):
        code = (code << 1) + nz.count(L)
    return code == 1 << mx or (code == 1 and mx == 1)


def canonical(lengths):
    """{(length, code): symbol} of the canonical code"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for L in range(1, 16):
        code = (code + count[L - 1]) << 1
        nxt[L] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[(n, nxt[n])] = s
            nxt[n] += 1
    return out


class Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0          # pos in bits

    def bit(self):
        if self.pos >= 8 * len(self.d):
            raise FlateError("unexpected EOF")
        b = (self.d[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for k in range(n):
            v |= self.bit() << k
        return v

    def sym(self, table):
        code = 0
        for L in range(1, 16):
            code = (code << 1) | self.bit()
            s = table.get((L, code))
            if s is not None:
                return s
        raise FlateError("invalid code")


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)


def inflate(data, limit):
    """zlib stream -> (decompressed bytes, offset of the first byte after the Adler-32).  FlateError on every rule of Go's reader;
    more than `limit` bytes out is an error too ("too much pixel data")."""
    if len(data) < 2:
        raise FlateError("zlib: unexpected EOF")
    cmf, flg = data[0], data[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31:
        raise FlateError("zlib: invalid header")
    if flg & 0x20:
        raise FlateError("zlib: invalid dictionary")
    br = Bits(data)
    br.pos = 16
    out = bytearray()
    final = False
    while not final:
        final = br.bits(1)
        t = br.bits(2)
        if t == 0:
            br.pos = (br.pos + 7) & ~7
            p = br.pos >> 3
            if p + 4 > len(data):
                raise FlateError("unexpected EOF")
            n, nn = data[p] | data[p + 1] << 8, data[p + 2] | data[p + 3] << 8
            if n != (~nn & 0xFFFF):
                raise FlateError("stored length")
            if p + 4 + n > len(data):
                raise FlateError("unexpected EOF")
            if len(out) + n > limit:
                raise FlateError("too much pixel data")
            out += data[p + 4:p + 4 + n]
            br.pos = 8 * (p + 4 + n)
            continue
        if t == 3:
            raise FlateError("block type 3")
        if t == 1:
            lit, dist = FIXED_LIT, FIXED_DIST
        else:
            hlit, hdist, hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
            if hlit > 286 or hdist > 30:
                raise FlateError("HLIT / HDIST")
            cl = [0] * 19
            for k in range(hclen):
                cl[CLEN_ORDER[k]] = br.bits(3)
            if not go_huffman_ok(cl):
                raise FlateError("code length code")
            ct = canonical(cl)
            lens = []
            n = hlit + hdist
            while len(lens) < n:
                s = br.sym(ct)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16:
                    if not lens:
                        raise FlateError("repeat at the first position")
                    rep, val = 3 + br.bits(2), lens[-1]
                elif s == 17:
                    rep, val = 3 + br.bits(3), 0
                else:
                    rep, val = 11 + br.bits(7), 0
                if len(lens) + rep > n:
                    raise FlateError("repeat past HLIT + HDIST")
                lens += [val] * rep
            if not go_huffman_ok(lens[:hlit]) or not go_huffman_ok(lens[hlit:]):
                raise FlateError("incomplete code")
            lit, dist = canonical(lens[:hlit]), canonical(lens[hlit:])
        while True:
            s = br.sym(lit)
            if s < 256:
                if len(out) >= limit:
                    raise FlateError("too much pixel data")
                out.append(s)
            elif s == 256:
                break
            elif s > 285:
                raise FlateError("length symbol 286 / 287")
            else:
                L = LEN_BASE[s - 257] + br.bits(LEN_EXTRA[s - 257])
                ds = br.sym(dist)
                if ds >= 30:
                    raise FlateError("distance code 30 / 31")
                D = DIST_BASE[ds] + br.bits(DIST_EXTRA[ds])
                if D > len(out):
                    raise FlateError("distance too far back")
                if len(out) + L > limit:
                    raise FlateError("too much pixel data")
                for _ in range(L):
                    out.append(out[-D])
    p = (br.pos + 7) >> 3
    if p + 4 > len(data):
        raise FlateError("unexpected EOF")
    if struct.unpack(">I", data[p:p + 4])[0] != zlib.adler32(bytes(out)):
        raise FlateError("zlib: invalid checksum")
    return bytes(out), p + 4


# ---- image/png -----------------------------------------------------------------------------------------------------------------
def parse(data):
    """the chunk walk (the host half): (status, fields); fields: w, h, depth, ctype, plte (entries), trns (bytes), idat (payload list),
    crc (list of (type + data, stored crc))"""
    f = {"crc": [], "idat": [], "plte": None, "trns": None, "w": 0, "h": 0, "depth": 0, "ctype": 0}
    if len(data) < 8 or data[:8] != SIG:
        return INVALID, f
    stage, i, last_idat = "start", 8, False
    while True:
        if len(data) - i < 12:
            return INVALID, f
        n = struct.unpack(">I", data[i:i + 4])[0]
        if n > len(data) - i - 12:
            return INVALID, f
        t, d = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        f["crc"].append((data[i + 4:i + 8 + n], struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0]))
        was_idat, last_idat = last_idat, False
        ct, dep = f["ctype"], f["depth"]
        if t == b"IHDR":
            if stage != "start" or n != 13:
                return INVALID, f
            w, h, dep, ct, comp, filt, il = struct.unpack(">iiBBBBB", d)
            f.update(w=w, h=h, depth=dep, ctype=ct)
            if comp or filt or il > 1 or w <= 0 or h <= 0 or dep not in LEGAL.get(ct, ()):
                return INVALID, f
            if il:
                return UNSUPPORTED, f
            stage = "IHDR"
        elif stage == "start":
            return (INVALID if t in (b"PLTE", b"tRNS", b"IDAT", b"IEND") else UNSUPPORTED), f
        elif t == b"PLTE":
            np_ = n // 3
            if stage != "IHDR" or n % 3 or not 0 < np_ <= 256 or (dep < 16 and np_ > 1 << dep) or ct in (0, 4):
                return INVALID, f
            if ct == 3:
                f["plte"] = d
            stage = "PLTE"
        elif t == b"tRNS":
            if ct in (4, 6):
                return INVALID, f
            if ct == 3:
                if stage != "PLTE" or n > 256:
                    return INVALID, f
                if n > len(f["plte"]) // 3:
                    return UNSUPPORTED, f
            else:
                if stage == "PLTE":
                    return UNSUPPORTED, f
                if stage != "IHDR" or n != (2 if ct == 0 else 6):
                    return INVALID, f
                vals = struct.unpack(">%dH" % (n // 2), d)
                if dep < 16 and any(v >= 1 << dep for v in vals):
                    return UNSUPPORTED, f
                if ct == 0 and dep < 8:
                    return UNSUPPORTED, f
            f["trns"] = d
            stage = "tRNS"
        elif t == b"IDAT":
            if ct == 3 and f["plte"] is None:
                return INVALID, f
            if stage == "IDAT" and not was_idat:
                return UNSUPPORTED, f
            f["idat"].append(d)
            stage, last_idat = "IDAT", True
        elif t == b"IEND":
            if stage != "IDAT" or n:
                return INVALID, f
            return OK, f
        elif not t[0] & 0x20:
            return UNSUPPORTED, f
        i += 12 + n


def kind_of(ctype, depth, trns):
    if ctype == 3:
        return PALETTED
    if ctype in (4, 6):
        return NRGBA64 if depth == 16 else NRGBA
    if ctype == 0:
        return (NRGBA64 if trns else GRAY16) if depth == 16 else (NRGBA if trns else GRAY)
    return (NRGBA64 if trns else RGBA64) if depth == 16 else (NRGBA if trns else RGBA)


def geometry(ctype, depth, w):
    bits = CHANNELS[ctype] * depth
    return max(1, bits // 8), 1 + (bits * w + 7) // 8          # filter bytes per pixel, row bytes with the filter byte


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def unfilter(raw, h, rowbytes, bpp):
    """-> h x (rowbytes - 1) uint8, or None on a filter type above 4"""
    out = np.zeros((h, rowbytes - 1), np.uint8)
    prev = [0] * (rowbytes - 1)
    for y in range(h):
        ft = raw[y * rowbytes]
        cur = list(raw[y * rowbytes + 1:(y + 1) * rowbytes])
        if ft > 4:
            return None
        for x in range(len(cur)):
            a = cur[x - bpp] if x >= bpp else 0
            b = prev[x]
            c = prev[x - bpp] if x >= bpp else 0
            if ft == 1:
                cur[x] = (cur[x] + a) & 255
            elif ft == 2:
                cur[x] = (cur[x] + b) & 255
            elif ft == 3:
                cur[x] = (cur[x] + ((a + b) >> 1)) & 255
            elif ft == 4:
                cur[x] = (cur[x] + paeth(a, b, c)) & 255
        out[y] = cur
        prev = cur
    return out


def convert(rows, ctype, depth, w, h, trns):
    """unfiltered rows -> Go's Pix for the type readImagePass builds"""
    if depth < 8:
        ppb = 8 // depth
        bits = np.unpackbits(rows, axis=1) if depth == 1 else None
        if depth == 1:
            v = bits[:, :w]
        else:
            shifts = np.array([8 - depth * (j + 1) for j in range(ppb)], np.uint8)
            v = ((rows[:, :, None] >> shifts[None, None, :]) & ((1 << depth) - 1)).reshape(h, -1)[:, :w]
        return (v * (255 // ((1 << depth) - 1))).astype(np.uint8) if ctype == 0 else v.astype(np.uint8)
    if depth == 8:
        if ctype == 3:
            return rows.copy()
        if ctype == 0:
            if not trns:
                return rows.copy()
            a = np.where(rows == trns[1], 0, 255).astype(np.uint8)
            return np.stack([rows, rows, rows, a], -1).reshape(h, w * 4)
        if ctype == 4:
            p = rows.reshape(h, w, 2)
            return np.stack([p[..., 0], p[..., 0], p[..., 0], p[..., 1]], -1).reshape(h, w * 4)
        if ctype == 6:
            return rows.copy()
        p = rows.reshape(h, w, 3)
        a = np.full((h, w), 255, np.uint8)
        if trns:
            m = (p[..., 0] == trns[1]) & (p[..., 1] == trns[3]) & (p[..., 2] == trns[5])
            a[m] = 0
        return np.concatenate([p, a[..., None]], -1).reshape(h, w * 4)
    # 16-bit: big-endian samples as stored
    if ctype == 0:
        if not trns:
            return rows.copy()
        p = rows.reshape(h, w, 2)
        y = p[..., 0].astype(np.uint16) << 8 | p[..., 1]
        a = np.where(y == (trns[0] << 8 | trns[1]), 0, 255).astype(np.uint8)
        return np.concatenate([p, p, p, a[..., None], a[..., None]], -1).reshape(h, w * 8)
    if ctype == 4:
        p = rows.reshape(h, w, 4)
        return np.concatenate([p[..., :2], p[..., :2], p[..., :2], p[..., 2:]], -1).reshape(h, w * 8)
    if ctype == 6:
        return rows.copy()
    p = rows.reshape(h, w, 6)
    a = np.full((h, w, 2), 255, np.uint8)
    if trns:
        m = np.all(p == np.frombuffer(trns, np.uint8)[None, None, :], axis=-1)
        a[m] = 0
    return np.concatenate([p, a], -1).reshape(h, w * 8)


def palette(f):
    pal = np.zeros((256, 4), np.uint8)
    pal[:, 3] = 255
    e = np.frombuffer(f["plte"], np.uint8).reshape(-1, 3)
    pal[:len(e), :3] = e
    if f["trns"]:
        pal[:len(f["trns"]), 3] = np.frombuffer(f["trns"], np.uint8)
    return pal


def decode(data, fast=False):
    data = bytes(data)
    st, f = parse(data)
    r = {"status": st, "stage": "container", "kind": None, "w": f["w"], "h": f["h"], "pix": None, "palette": None, "why": None}
    if st != OK:
        return r
    ct, dep, w, h = f["ctype"], f["depth"], f["w"], f["h"]
    r["kind"] = kind = kind_of(ct, dep, f["trns"] is not None)
    bpp, rowbytes = geometry(ct, dep, w)
    kb = BPP[kind]
    if w > 65535 or h > 65535 or (h - 1) * w * kb + w * kb > MAX_SPAN or h * rowbytes >= 1 << 32:
        r["status"] = UNSUPPORTED
        return r
    r["stage"] = "data"
    if any(zlib.crc32(body) != crc for body, crc in f["crc"]):
        r.update(status=INVALID, why="crc")
        return r
    stream = b"".join(f["idat"])
    limit = h * rowbytes
    if fast:
        d = zlib.decompressobj()
        raw = d.decompress(stream)
        assert d.eof and len(raw) == limit, "fast=True takes valid streams only"
        end = len(stream) - len(d.unused_data)
    else:
        try:
            raw, end = inflate(stream, limit)
        except FlateError as e:
            r.update(status=INVALID, why=str(e))
            return r
        if len(raw) != limit:
            r.update(status=INVALID, why="not enough pixel data")
            return r
    rows = unfilter(raw, h, rowbytes, bpp)
    if rows is None:
        r.update(status=INVALID, why="bad filter type")
        return r
    if end != len(stream) or len(stream) - len(f["idat"][-1]) >= end:
        r.update(status=UNSUPPORTED, why="bytes or an IDAT chunk after the Adler-32")
        return r
    r["pix"] = convert(rows, ct, dep, w, h, f["trns"])
    if kind == PALETTED:
        r["palette"] = palette(f)
    return r


def entry_status(r, size=None, kind=None):
    """the status ipx_png_decode_batch gives the file in a batch of this size and kind (None: the first decodable file's)"""
    if r["status"] != OK and r["stage"] == "container":
        return r["status"]
    if size is not None and (r["w"], r["h"]) != tuple(size):
        return UNSUPPORTED
    if kind is not None and r["kind"] != kind:
        return UNSUPPORTED
    return r["status"]
