"""An independent restatement of Go's sequential JPEG reader (image/jpeg: reader.go, huffman.go, scan.go, idct.go) in Python / numpy,
written from ITU-T T.81 and the rules DESIGN.md section 4.6 and the oracle's comments document -- not from the oracle's C.

Scope: SOF0 / SOF1, 8-bit samples; one component (*image.Gray) or three with Y sampling (1|2) x (1|2) and chroma 1 x 1 (the
samplings the product takes); one interleaved scan or several scans (any component order, non-interleaved scans included).  What it
restates:
  marker loop      SOI; bytes that are not 0xff between segments skipped; "\\xff\\x00" and stray RSTn ignored; fill bytes; EOI required;
                   APPn / COM skipped; unknown markers malformed below 0xc0, unsupported above; a second SOF malformed
  processDQT       Pq 0 / 1 (8- or 16-bit entries), Tq 0..3, several tables per segment, a table undefined at use is all zero
  processDHT       Tc 0 / 1, Th 0..3 (0 / 1 in a SOF0 frame), several tables per segment, 1..256 codes, canonical codes (F.2.2.3)
  processSOF       component ids, (h, v) with 3 refused for any component, a single component's factors taken as (1, 1)
  processSOS       component selectors in any order, DC prediction (F.2.1.3.1), decodeHuffman, receiveExtend (F.2.2.1), the AC loop
                   (F.2.2.2) with the zig > 63 break before the magnitude bits are read, ZRL, the end-of-band run an AC symbol
                   (r < 15, s = 0) starts in a sequential scan too, restart intervals (bits and predictions reset; the RSTn has to be the
                   next two bytes, anything else -- where Go would search for it -- is "unsupported", as the oracle says)
  reconstructBlock dequantisation and idct.go in int32 arithmetic that WRAPS (Go defines overflow), the all-zero-AC row shortcut
                   included; level shift and clip into the MCU-padded planes of image.NewYCbCr / image.NewGray
Verdicts: decode() raises ValueError("malformed" | "unsupported") where the oracle does.  A result's dc_wide says that a DC value
left the int16 range (the GPU pipeline hands such files back)."""
import numpy as np

ZIG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                62, 63])


class Malformed(ValueError):
    def __init__(self, why=""):
        super().__init__("malformed" + (": " + why if why else ""))


class Unsupported(ValueError):
    def __init__(self, why=""):
        super().__init__("unsupported" + (": " + why if why else ""))


# ---- idct.go in int32 that wraps ------------------------------------------------------------------------------------------------
def i32(x):
    """x (int64 array) reduced to int32 the way two's complement arithmetic wraps"""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


W1, W2, W3, W5, W6, W7, R2 = 2841, 2676, 2408, 1609, 1108, 565, 181


def _pass(s, pre, rnd, post, out_shift):
    """one 1-D pass of the Chen-Wang transform over s[..., 0:8]; pre: the prescale shift of s0 / s4 (11, or 8), rnd: what is added to
    s0 (128, or 8192), post: rounding and shift of the odd part (0: none, 3: + 4 >> 3), out_shift: the final shift (8, or 14)"""
    s = [s[..., i] for i in range(8)]
    x0, x1 = i32(i32(s[0] << pre) + rnd), i32(s[4] << pre)
    x2, x3, x4, x5, x6, x7 = s[6], s[2], s[1], s[7], s[5], s[3]

    def odd(v):
        return i32(v) >> post if post else i32(v)
    x8 = i32(W7 * i32(x4 + x5) + (4 if post else 0))
    x4, x5 = odd(x8 + i32((W1 - W7) * x4)), odd(x8 - i32((W1 + W7) * x5))
    x8 = i32(W3 * i32(x6 + x7) + (4 if post else 0))
    x6, x7 = odd(x8 - i32((W3 - W5) * x6)), odd(x8 - i32((W3 + W5) * x7))
    x8, x0 = i32(x0 + x1), i32(x0 - x1)
    x1 = i32(W6 * i32(x3 + x2) + (4 if post else 0))
    x2, x3 = odd(x1 - i32((W2 + W6) * x2)), odd(x1 + i32((W2 - W6) * x3))
    x1, x4 = i32(x4 + x6), i32(x4 - x6)
    x6, x5 = i32(x5 + x7), i32(x5 - x7)
    x7, x8 = i32(x8 + x3), i32(x8 - x3)
    x3, x0 = i32(x0 + x2), i32(x0 - x2)
    x2 = i32(R2 * i32(x4 + x5) + 128) >> 8
    x4 = i32(R2 * i32(x4 - x5) + 128) >> 8
    out = [x7 + x1, x3 + x2, x0 + x4, x8 + x6, x8 - x6, x0 - x4, x3 - x2, x7 - x1]
    return np.stack([i32(v) >> out_shift for v in out], -1)


def idct(blocks, shortcut=True):
    """idct.go on (n, 64) int32 values in natural order -> (n, 64) int64 (int32 values); shortcut=False leaves out the row shortcut
    (what the GPU kernel once did: the tests show that the corpus tells the two apart)"""
    b = np.asarray(blocks, np.int64).reshape(-1, 8, 8)
    full = _pass(b, 11, 128, 0, 8)
    dc_only = ~np.any(b[..., 1:] != 0, axis=-1) & shortcut         # the row shortcut: seven zero AC terms -> s[0] << 3
    rows = np.where(dc_only[..., None], i32(b[..., :1] << 3), full)
    cols = _pass(np.swapaxes(rows, 1, 2), 8, 8192, 3, 14)           # the vertical pass has no shortcut
    return np.swapaxes(cols, 1, 2).reshape(-1, 64)


def reconstruct(zz, q, shortcut=True):
    """reconstructBlock: zig-zag coefficients (n, 64) and the table (64, zig-zag order) -> (n, 8, 8) uint8 pixels"""
    nat = np.zeros((len(zz), 64), np.int64)
    nat[:, ZIG] = i32(np.asarray(zz, np.int64) * np.asarray(q, np.int64))
    px = idct(nat, shortcut)
    return (np.clip(px, -128, 127) + 128).astype(np.uint8).reshape(-1, 8, 8)


# ---- huffman.go ---------------------------------------------------------------------------------------------------------------
class Table:
    def __init__(self, counts, vals):
        self.vals = list(vals)
        self.maxcode, self.mincode, self.valptr = [-1] * 17, [0] * 17, [0] * 17
        code = k = 0
        for ln in range(1, 17):
            n = counts[ln - 1]
            if n:
                self.mincode[ln], self.valptr[ln] = code, k
                self.maxcode[ln] = code + n - 1
                code += n
                k += n
            code <<= 1


class Bits:
    """the entropy-coded bits from pos on: 0xff 0x00 is a 0xff; any other 0xff xx ends the data (the decoder may not read past it)"""

    def __init__(self, data, pos):
        self.data, self.pos = data, pos
        self.acc = 0
        self.n = 0

    def bit(self):
        if self.n == 0:
            d = self.data
            if self.pos >= len(d):
                raise Malformed("short Huffman data")
            c = d[self.pos]
            if c == 0xFF:
                if self.pos + 1 >= len(d) or d[self.pos + 1] != 0:
                    raise Malformed("missing 0xff00 sequence")
                self.pos += 1
            self.pos += 1
            self.acc, self.n = c, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, t):
        v = 0
        for _ in range(t):
            v = v << 1 | self.bit()
        return v

    def huffman(self, t):
        code = 0
        for ln in range(1, 17):
            code = code << 1 | self.bit()
            if code <= t.maxcode[ln]:
                self.last_len = ln
                return t.vals[t.valptr[ln] + code - t.mincode[ln]]
        raise Malformed("bad Huffman code")

    def receive_extend(self, t):
        v = self.bits(t)
        if t and v < 1 << (t - 1):
            v += (-1 << t) + 1
        return v

    def reset(self):
        """the bit buffer is dropped (Go's d.bits = bits{}): the next read starts at the next byte"""
        self.acc = self.n = 0


# ---- the reader --------------------------------------------------------------------------------------------------------------
def decode(data, want_coefs=False, stats=None, shortcut=True):
    """Go's image.Decode of a sequential JPEG -> dict(w, h, ratio, y, cb, cr, dc_wide[, coefs]).  Planes as the oracle returns them:
    y is (8 * v0 * myy) x (8 * h0 * mxx), cb / cr (8 * myy) x (8 * mxx) (all zero for Gray, ratio 4).  coefs: per component the
    zig-zag coefficients of the last scan that coded each block, (rows, cols, 64).  stats (a set) receives what the scans exercised:
    ("dc_size", t), ("ac_size", s), ("code_len", n), "dc16_code16", "zrl_eob", "zrl_to_63", "run_past_63", "eob_run", "rst_wrap"."""
    data = bytes(data)
    if len(data) < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise Malformed("missing SOI marker")
    st = dict(shortcut=shortcut, stats=set() if stats is None else stats, quant=np.zeros((4, 64), np.int64), huff={}, ncomp=0, ri=0, jfif=False, adobe=None, planes=None, coefs=None, wide=False)
    pos = 2
    n = len(data)
    while True:
        if pos + 2 > n:
            raise Malformed("unexpected EOF")
        t0, t1 = data[pos], data[pos + 1]
        pos += 2
        while t0 != 0xFF:                                   # "libjpeg is liberal in what it accepts"
            if pos >= n:
                raise Malformed("unexpected EOF")
            t0, t1 = t1, data[pos]
            pos += 1
        marker = t1
        if marker == 0:
            continue
        while marker == 0xFF:                               # fill bytes
            if pos >= n:
                raise Malformed("unexpected EOF")
            marker = data[pos]
            pos += 1
        if marker == 0xD9:
            break
        if 0xD0 <= marker <= 0xD7:
            continue
        if pos + 2 > n:
            raise Malformed("unexpected EOF")
        ln = (data[pos] << 8 | data[pos + 1]) - 2
        pos += 2
        if ln < 0:
            raise Malformed("short segment length")
        if pos + ln > n:
            raise Malformed("unexpected EOF")
        body = data[pos:pos + ln]
        pos += ln
        if marker in (0xC0, 0xC1):
            _sof(st, body, marker == 0xC0)
        elif marker == 0xC2:
            raise Unsupported("progressive (outside this model)")
        elif marker == 0xC4:
            _dht(st, body)
        elif marker == 0xDB:
            _dqt(st, body)
        elif marker == 0xDD:
            if ln != 2:
                raise Malformed("DRI has wrong length")
            st["ri"] = body[0] << 8 | body[1]
        elif marker == 0xE0:
            if ln >= 5 and body[:5] == b"JFIF\x00":
                st["jfif"] = True
        elif marker == 0xEE:
            if ln >= 12 and body[:5] == b"Adobe":
                st["adobe"] = body[11]
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass
        elif marker == 0xDA:
            pos = _sos(st, data, body, pos)
        elif marker < 0xC0:
            raise Malformed("unknown marker")
        else:
            raise Unsupported("unknown marker")
    if st["planes"] is None:
        raise Malformed("missing SOS marker")
    if st["ncomp"] == 3 and not st["jfif"] and (st["adobe"] == 0 or st["ids"] == [ord("R"), ord("G"), ord("B")]):
        raise Unsupported("RGB")
    y, cb, cr = st["planes"]
    out = dict(w=st["w"], h=st["h"], ratio=st["ratio"], y=y, cb=cb, cr=cr, dc_wide=st["wide"])
    if want_coefs:
        out["coefs"] = st["coefs"]
    return out


def _sof(st, b, baseline):
    if st["ncomp"]:
        raise Malformed("multiple SOF markers")
    if len(b) not in (9, 15, 18):
        raise Unsupported("number of components")
    if len(b) == 18:
        raise Unsupported("CMYK")
    nc = 1 if len(b) == 9 else 3
    if b[0] != 8:
        raise Unsupported("precision")
    h, w = b[1] << 8 | b[2], b[3] << 8 | b[4]
    if b[5] != nc:
        raise Malformed("SOF has wrong length")
    ids, hv, tq = [], [], []
    for i in range(nc):
        cid, f, q = b[6 + 3 * i], b[7 + 3 * i], b[8 + 3 * i]
        if cid in ids:
            raise Malformed("repeated component identifier")
        if q > 3:
            raise Malformed("bad Tq value")
        ch, cv = f >> 4, f & 15
        if not (1 <= ch <= 4 and 1 <= cv <= 4):
            raise Malformed("sampling factor")
        if ch == 3 or cv == 3:
            raise Unsupported("sampling factor of 3")
        ids.append(cid)
        hv.append((1, 1) if nc == 1 else (ch, cv))
        tq.append(q)
    if nc == 3 and (hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0][0] > 2 or hv[0][1] > 2):
        raise Unsupported("sampling outside 4:4:4 / 4:4:0 / 4:2:2 / 4:2:0")
    if w <= 0 or h <= 0:
        raise Malformed("empty frame")
    h0, v0 = hv[0]
    st.update(ncomp=nc, w=w, h=h, ids=ids, hv=hv, tq=tq, baseline=baseline,
              mxx=(w + 8 * h0 - 1) // (8 * h0), myy=(h + 8 * v0 - 1) // (8 * v0),
              ratio=4 if nc == 1 else {(1, 1): 0, (2, 1): 1, (2, 2): 2, (1, 2): 3}[(h0, v0)])


def _dht(st, b):
    k = 0
    while k < len(b):
        if len(b) - k < 17:
            raise Malformed("DHT has wrong length")
        tc, th = b[k] >> 4, b[k] & 15
        if tc > 1 or th > 3 or (st.get("baseline") and th > 1):
            raise Malformed("bad Tc / Th value")
        counts = list(b[k + 1:k + 17])
        total = sum(counts)
        if total == 0 or total > 256:
            raise Malformed("Huffman table length")
        if k + 17 + total > len(b):
            raise Malformed("DHT has wrong length")
        st["huff"][tc, th] = Table(counts, b[k + 17:k + 17 + total])
        k += 17 + total


def _dqt(st, b):
    k = 0
    while k < len(b):
        pq, tq = b[k] >> 4, b[k] & 15
        if tq > 3 or pq > 1:
            raise Malformed("bad Pq / Tq value")
        need = 128 if pq else 64
        if k + 1 + need > len(b):
            raise Malformed("DQT has wrong length")
        raw = np.frombuffer(b[k + 1:k + 1 + need], ">u2" if pq else np.uint8)
        st["quant"][tq] = raw.astype(np.int64)
        k += 1 + need


def _sos(st, data, b, pos):
    """one scan: decodes and reconstructs its blocks; returns the position after the last byte the entropy decoder used"""
    nc = st["ncomp"]
    if not nc:
        raise Malformed("missing SOF marker")
    if len(b) < 6 or len(b) > 4 + 2 * nc or len(b) % 2:
        raise Malformed("SOS has wrong length")
    ns = b[0]
    if len(b) != 4 + 2 * ns:
        raise Malformed("SOS length inconsistent")
    sel = []
    for i in range(ns):
        cs = b[1 + 2 * i]
        if cs not in st["ids"]:
            raise Malformed("unknown component selector")
        c = st["ids"].index(cs)
        if c in [s[0] for s in sel]:
            raise Malformed("repeated component selector")
        td, ta = b[2 + 2 * i] >> 4, b[2 + 2 * i] & 15
        if td > 3 or ta > 3 or (st["baseline"] and (td > 1 or ta > 1)):
            raise Malformed("bad Td / Ta value")
        sel.append((c, td, ta))
    if nc > 1 and sum(st["hv"][c][0] * st["hv"][c][1] for c, _, _ in sel) > 10:
        raise Malformed("total sampling factors too large")
    mxx, myy = st["mxx"], st["myy"]
    if st["planes"] is None:
        h0, v0 = st["hv"][0]
        st["planes"] = [np.zeros((8 * v0 * myy, 8 * h0 * mxx), np.uint8), np.zeros((8 * myy, 8 * mxx), np.uint8),
                        np.zeros((8 * myy, 8 * mxx), np.uint8)]
        st["coefs"] = [np.zeros((myy * st["hv"][c][1], mxx * st["hv"][c][0], 64), np.int64) for c in range(nc)]
    # the blocks in scan order (as jpeg_writer.Frame.order, restated: interleaved MCU by MCU; non-interleaved row by row over the
    # component's grid, blocks wholly outside the image skipped)
    order = []
    if ns == 1:
        c = sel[0][0]
        hi, vi = st["hv"][c]
        q = mxx * hi
        for m in range(mxx * myy):
            for j in range(hi * vi):
                cnt = m * hi * vi + j
                bx, by = cnt % q, cnt // q
                if bx * 8 < st["w"] and by * 8 < st["h"]:
                    order.append((m, 0, by, bx))
    else:
        for my in range(myy):
            for mx in range(mxx):
                for i, (c, _, _) in enumerate(sel):
                    hi, vi = st["hv"][c]
                    for j in range(hi * vi):
                        order.append((my * mxx + mx, i, vi * my + j // hi, hi * mx + j % hi))
    tabs = []
    for c, td, ta in sel:
        if (0, td) not in st["huff"] or (1, ta) not in st["huff"]:
            raise Malformed("uninitialized Huffman table")
        tabs.append((st["huff"][0, td], st["huff"][1, ta]))
    br = Bits(data, pos)
    dc = [0, 0, 0]
    eobrun = 0
    ri, nmcu = st["ri"], mxx * myy
    rst = 0xD0
    done = -1                                         # MCUs finished
    got = {c: [] for c, _, _ in sel}                  # per component: [(by, bx, zig-zag coefficients)]

    def restart_after(m):
        nonlocal rst, eobrun
        if ri and (m + 1) % ri == 0 and m + 1 < nmcu:
            br.reset()
            p = br.pos
            if p + 2 > len(data):
                raise Malformed("unexpected EOF")
            if data[p] != 0xFF or data[p + 1] != rst:
                raise Unsupported("restart marker not where it belongs (Go's findRST)")
            br.pos = p + 2
            if rst == 0xD7:
                st["stats"].add("rst_wrap")
            rst = 0xD0 if rst == 0xD7 else rst + 1
            dc[0] = dc[1] = dc[2] = 0
            eobrun = 0

    for m, i, by, bx in order:
        while done < m - 1:
            done += 1
            restart_after(done)
        c = sel[i][0]
        dct, act = tabs[i]
        zz = np.zeros(64, np.int64)
        t = br.huffman(dct)
        stats = st["stats"]
        stats.add(("dc_size", t))
        stats.add(("code_len", br.last_len))
        if t == 16 and br.last_len == 16:
            stats.add("dc16_code16")
        if t > 16:
            raise Unsupported("excessive DC component")
        dc[c] = int(i32(np.int64(dc[c] + br.receive_extend(t))))
        if not -32768 <= dc[c] <= 32767:
            st["wide"] = True
        zz[0] = dc[c]
        if eobrun > 0:
            eobrun -= 1
        else:
            zig, prev = 1, None
            while zig <= 63:
                v = br.huffman(act)
                stats.add(("code_len", br.last_len))
                r, s = v >> 4, v & 15
                if s:
                    stats.add(("ac_size", s))
                    zig += r
                    if zig > 63:
                        stats.add("run_past_63")
                        break                          # the magnitude bits are not read
                    zz[zig] = br.receive_extend(s)
                elif r == 15:
                    zig += 15
                    if zig == 63:
                        stats.add("zrl_to_63")
                else:
                    if prev == 0xF0 and r == 0:
                        stats.add("zrl_eob")
                    if r:
                        stats.add("eob_run")
                    eobrun = (1 << r) | (br.bits(r) if r else 0)
                    eobrun -= 1
                    break
                prev = v
                zig += 1
        got[c].append((by, bx, zz))
        done = max(done, m - 1)
    while done < nmcu - 2:                             # markers still due after the last block (MCUs with no blocks of this scan)
        done += 1
        restart_after(done)
    for c, blocks in got.items():
        if not blocks:
            continue
        zz = np.stack([b[2] for b in blocks])
        px = reconstruct(zz, st["quant"][st["tq"][c]], st["shortcut"])
        plane = st["planes"][c]
        for (by, bx, z), p in zip(blocks, px):
            st["coefs"][c][by, bx] = z
            plane[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = p
    br.reset()
    return br.pos
