"""gif.Encode(w, *image.RGBA, nil) restated in Python: the model the GPU GIF encoder is held to.

PARITY UNPINNED against Go itself (no toolchain): this restates Go 1.24's image/color/palette (gen.go: Plan9),
image/draw (drawPaletted with Floyd-Steinberg), compress/lzw (writer.go, LSB order, literal width 8) and image/gif
(writer.go: Encode, writeHeader, writeImageBlock, blockWriter) as read, not run.  What pins it here: Pillow decodes
every stream to the model's indices and to the Plan 9 colours, and the hand-derived known answers of
tests/golden/gif_kats.json.  A helper of the tests only: the product never imports it.

Two forms of the dither:
  * dither_scalar -- drawPaletted line by line (per-pixel Python over the palette: small frames only);
  * dither_wavefront -- the same arithmetic over anti-diagonals t = x + 2y, vectorised with numpy.  Pixel (x, y) needs
    (x-1, y) and (x-1 .. x+1, y-1), which all lie on earlier diagonals; every error term is an int32 sum, so the order of
    the adds cannot change a result, and the truncating division by 16 happens once per read, after every add.
"""
import numpy as np


def plan9():
    """palette.Plan9: 256 x 3 uint8 (every entry opaque)."""
    pal = np.zeros((256, 3), np.uint8)
    i = 0
    for r in range(4):
        for v in range(4):
            j = v - r
            for g in range(4):
                for b in range(4):
                    den = max(r, g, b)
                    if den == 0:
                        c = (0x11 * v,) * 3
                    else:
                        num = 17 * (4 * den + v)
                        c = (r * num // den, g * num // den, b * num // den)
                    pal[i + (j & 15)] = c
                    j += 1
            i += 16
    return pal


PLAN9 = plan9()
# the palette as drawPaletted holds it: color.RGBA.RGBA(), i.e. each byte x 0x101, alpha 0xffff
_PAL16 = np.concatenate([PLAN9.astype(np.int64) * 0x101, np.full((256, 1), 0xFFFF, np.int64)], axis=1)


def _clamp(i):
    return 0 if i < 0 else (0xFFFF if i > 0xFFFF else i)


def _div16(v):
    """Go's int32 division: truncates toward zero"""
    q = abs(v) // 16
    return q if v >= 0 else -q


def _sqdiff(x, y):
    d = (x - y) & 0xFFFFFFFF
    return ((d * d) & 0xFFFFFFFF) >> 2


def dither_scalar(rgba):
    """draw.FloydSteinberg.Draw(pm, b, m, b.Min) for m *image.RGBA (premultiplied h x w x 4 uint8) -> h x w uint8 indices"""
    h, w = rgba.shape[:2]
    pal = [tuple(int(v) for v in p) for p in _PAL16]
    out = np.zeros((h, w), np.uint8)
    curr = [[0] * 4 for _ in range(w + 2)]
    nxt = [[0] * 4 for _ in range(w + 2)]
    for y in range(h):
        for x in range(w):
            e = [_clamp(int(rgba[y, x, c]) * 0x101 + _div16(curr[x + 1][c])) for c in range(4)]
            best, best_sum = 0, (1 << 32) - 1
            for idx, p in enumerate(pal):
                s = _sqdiff(e[0], p[0]) + _sqdiff(e[1], p[1]) + _sqdiff(e[2], p[2]) + _sqdiff(e[3], p[3])
                if s < best_sum:
                    best, best_sum = idx, s
                    if s == 0:
                        break
            out[y, x] = best
            e = [e[c] - pal[best][c] for c in range(4)]
            for c in range(4):
                nxt[x][c] += e[c] * 3
                nxt[x + 1][c] += e[c] * 5
                nxt[x + 2][c] += e[c] * 1
                curr[x + 2][c] += e[c] * 7
        curr, nxt = nxt, curr
        for q in nxt:
            q[:] = [0, 0, 0, 0]
    return out


def dither_wavefront(rgba):
    """dither_scalar's result, one anti-diagonal t = x + 2y at a time (numpy over the pixels of a diagonal and the palette)"""
    h, w = rgba.shape[:2]
    src = rgba.astype(np.int64) * 0x101
    # acc[y, x + 1]: the quantErrorCurr entry row y reads at pixel x (columns 0 and w + 1 catch the terms Go drops)
    acc = np.zeros((h + 1, w + 2, 4), np.int64)
    out = np.zeros((h, w), np.uint8)
    pal = _PAL16[None, :, :]
    for t in range(w + 2 * h - 2):
        y = np.arange(max(0, (t - w + 2) // 2), min(h - 1, t // 2) + 1)
        x = t - 2 * y
        ok = (x >= 0) & (x < w)
        y, x = y[ok], x[ok]
        if y.size == 0:
            continue
        q = acc[y, x + 1]
        e = np.clip(src[y, x] + np.sign(q) * (np.abs(q) // 16), 0, 0xFFFF)
        d = (e[:, None, :] - pal) ** 2 >> 2
        best = np.argmin(d.sum(axis=2), axis=1)            # argmin returns the first minimum
        out[y, x] = best
        e = e - _PAL16[best]
        acc[y + 1, x] += 3 * e
        acc[y + 1, x + 1] += 5 * e
        acc[y + 1, x + 2] += e
        acc[y, x + 2] += 7 * e
    return out


def lzw_encode(index):
    """compress/lzw NewWriter(w, LSB, 8), Write(index bytes), Close() -> bytes.  The codes are fixed by the algorithm (greedy
    longest match; Go's code widths and clear timing); Go's hash table only finds them, so a dict stands in for it."""
    data = bytes(np.ascontiguousarray(index, dtype=np.uint8).reshape(-1))
    out = bytearray()
    st = {"bits": 0, "nbits": 0, "width": 9, "hi": 257, "overflow": 512}
    table = {}

    def write(c):
        st["bits"] |= c << st["nbits"]
        st["nbits"] += st["width"]
        while st["nbits"] >= 8:
            out.append(st["bits"] & 0xFF)
            st["bits"] >>= 8
            st["nbits"] -= 8

    def inc_hi():
        """False: out of codes (a clear code went out and the table is empty)"""
        st["hi"] += 1
        if st["hi"] == st["overflow"]:
            st["width"] += 1
            st["overflow"] <<= 1
        if st["hi"] == 4095:
            write(256)
            st["width"], st["hi"], st["overflow"] = 9, 257, 512
            table.clear()
            return False
        return True

    if not data:
        write(256)
    else:
        write(256)
        code = data[0]
        for lit in data[1:]:
            key = code << 8 | lit
            hit = table.get(key)
            if hit is not None:
                code = hit
                continue
            write(code)
            code = lit
            if inc_hi():
                table[key] = st["hi"]
        write(code)
        inc_hi()
    write(257)
    if st["nbits"] > 0:
        out.append(st["bits"] & 0xFF)
    return bytes(out)


def sub_blocks(data):
    """image/gif's blockWriter: blocks of at most 255 bytes behind their length, then the 0x00 terminator"""
    out = bytearray()
    for i in range(0, len(data), 255):
        blk = data[i:i + 255]
        out.append(len(blk))
        out += blk
    out.append(0)
    return bytes(out)


def header(w, h):
    """GIF89a, the logical screen with the Plan 9 table as global colour table, the image descriptor, LZW minimum code size 8"""
    b = bytearray(b"GIF89a")
    b += bytes([w & 0xFF, w >> 8, h & 0xFF, h >> 8, 0x87, 0, 0])
    b += PLAN9.tobytes()
    b += bytes([0x2C, 0, 0, 0, 0, w & 0xFF, w >> 8, h & 0xFF, h >> 8, 0])
    b.append(8)
    return bytes(b)


def encode_index(index):
    """the stream gif.Encode writes for an already dithered h x w index frame"""
    h, w = index.shape
    if w >= 1 << 16 or h >= 1 << 16:
        raise ValueError("gif: image is too large to encode")
    return header(w, h) + sub_blocks(lzw_encode(index)) + b"\x3b"


def encode(rgba, scalar=False):
    """gif.Encode(buf, rgba, nil): Plan 9 + Floyd-Steinberg, then the stream"""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    return encode_index(dither_scalar(rgba) if scalar else dither_wavefront(rgba))


def size_bound(w, h):
    """an upper bound of the stream's length (the library sizes its per-frame regions by the same rule)"""
    npix = w * h
    codes = npix + 3 + npix // 3838 + 1
    data = (codes * 12 + 7) // 8
    return len(header(1, 1)) + data + (data + 254) // 255 + 1 + 1
