"""image.Decode of a GIF (gif.Decode: the FIRST image of the file, as an *image.Paletted) restated in Python: the model the GPU GIF
decoder is held to.

PARITY UNPINNED against Go itself (no toolchain): this restates Go's image/gif/reader.go and compress/lzw/reader.go as recalled,
not as read, and not as run.  What pins it here: Pillow decodes the same pixels and palette on valid files, the GIF encoder model
(tests/gif_model.py) round-trips through it, and the hand-derived known answers of tests/golden/gif_dec_kats.json carry every rule.
A helper of the tests only: the product never imports it.

decode(data) -> dict:
  ok       True when gif.Decode returns an image;
  error    why not (Go's message, roughly), None when ok;
  stage    "container" (header, tables, extensions, descriptor, LZW width), "lzw" (the image data, its sub-blocks, the pixel check)
           or None when ok;
  rect     (left, top, w, h) of the first image once its descriptor was read (else None);
  index    h x w uint8 (row order, interlace undone) when ok;
  palette  256 x 4 uint8 (R, G, B, A; opaque entries A = 255; the transparent entry and unused entries zero) when ok;
  pal_len  len(m.Palette) when ok.

Rules carried (reader.go):
  * "GIF87a" / "GIF89a", 13 header bytes; the global table (flag 0x80, 1 << (1 + (flags & 7)) entries) when present, truncated = error;
  * before the first image: 0x21 extensions -- 0xF9 graphic control (6 bytes: size 4, flags, delay, transparent index, terminator 0;
    flag 1 sets the transparent index), 0xFE comment, 0xFF application (a size byte, that many bytes), 0x01 plain text (13 bytes),
    any other label an error; their sub-blocks are skipped -- 0x2C the image, 0x3B trailer = "missing image data", anything else an
    error;
  * the descriptor: left + w <= screen w and top + h <= screen h; a local table replaces the global one; no table at all = error;
    the transparent index's entry becomes color.RGBA{} (a copy of the global table), an index >= len(palette) lengthens the palette
    with color.RGBA{} up to index + 1 (golang.org/issue/15059); LZW minimum code size 2..8;
  * LZW (LSB): clear = 1 << lit, eof = clear + 1, width lit + 1 growing when hi reaches overflow; KwKwK = code == hi with a previous
    code; a code above hi = "invalid code"; with hi at 4095 and width 12 the reader drops its previous code (no entry is added until
    a clear), so 4095 then means the entry 4095 that the code which filled the table defined;
  * fewer than w * h bytes = "not enough image data", one more = "too much image data"; a missing EOF code is accepted;
  * blockReader.close: after the EOF code at most the rest of the current sub-block may follow, or -- when the data ended exactly on a
    sub-block boundary -- one more sub-block of ONE byte, then the block terminator (golang.org/issue/16146); truncated files fail;
  * len(palette) < 256: an index >= len(palette) = "invalid pixel value"; interlaced frames are put back into row order, passes
    (8, 0), (8, 4), (4, 2), (2, 1); later bytes (further frames, the trailer) are never read.
"""
import numpy as np

INTERLACE = ((8, 0), (8, 4), (4, 2), (2, 1))


class _Fail(Exception):
    def __init__(self, msg, stage):
        super().__init__(msg)
        self.stage = stage


class _Reader:
    def __init__(self, data):
        self.d = bytes(data)
        self.p = 0

    def byte(self, what):
        if self.p >= len(self.d):
            raise _Fail("gif: %s: unexpected EOF" % what, self.stage)
        self.p += 1
        return self.d[self.p - 1]

    def full(self, n, what):
        if self.p + n > len(self.d):
            raise _Fail("gif: %s: unexpected EOF" % what, self.stage)
        self.p += n
        return self.d[self.p - n:self.p]


def read_sub_blocks(r):
    """(data, sizes, terminated): the sub-blocks as blockReader.fill sees them -- a sub-block the file cuts short is not delivered"""
    data, sizes = bytearray(), []
    while True:
        if r.p >= len(r.d):
            return bytes(data), sizes, False
        n = r.d[r.p]
        r.p += 1
        if n == 0:
            return bytes(data), sizes, True
        if r.p + n > len(r.d):
            return bytes(data), sizes, False
        data += r.d[r.p:r.p + n]
        sizes.append(n)
        r.p += n


def lzw_decode(data, lit, limit):
    """compress/lzw's reader over the bytes -> (pixels (at most limit + 1 of them), how it ended: "eof" / "end" (a code would need bits
    past the data) / "invalid" / "too much", bytes consumed at the EOF code).  The dictionary holds each entry's whole string (what
    the prefix / suffix chains of reader.go spell out)."""
    clear, eof = 1 << lit, (1 << lit) + 1
    lits = [bytes([v]) for v in range(clear)]
    table = lits + [b""] * (4096 - clear)
    width, hi, overflow, last = lit + 1, eof, 1 << (lit + 1), None
    nbits, bit = 8 * len(data), 0
    out = []
    n = 0
    while True:
        if bit + width > nbits:
            return b"".join(out), "end", len(data)
        p = bit >> 3
        code = (int.from_bytes(data[p:p + 3], "little") >> (bit & 7)) & ((1 << width) - 1)
        bit += width
        if code == clear:
            width, hi, overflow, last = lit + 1, eof, 1 << (lit + 1), None
            continue
        if code == eof:
            return b"".join(out), "eof", (bit + 7) // 8
        if code < clear:
            s = lits[code]
        elif code < hi or (code == hi and last is None):
            s = table[code]
        elif code == hi:                      # KwKwK: the last expansion and its own first byte
            s = table[last] + table[last][:1]
        else:
            return b"".join(out), "invalid", None
        if last is not None:
            table[hi] = table[last] + s[:1]
        out.append(s)
        n += len(s)
        if n > limit:
            return b"".join(out)[:limit + 1], "too much", None
        last, hi = code, hi + 1
        if hi >= overflow:
            if width == 12:                   # full: the previous code is dropped, hi stays at 4095, no entry until a clear
                last = None
                hi -= 1
            else:
                width += 1
                overflow = 1 << width


def uninterlace(pix, w, h):
    out = np.empty((h, w), np.uint8)
    src = pix.reshape(h, w)
    r = 0
    for skip, start in INTERLACE:
        for y in range(start, h, skip):
            out[y] = src[r]
            r += 1
    return out


def _close_ok(sizes, terminated, consumed):
    """blockReader.close after the EOF code, `consumed` bytes of the sub-blocks' data read"""
    if not terminated:
        return False
    ends = np.cumsum(sizes).tolist() if sizes else []
    m = next(k for k, e in enumerate(ends) if e >= consumed)       # the sub-block holding the last byte read
    rest = sizes[m + 1:]
    if not rest:
        return True
    return consumed == ends[m] and len(rest) == 1 and rest[0] == 1


def decode(data):
    r = _Reader(data)
    r.stage = "container"
    res = {"ok": False, "error": None, "stage": None, "rect": None, "index": None, "palette": None, "pal_len": None}
    try:
        hdr = r.full(13, "reading header")
        if hdr[:6] not in (b"GIF87a", b"GIF89a"):
            raise _Fail("gif: can't recognize format %r" % hdr[:6], "container")
        sw, sh = hdr[6] | hdr[7] << 8, hdr[8] | hdr[9] << 8
        gtab = None
        if hdr[10] & 0x80:
            n = 1 << (1 + (hdr[10] & 7))
            t = r.full(3 * n, "reading color table")
            gtab = [(t[3 * i], t[3 * i + 1], t[3 * i + 2], 255) for i in range(n)]
        trans = None
        while True:
            c = r.byte("reading frames")
            if c == 0x21:
                label = r.byte("reading extension")
                if label == 0xF9:
                    g = r.full(6, "can't read graphic control")
                    if g[0] != 4:
                        raise _Fail("gif: invalid graphic control extension block size: %d" % g[0], "container")
                    if g[1] & 1:
                        trans = g[4]
                    if g[5] != 0:
                        raise _Fail("gif: invalid graphic control extension block terminator: %d" % g[5], "container")
                    continue
                if label == 0x01:
                    r.full(13, "reading extension")
                elif label == 0xFE:
                    pass
                elif label == 0xFF:
                    r.full(r.byte("reading extension"), "reading extension")
                else:
                    raise _Fail("gif: unknown extension 0x%.2x" % label, "container")
                while True:
                    n = r.byte("reading extension")
                    if n == 0:
                        break
                    r.full(n, "reading extension")
            elif c == 0x2C:
                break
            elif c == 0x3B:
                raise _Fail("gif: missing image data", "container")
            else:
                raise _Fail("gif: unknown block type: 0x%.2x" % c, "container")
        d = r.full(9, "can't read image descriptor")
        left, top = d[0] | d[1] << 8, d[2] | d[3] << 8
        w, h = d[4] | d[5] << 8, d[6] | d[7] << 8
        fields = d[8]
        if left + w > sw or top + h > sh:
            raise _Fail("gif: frame bounds larger than image bounds", "container")
        res["rect"] = (left, top, w, h)
        if fields & 0x80:
            n = 1 << (1 + (fields & 7))
            t = r.full(3 * n, "reading color table")
            pal = [(t[3 * i], t[3 * i + 1], t[3 * i + 2], 255) for i in range(n)]
        else:
            if gtab is None:
                raise _Fail("gif: no color table", "container")
            pal = list(gtab)
        if trans is not None:
            if trans < len(pal):
                pal[trans] = (0, 0, 0, 0)
            else:
                pal += [(0, 0, 0, 0)] * (trans + 1 - len(pal))
        lit = r.byte("reading image data")
        if lit < 2 or lit > 8:
            raise _Fail("gif: pixel size in decode out of range: %d" % lit, "container")
        r.stage = "lzw"
        data, sizes, terminated = read_sub_blocks(r)
        npix = w * h
        pix, how, consumed = lzw_decode(data, lit, npix)
        if how == "invalid":
            raise _Fail("gif: reading image data: lzw: invalid code", "lzw")
        if how == "too much" or (how in ("eof", "end") and len(pix) > npix):
            raise _Fail("gif: too much image data", "lzw")
        if len(pix) < npix:
            raise _Fail("gif: not enough image data", "lzw")
        if how == "end" and not terminated:
            raise _Fail("gif: reading image data: unexpected EOF", "lzw")
        if how == "eof" and not _close_ok(sizes, terminated, consumed):
            raise _Fail("gif: too much image data (or unexpected EOF) after the LZW data", "lzw")
        idx = np.frombuffer(pix, np.uint8).copy()
        if len(pal) < 256 and npix and int(idx.max()) >= len(pal):
            raise _Fail("gif: invalid pixel value", "lzw")
        idx = uninterlace(idx, w, h) if fields & 0x40 else idx.reshape(h, w)
        palette = np.zeros((256, 4), np.uint8)
        palette[:min(len(pal), 256)] = np.array(pal[:256], np.uint8).reshape(-1, 4)
        res.update(ok=True, index=idx, palette=palette, pal_len=len(pal))
        return res
    except _Fail as e:
        res.update(error=str(e), stage=e.stage)
        return res


# status codes of include/ipx.h
OK, INVALID, UNSUPPORTED = 0, -1, -4


def entry_status(res, batch_wh=None):
    """what ipx_gif_decode_batch reports for a file the model decoded to `res`, in a batch of size batch_wh (None: this file sets it).
    Container errors are Go's errors; then the first image's geometry decides what the GPU takes (a non-zero origin, an empty frame
    or another size: Go decodes those itself); image-data errors come last."""
    if res["stage"] == "container":
        return INVALID
    left, top, w, h = res["rect"]
    if left or top or w == 0 or h == 0 or (batch_wh is not None and (w, h) != tuple(batch_wh)) or w * h > 0x7fff0000:
        return UNSUPPORTED
    return OK if res["ok"] else INVALID
