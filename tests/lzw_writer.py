"""A GIF writer with an LZW encoder of its own, for the GIF decoder's edge corpus (tests/gif_edge_corpus.py).

Pillow clears the dictionary in its own way and always at one literal width per palette size; other encoders (Go, giflib, gifsicle)
clear when the table is full, never clear (the table freezes at 4095 and every later code is 12 bits), or clear more often.  This one
does what it is told:

  lzw(index, lit, clear=..., every=N, lead=True, double=False) -> the LZW bytes
    clear "full": a clear code once the encoder's next entry would be 4095 (what Go's and giflib's writers do)
          "never": no clear after the leading one; the decoder's table freezes at 4095 ("deferred clear")
          "every": a clear code after every N codes
    lead: a clear code first (or not: the decoder starts in the cleared state anyway)
    double: every clear written twice
  gif(index, palette, lit=None, sub=255 | 1 | "random", interlace=False, seed=0, **lzw) -> the file

Code widths follow compress/lzw's reader exactly: the encoder mirrors the decoder's hi / width / overflow, so a code is written at the
width the reader will read it with; the width grows when hi reaches 1 << width, and nothing is added once the table is full.
A helper of the tests only."""
import numpy as np


def lzw(index, lit, clear="full", every=0, lead=True, double=False):
    """(LZW bytes, how many codes the decoder reads while its table is frozen)"""
    data = bytes(np.asarray(index, np.uint8).ravel())
    assert 2 <= lit <= 8 and (not data or max(data) < 1 << lit)
    CLR, EOF = 1 << lit, (1 << lit) + 1
    codes, widths = [], []
    st = {}

    def reset():
        st.update(width=lit + 1, hi=EOF, overflow=1 << (lit + 1), dict={}, next=EOF + 1, since=0)

    def emit(c):
        codes.append(c)
        widths.append(st["width"])

    def emit_clear():
        for _ in range(2 if double else 1):
            emit(CLR)
            reset()

    def step():
        """the reader's bookkeeping after a code that outputs bytes"""
        st["hi"] += 1
        if st["hi"] >= st["overflow"]:
            if st["width"] == 12:
                st["hi"] -= 1
            else:
                st["width"] += 1
                st["overflow"] <<= 1

    reset()
    if lead:
        emit_clear()
    frozen = 0
    i, n = 0, len(data)
    while i < n:
        d = st["dict"]
        code, j = data[i], i + 1
        while j < n:
            c = d.get((code, data[j]))
            if c is None:
                break
            code, j = c, j + 1
        if st["next"] > 4096:                         # the table was full before this code: the reader's frozen state
            frozen += 1
        emit(code)
        if j < n and st["next"] <= 4095:
            d[(code, data[j])] = st["next"]           # the entry the reader defines on the next code
        st["next"] += 1
        step()
        st["since"] += 1
        i = j
        if i < n and (clear == "full" and st["next"] >= 4095 or clear == "every" and st["since"] >= every):
            emit_clear()
    emit(EOF)
    # pack LSB first
    acc, nacc, out = 0, 0, bytearray()
    for c, w in zip(codes, widths):
        acc |= c << nacc
        nacc += w
        while nacc >= 8:
            out.append(acc & 255)
            acc >>= 8
            nacc -= 8
    if nacc:
        out.append(acc & 255)
    return bytes(out), frozen


def sub_blocks(data, sub, seed=0):
    """the data cut into sub-blocks of `sub` bytes (1 .. 255) or seeded random sizes 1 .. 254 ("random"), and the terminator"""
    rng = np.random.default_rng(seed)
    out, i = bytearray(), 0
    while i < len(data):
        k = int(rng.integers(1, 255)) if sub == "random" else sub
        part = data[i:i + k]
        out.append(len(part))
        out += part
        i += k
    return bytes(out + b"\0")


def gif(index, palette, lit=None, sub=255, interlace=False, seed=0, **kw):
    """(GIF89a file with a global table of len(palette) colours (a power of two, 2 .. 256), frozen-code count)"""
    index = np.asarray(index, np.uint8)
    h, w = index.shape
    pal = np.asarray(palette, np.uint8).reshape(-1, 3)
    bits = max(1, (len(pal) - 1).bit_length())
    assert len(pal) == 1 << bits
    lit = lit or max(2, bits)
    rows = index
    if interlace:
        order = [y for skip, start in ((8, 0), (8, 4), (4, 2), (2, 1)) for y in range(start, h, skip)]
        rows = index[order]
    data, frozen = lzw(rows, lit, **kw)
    out = bytearray(b"GIF89a")
    out += w.to_bytes(2, "little") + h.to_bytes(2, "little") + bytes([0x80 | (bits - 1), 0, 0])
    out += pal.tobytes()
    out += b"\x2c" + bytes(4) + w.to_bytes(2, "little") + h.to_bytes(2, "little") + bytes([0x40 if interlace else 0])
    out.append(lit)
    out += sub_blocks(data, sub, seed)
    return bytes(out + b"\x3b"), frozen
