"""png.Decode of Adam7-interlaced files restated (image/png reader.go's readImagePass over the seven passes), on top of
tests/png_decode_model.py; the model the GPU decoder is held to under IPX_PNG_ADAM7=1.  PARITY UNPINNED, like that module.

decode(data, adam7=True, fast=False) -> png_decode_model.decode's dict.
  interlace 0:             png_decode_model.decode's answer, unchanged
  interlace 1, adam7 off:  that answer too (UNSUPPORTED from the container, whatever follows the IHDR)
  interlace 1, adam7 on:   every container rule as for any other file; then each non-empty pass (pw x ph, by PASSES) is an image of its
                           own: ph rows of 1 + (bits * pw + 7) / 8 bytes, unfiltered from a zero row above, sub-byte samples packed by
                           the pass's width; its pixel (px, py) is the frame's (xo + px * xf, yo + py * yf), converted as a
                           non-interlaced pixel of the type is.  The raw length is the sum over those passes, and everything about it
                           (too little, too much, bytes after the Adler-32, 2^32 and up) is as for non-interlaced files."""
import struct
import zlib

import numpy as np

import png_decode_model as dm
from png_decode_model import INVALID, OK, UNSUPPORTED

PASSES = [(8, 8, 0, 0), (8, 8, 4, 0), (4, 8, 0, 4), (4, 4, 2, 0), (2, 4, 0, 2), (2, 2, 1, 0), (1, 2, 0, 1)]


def interlace_of(data):
    """the IHDR's interlace byte when the file starts with a 13-byte IHDR, else 0"""
    if len(data) >= 33 and data[:8] == dm.SIG and data[8:16] == b"\x00\x00\x00\x0dIHDR":
        return data[28]
    return 0


def decode(data, adam7=True, fast=False):
    data = bytes(data)
    if interlace_of(data) != 1 or not adam7:
        return dm.decode(data, fast=fast)
    # the container's verdict: the walk of a copy with the interlace byte cleared (its IHDR CRC redone so that the copy's fields are the
    # file's); the file's own IHDR CRC is checked with the others below
    plain = bytearray(data)
    plain[28] = 0
    plain[29:33] = struct.pack(">I", zlib.crc32(bytes(plain[12:29])))
    st, f = dm.parse(bytes(plain))
    r = {"status": st, "stage": "container", "kind": None, "w": f["w"], "h": f["h"], "pix": None, "palette": None, "why": None}
    if st != OK:
        return r
    f["crc"][0] = (data[12:29], struct.unpack(">I", data[29:33])[0])
    ct, dep, w, h = f["ctype"], f["depth"], f["w"], f["h"]
    r["kind"] = kind = dm.kind_of(ct, dep, f["trns"] is not None)
    bpp, _ = dm.geometry(ct, dep, w)
    kb = dm.BPP[kind]
    passes = []                                            # (pw, ph, rowbytes, xf, yf, xo, yo) of the non-empty ones
    for xf, yf, xo, yo in PASSES:
        pw, ph = (w - xo + xf - 1) // xf, (h - yo + yf - 1) // yf
        if pw > 0 and ph > 0:
            passes.append((pw, ph, dm.geometry(ct, dep, pw)[1], xf, yf, xo, yo))
    limit = sum(p[1] * p[2] for p in passes)
    if w > 65535 or h > 65535 or (h - 1) * w * kb + w * kb > dm.MAX_SPAN or limit >= 1 << 32:
        r["status"] = UNSUPPORTED
        return r
    r["stage"] = "data"
    if any(zlib.crc32(body) != crc for body, crc in f["crc"]):
        r.update(status=INVALID, why="crc")
        return r
    stream = b"".join(f["idat"])
    if fast:
        d = zlib.decompressobj()
        raw = d.decompress(stream)
        assert d.eof and len(raw) == limit, "fast=True takes valid streams only"
        end = len(stream) - len(d.unused_data)
    else:
        try:
            raw, end = dm.inflate(stream, limit)
        except dm.FlateError as e:
            r.update(status=INVALID, why=str(e))
            return r
        if len(raw) != limit:
            r.update(status=INVALID, why="not enough pixel data")
            return r
    pix = np.zeros((h, w, kb), np.uint8)
    at = 0
    for pw, ph, rb, xf, yf, xo, yo in passes:
        rows = dm.unfilter(raw[at:at + ph * rb], ph, rb, bpp)            # a zero row above the pass's first
        at += ph * rb
        if rows is None:
            r.update(status=INVALID, why="bad filter type")
            return r
        pix[yo::yf, xo::xf] = dm.convert(rows, ct, dep, pw, ph, f["trns"]).reshape(ph, pw, kb)
    if end != len(stream) or len(stream) - len(f["idat"][-1]) >= end:
        r.update(status=UNSUPPORTED, why="bytes or an IDAT chunk after the Adler-32")
        return r
    r["pix"] = pix.reshape(h, w * kb)
    if kind == dm.PALETTED:
        r["palette"] = dm.palette(f)
    return r


entry_status = dm.entry_status
