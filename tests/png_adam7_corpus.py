"""Adam7-interlaced PNG files for the decoder tests: png_corpus's writer with the rows laid out as the seven passes.  Each non-empty
pass is an image of its own (packed by the pass's width, filtered from a zero row above); the passes are concatenated and compressed as
one zlib stream under an IHDR with interlace 1.  Pillow cannot write such files."""
import struct
import zlib

import numpy as np

import png_corpus as pc
import png_decode_model as dm

# (xFactor, yFactor, xOffset, yOffset) of passes 1 .. 7
PASSES = [(8, 8, 0, 0), (8, 8, 4, 0), (4, 8, 0, 4), (4, 4, 2, 0), (2, 4, 0, 2), (2, 2, 1, 0), (1, 2, 0, 1)]


def pass_sizes(w, h):
    """(pw, ph) of the seven passes; a pass with a zero side has no bytes at all"""
    return [((w - xo + xf - 1) // xf if w > xo else 0, (h - yo + yf - 1) // yf if h > yo else 0) for xf, yf, xo, yo in PASSES]


def raw_length(ctype, depth, w, h):
    return sum(ph * dm.geometry(ctype, depth, pw)[1] for pw, ph in pass_sizes(w, h) if pw and ph)


def raw_stream(samples, ctype, depth, filters=(0,)):
    """the filtered bytes of the seven passes, and where each pass starts in them (None: empty)"""
    samples = np.asarray(samples)
    bpp, _ = dm.geometry(ctype, depth, samples.shape[1])
    raw, starts = b"", []
    for xf, yf, xo, yo in PASSES:
        sub = samples[yo::yf, xo::xf]
        starts.append(len(raw) if sub.shape[0] and sub.shape[1] else None)
        if sub.shape[0] and sub.shape[1]:
            raw += pc.filter_rows(pc.pack_rows(sub, ctype, depth), bpp, filters)
    return raw, starts


def wrap(w, h, ctype, depth, stream, plte=None, trns=None, split=None, extra=b"", seed=0, interlace=1):
    """the file around a zlib stream"""
    out = dm.SIG + pc.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if plte is not None:
        out += pc.chunk(b"PLTE", bytes(np.asarray(plte, np.uint8).ravel()))
    if trns is not None:
        out += pc.chunk(b"tRNS", bytes(trns))
    out += extra
    if split is None:
        parts = [stream]
    elif split == "random":
        rng = np.random.default_rng(seed)
        cuts = sorted(set(rng.integers(1, max(2, len(stream)), 4).tolist()))
        parts = [stream[a:b] for a, b in zip([0] + cuts, cuts + [len(stream)])]
    else:
        parts = [stream[i:i + split] for i in range(0, len(stream), split)] or [b""]
    return out + b"".join(pc.chunk(b"IDAT", p) for p in parts) + pc.chunk(b"IEND", b"")


def write(samples, ctype, depth, plte=None, trns=None, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, split=None,
          extra=b"", seed=0):
    """png_corpus.write, interlaced"""
    samples = np.asarray(samples)
    h, w = samples.shape[:2]
    raw, _ = raw_stream(samples, ctype, depth, filters)
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return wrap(w, h, ctype, depth, co.compress(raw) + co.flush(), plte, trns, split, extra, seed)


def of_type(ctype, depth, trns, h, w, seed, kind="photo", interlace=True, **kw):
    """png_corpus.of_type, interlaced or not: the same samples, palette and tRNS either way (the twin of a file)"""
    rng = np.random.default_rng(seed)
    maxv = (1 << depth) - 1
    c = dm.CHANNELS[ctype]
    s = pc.samples_of_type(ctype, depth, h, w, seed, kind)
    plte = t = None
    if ctype == 3:
        npal = max(1, min(256, (maxv + 1) * 3 // 4))
        plte = rng.integers(0, 256, (npal, 3))
        if trns:
            t = rng.integers(0, 256, max(1, npal // 2)).astype(np.uint8).tobytes()
    elif trns:
        t = struct.pack(">%dH" % c, *[int(x) for x in np.atleast_1d(s[0, 0])])
    return (write if interlace else pc.write)(s, ctype, depth, plte=plte, trns=t, seed=seed, **kw)

