"""PNG files for the decoder tests: a small writer that controls everything the decoder has to handle (colour type and depth, tRNS,
the filter of every row, zlib level / strategy / window bits, where the IDAT chunks split), and seeded photo-like / flat frames."""
import struct
import zlib

import numpy as np

import png_decode_model as dm


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


def filter_rows(rows, bpp, filters):
    """raw rows (h x rowbytes - 1 uint8) -> the filtered stream with filters[y] (0 .. 4) on row y"""
    h, n = rows.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    for y in range(h):
        cur = rows[y].astype(np.int32)
        ft = int(filters[y % len(filters)])
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])[:n]
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])[:n]
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - a
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((a + prev) >> 1)
        else:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            f = cur - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        out.append(ft)
        out += (f & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def pack_rows(samples, ctype, depth):
    """h x w x channels integer samples -> raw rows (h x rowbytes - 1 uint8)"""
    h, w = samples.shape[:2]
    s = samples.reshape(h, -1)
    if depth == 16:
        return s.astype(">u2").view(np.uint8).reshape(h, -1)
    if depth == 8:
        return s.astype(np.uint8)
    ppb = 8 // depth
    wp = -(-s.shape[1] // ppb) * ppb
    p = np.zeros((h, wp), np.uint8)
    p[:, :s.shape[1]] = s
    p = p.reshape(h, -1, ppb)
    out = np.zeros(p.shape[:2], np.uint8)
    for j in range(ppb):
        out |= (p[:, :, j] << (8 - depth * (j + 1))).astype(np.uint8)
    return out


def write(samples, ctype, depth, plte=None, trns=None, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, split=None,
          extra=b"", seed=0):
    """a PNG of these samples.  split: None (one IDAT), an int (IDAT chunks of that many bytes) or "random" (seeded split points);
    extra: chunks to put before the first IDAT"""
    samples = np.asarray(samples)
    h, w = samples.shape[:2]
    bpp, _ = dm.geometry(ctype, depth, w)
    raw = filter_rows(pack_rows(samples, ctype, depth), bpp, filters)
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    stream = co.compress(raw) + co.flush()
    out = dm.SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
    if plte is not None:
        out += chunk(b"PLTE", bytes(np.asarray(plte, np.uint8).ravel()))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    out += extra
    if split is None:
        parts = [stream]
    elif split == "random":
        rng = np.random.default_rng(seed)
        cuts = sorted(set(rng.integers(1, max(2, len(stream)), 4).tolist()))      # no empty IDAT after the stream
        parts = [stream[a:b] for a, b in zip([0] + cuts, cuts + [len(stream)])]
    else:
        parts = [stream[i:i + split] for i in range(0, len(stream), split)] or [b""]
    for p in parts:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"")


def photo(h, w, c, seed, maxv=255):
    """smooth gradients plus noise: what a photograph looks like to the filters"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (k + 1) * 3 + y * (3 - k) * 2) % 256 for k in range(c)], -1)
    v = (base + rng.integers(-12, 13, (h, w, c))) % 256
    return (v * maxv // 255).astype(np.int64)


def flat(h, w, c, seed, maxv=255):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, maxv + 1, (h // 16 + 1, w // 16 + 1, c))
    return np.repeat(np.repeat(blocks, 16, 0), 16, 1)[:h, :w].astype(np.int64)


# one file per row of the type table: (name, ctype, depth, with tRNS)
TYPES = [("gray1", 0, 1, False), ("gray2", 0, 2, False), ("gray4", 0, 4, False), ("gray8", 0, 8, False), ("gray8_trns", 0, 8, True),
         ("ga8", 4, 8, False), ("rgb8_trns", 2, 8, True), ("rgba8", 6, 8, False), ("rgb8", 2, 8, False), ("pal1", 3, 1, False),
         ("pal2", 3, 2, False), ("pal4", 3, 4, True), ("pal8", 3, 8, True), ("gray16", 0, 16, False), ("rgb16", 2, 16, False),
         ("gray16_trns", 0, 16, True), ("ga16", 4, 16, False), ("rgb16_trns", 2, 16, True), ("rgba16", 6, 16, False)]


def samples_of_type(ctype, depth, h, w, seed, kind="photo"):
    """the samples of_type writes"""
    c = dm.CHANNELS[ctype]
    return (photo if kind == "photo" else flat)(h, w, c, seed, 255) * ((1 << depth) - 1) // 255


def of_type(ctype, depth, trns, h, w, seed, kind="photo", **kw):
    """a file of the type with seeded samples; tRNS picks a sample value that occurs, palettes hold fewer entries than indices reach"""
    rng = np.random.default_rng(seed)
    maxv = (1 << depth) - 1
    c = dm.CHANNELS[ctype]
    s = samples_of_type(ctype, depth, h, w, seed, kind)
    plte = t = None
    if ctype == 3:
        npal = max(1, min(256, (maxv + 1) * 3 // 4))
        plte = rng.integers(0, 256, (npal, 3))
        if trns:
            t = rng.integers(0, 256, max(1, npal // 2)).astype(np.uint8).tobytes()
    elif trns:
        v = s[0, 0]
        t = struct.pack(">%dH" % c, *[int(x) for x in np.atleast_1d(v)])
    return write(s, ctype, depth, plte=plte, trns=t, seed=seed, **kw)
