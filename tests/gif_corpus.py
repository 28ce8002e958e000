"""Seeded GIF files written by Pillow, for the GIF decoder's tests and tools/bench_gif_decode.py: photo-like frames (noise over
gradients) and flat graphics (a few colours in rectangles), interlaced or not, palettes of 2 to 256 colours, with or without a
transparent index."""
import io

import numpy as np


def indices(w, h, ncol, seed, kind="photo"):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        idx = np.zeros((h, w), np.int64)
        for _ in range(6):
            x0, y0 = rng.integers(0, max(w, 1)), rng.integers(0, max(h, 1))
            idx[y0:y0 + rng.integers(1, h + 1), x0:x0 + rng.integers(1, w + 1)] = rng.integers(0, ncol)
    elif kind == "solid":
        idx = np.full((h, w), int(rng.integers(0, ncol)), np.int64)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        base = (xx * ncol // max(w, 1) + yy * ncol // max(h, 1)) // 2
        idx = base + rng.integers(-2, 3, (h, w))
    return (idx % ncol).astype(np.uint8)


def write(idx, ncol, seed, interlace=False, transparency=None):
    """a GIF of the index frame with a seeded palette of ncol colours (Pillow pads the table to a power of two)"""
    from PIL import Image
    rng = np.random.default_rng(seed + 1000)
    im = Image.fromarray(idx, "P")
    im.putpalette(rng.integers(0, 256, 3 * ncol).tolist())
    kw = {"interlace": interlace}
    if transparency is not None:
        kw["transparency"] = transparency
    b = io.BytesIO()
    im.save(b, "GIF", optimize=False, **kw)
    return b.getvalue()


def make(w, h, seed, kind="photo", ncol=None, interlace=None, transparency=False):
    rng = np.random.default_rng(seed)
    ncol = ncol or int(rng.choice([2, 3, 16, 100, 256]))
    il = bool(rng.integers(0, 2)) if interlace is None else interlace
    tr = int(rng.integers(0, ncol)) if transparency else None
    return write(indices(w, h, ncol, seed, kind), ncol, seed, il, tr)


def corpus(seed=7):
    """(name, bytes) of a mixed corpus: sizes from 1 x 1 to 1024 x 768"""
    rng = np.random.default_rng(seed)
    out = []
    sizes = [(1, 1), (1, 7), (9, 1), (8, 9), (33, 17), (64, 64), (97, 131), (200, 200), (320, 240), (1024, 768)]
    for k, (w, h) in enumerate(sizes):
        for j, (kind, ncol) in enumerate((("photo", 256), ("flat", 2), ("photo", int(rng.integers(3, 200))))):
            s = seed * 1000 + 10 * k + j
            out.append(("%dx%d %s %d il=%d" % (w, h, kind, ncol, (k + j) % 2),
                        make(w, h, s, kind, ncol, interlace=bool((k + j) % 2), transparency=j == 2)))
    return out
