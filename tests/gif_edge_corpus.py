"""GIF files whose LZW streams do what Pillow's never do (tests/lzw_writer.py): every literal width 2 .. 8 (also wider than the palette
needs), a table that freezes at 4095 and serves 12-bit codes for the rest of the frame, clear codes every N codes, doubled clears, no
leading clear, sub-blocks of 1 .. 255 bytes, interlaced or not.  corpus() -> [(name, file, index frame, palette, frozen codes)]."""
import numpy as np

import gif_corpus
import lzw_writer as lw


def frame(w, h, ncol, seed, kind):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, ncol, (h, w)).astype(np.uint8)
    if kind == "runs":                                    # long runs: the longest strings the dictionary can hold
        rng = np.random.default_rng(seed)
        v = np.repeat(rng.integers(0, ncol, w * h // 64 + 1), 64)[:w * h]
        return v.reshape(h, w).astype(np.uint8)
    return gif_corpus.indices(w, h, ncol, seed, kind)


def make(name, w, h, bits, lit, seed, kind="photo", **kw):
    """(name, file, index, palette, frozen codes): a palette of 1 << bits colours, indices below it, literal width lit"""
    ncol = 1 << bits
    idx = frame(w, h, ncol, seed, kind)
    pal = np.random.default_rng(seed + 500).integers(0, 256, (ncol, 3)).astype(np.uint8)
    data, frozen = lw.gif(idx, pal, lit=lit, seed=seed, **kw)
    return name, data, idx, pal, frozen


# (literal width, palette bits): every width at its own palette size and wider than the palette needs
WIDTHS = [(2, 1), (2, 2), (3, 3), (3, 1), (4, 4), (5, 5), (5, 2), (6, 6), (7, 7), (8, 8), (8, 2), (8, 5)]
POLICIES = [dict(clear="full"), dict(clear="never"), dict(clear="every", every=1), dict(clear="every", every=5),
            dict(clear="every", every=300), dict(clear="full", lead=False), dict(clear="never", lead=False),
            dict(clear="every", every=7, double=True), dict(clear="full", double=True)]


def corpus(w=160, h=120, seed=3):
    """every width under one policy each, every policy at width 8 and 3, sub-blocks 255 / 1 / random, interlace on and off; a
    frozen table serving tens of thousands of codes, and clears that come long after the table froze (a deferred clear)"""
    out = []
    for k, (lit, bits) in enumerate(WIDTHS):
        pol = POLICIES[k % len(POLICIES)]
        out.append(make("lit %d / %d colours %s" % (lit, 1 << bits, pol), w, h, bits, lit, seed + k, ("photo", "noise", "runs")[k % 3],
                        sub=(255, 1, "random")[k % 3], interlace=k % 2 == 1, **pol))
    for k, pol in enumerate(POLICIES):
        for lit, bits in ((8, 8), (3, 2)):
            out.append(make("policy %s lit %d" % (pol, lit), w, h, bits, lit, seed + 100 + 2 * k + lit, ("noise", "runs", "photo")[k % 3],
                            sub=("random", 255, 1)[k % 3], interlace=k % 2 == 0, **pol))
    out.append(make("frozen noise 256x200", 256, 200, 8, 8, seed + 300, "noise", clear="never"))
    out.append(make("frozen runs 256x200 lit 4", 256, 200, 4, 4, seed + 301, "runs", clear="never", sub="random"))
    out.append(make("deferred clear every 6000 codes 256x200", 256, 200, 8, 8, seed + 302, "noise", clear="every", every=6000,
                    interlace=True))
    return out


def large(seed=9):
    """GPU-only frames at 1024 x 768: the table frozen for most of the frame at every width, and the other policies at width 8"""
    out = []
    for k, lit in enumerate(range(2, 9)):
        bits = max(1, lit - k % 2)
        out.append(make("1024x768 frozen lit %d" % lit, 1024, 768, bits, lit, seed + k, ("noise", "runs", "photo")[k % 3],
                        clear="never", sub=(255, "random", 1)[k % 3], interlace=k % 2 == 1))
    for k, pol in enumerate(POLICIES[2:6] + [dict(clear="every", every=8000)]):
        out.append(make("1024x768 %s" % pol, 1024, 768, 8, 8, seed + 20 + k, ("photo", "noise")[k % 2], interlace=k % 2 == 0, **pol))
    return out
