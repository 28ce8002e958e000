#!/usr/bin/env python3
"""Every route through the encoders' host side, once each at tiny shapes: the five encode cores through their public entries, the two
single-frame entries that share a helper, the three host-frame legs (JPEG, PNG, GIF) and the JPEG-to-JPEG leg.  Made to be run under
    rocprofv3 --kernel-trace --stats -- python tools/enc_host_calls.py
on two trees whose device work should be the same: the kernel names and call counts of the two runs are then compared
(profiles/enc_host_refactor.txt).  Two or three frames per call, sides 17x9 and 33x16, one frame with non-opaque pixels so that both
PNG colour types occur.  Prints a digest of every stream it got, so two trees can also be compared byte for byte."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import imageprocessor_amd as ipx


def frames(n, w, h, seed):
    """n premultiplied RGBA8 frames; frame 1 has non-opaque pixels, the others are opaque"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    f[..., 3] = 255
    if n > 1:
        f[1, : h // 2, :, 3] = rng.integers(0, 255, (h // 2, w), dtype=np.uint8)
        a = f[1, ..., 3:4].astype(np.uint16)
        f[1, ..., :3] = (f[1, ..., :3].astype(np.uint16) * a // 255).astype(np.uint8)
    return f


digest = hashlib.sha256()


def took(name, streams):
    streams = [bytes(s) for s in streams]
    assert streams and all(streams), name
    for s in streams:
        digest.update(len(s).to_bytes(8, "little") + s)
    print("%-34s %d streams, %d bytes" % (name, len(streams), sum(len(s) for s in streams)), flush=True)


def legs(name, out):
    for k in sorted(out):
        took("%s %s" % (name, k), out[k])


with ipx.Context(device=0) as ctx:
    small, large = frames(3, 17, 9, 1), frames(2, 33, 16, 2)
    bufs = [ctx.alloc(a.nbytes).upload(a) for a in (small, large)]
    # the three uniform cores through their batch entries, at both sizes
    for a, b in zip((small, large), bufs):
        n, h, w = a.shape[:3]
        took("jpeg batch %dx%d" % (w, h), ctx.jpeg_encode_batch_dev(b.ptr, w, h, n, quality=85))
        took("png batch %dx%d" % (w, h), ctx.png_encode_batch_dev(b.ptr, w, h, n))
        took("gif batch %dx%d" % (w, h), ctx.gif_encode_batch_dev(b.ptr, w, h, n))
    # the two mixed-size cores: two frames of one size and one of the other
    mixed = [(bufs[0].ptr, 17, 9, 17 * 4), (bufs[0].ptr + 17 * 9 * 4, 17, 9, 17 * 4), (bufs[1].ptr, 33, 16, 33 * 4)]
    took("jpeg mixed", ctx.jpeg_encode_mixed_dev(mixed, quality=85))
    took("png mixed", ctx.png_encode_mixed_dev(mixed))
    # the single-frame entries
    took("png one frame", [ctx.png_encode(small[1])])
    took("gif one frame", [ctx.gif_encode(small[1])])
    # the legs: 33x16 sources, every output wanted
    glyph = {"mask": np.full((4, 4), 200, np.uint8), "dr": (2, 2, 6, 6), "mp": (0, 0)}
    gs = ctx.glyphset([glyph], (255, 255, 255, 127))
    plan = ctx.plan(33, 16, resize=(20, 10, False), thumbnail=(8, True), watermark=gs)
    src = frames(3, 33, 16, 3)
    legs("host jpeg", plan.run_host_jpeg(src, quality=85))
    legs("host png", plan.run_host_png(src))
    rng = np.random.default_rng(4)
    index = rng.integers(0, 256, (3, 16, 33), dtype=np.uint8)
    palettes = rng.integers(0, 256, (3, 256, 4), dtype=np.uint8)
    palettes[..., 3] = 255
    legs("host gif", plan.run_host_paletted_gif(index, palettes, quality=85))
    files = [ctx.jpeg_encode(src[i], 90) for i in range(3)]
    out, status = plan.run_jpeg_jpeg(files, quality=85)
    assert status == [0, 0, 0], status
    legs("jpeg to jpeg", out)
    plan.close()
    gs.close()
    for b in bufs:
        b.free()
print("digest %s" % digest.hexdigest())
