#!/usr/bin/env python
"""The marker pre-pass of the GPU scan walk under AddressSanitizer and UBSan, on the CPU: writes clean progressive files (Pillow, and the
writer corpus of tests/jpeg_prog_writer.py) and damaged ones (the recipe of tests/test_jpeg_progressive.py's damaged-file test: bit
flips and byte changes in the scans, bit flips in the headers, truncations, cuts), builds tools/prog_prepass_check.cpp with the two host
sources it drives under -fsanitize=address,undefined, and runs that program on the files.  Nothing is loaded into Python and no
device is used.

  python tools/prog_prepass_asan.py [--keep DIR]"""
import argparse
import io
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def files():
    import numpy as np
    import jpeg_prog_writer as pw
    from PIL import Image

    def picture(w, h, seed=0, noise=8.0):
        g = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([np.sin(xx / 9.0 + seed) * 100 + 128, np.cos(yy / 7.0) * 100 + 128, (xx * 2 + yy + 31 * seed) % 256], -1)
        return (img + g.normal(0, noise, img.shape)).clip(0, 255).astype(np.uint8)

    def pil_jpeg(img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **kw)
        return buf.getvalue()

    rng = np.random.default_rng(11)
    img = picture(333, 250, seed=8, noise=10.0)
    clean = [pil_jpeg(img, quality=85, progressive=True), pil_jpeg(img, quality=90, subsampling=0, optimize=True, progressive=True),
             pil_jpeg(img[..., 0], quality=80, progressive=True)] + [c[2] for c in pw.corpus()[:-1]]
    out = list(clean)
    for t in range(60 * len(clean)):
        f = bytearray(clean[t % len(clean)])
        sos = f.index(b"\xff\xda")
        kind = (t // len(clean)) % 5
        if kind == 0:
            for _ in range(3):
                f[int(rng.integers(sos + 14, len(f) - 2))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            f[int(rng.integers(sos + 14, len(f) - 2))] = int(rng.integers(0, 256))
        elif kind == 2:
            f[int(rng.integers(2, sos + 14))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 3:
            f = f[:int(rng.integers(sos, len(f)))]
        else:
            a = int(rng.integers(sos + 14, len(f) - 10))
            del f[a:a + int(rng.integers(1, 1500))]
        out.append(bytes(f))
    # ends that the reader and the marker loop treat differently: a lone 0xff, fill bytes, a stray RSTn, 0xff 0x00 before EOI
    base = clean[0]
    for tail in (b"\xff", b"\xff\xff", b"\xff\xff\xd9", b"\xff\xd3\xff\xd9", b"\xff\x00\xff\xd9", b"\x00\xff"):
        out.append(base[:-2] + tail)
    # more DHT definitions than a 16-bit index holds, none of them used by a scan
    import jpeg_writer as jw
    frame = pw.colour_frame(48, 40)
    out.append(pw.progressive(frame, jw.all_blocks(frame, np.random.default_rng(1)), pw.libjpeg_script(frame), extra=pw.unused_tables(70000)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", help="write the files and the program there instead of a temporary directory")
    a = ap.parse_args()
    from imageprocessor_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        os.makedirs(work, exist_ok=True)
        paths = []
        for k, f in enumerate(files()):
            paths.append(os.path.join(work, "f%04d.jpg" % k))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        exe = os.path.join(work, "prog_prepass_check")
        src = [os.path.join(ROOT, "tools", "prog_prepass_check.cpp"), os.path.join(b.CSRC, "ipx_jpeg_dec_host.cpp"), os.path.join(b.CSRC, "ipx_jpeg_dec_prog.cpp")]
        # the host compiler and flags of tools/sanitize/run.sh (the sources are plain C++ behind the HIP headers they include)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
               "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-pthread", "-o", exe] + src
        print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        for k in range(0, len(paths), 200):
            subprocess.check_call([exe] + paths[k:k + 200], env=dict(os.environ, IPX_JPEG_PROG_GPU="1"))
    print("prog_prepass_asan: clean")


if __name__ == "__main__":
    main()
