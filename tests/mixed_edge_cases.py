"""The inputs of tests/test_jpeg_mixed_edges_gpu.py and tests/test_png_mixed_edges_gpu.py, built without a GPU, and the conditions each
input has to meet to reach the edge it is there for (tests/test_mixed_edge_cases.py asserts them on the CPU, so a case that stops
reaching its edge fails there).  The mixed entries read an image's geometry from a per-image record (JpegMixGeom, PngMixFrame) and
find their image by a search; the inputs put a file whose scan is too long, too short or cut in front of a file of another shape,
scans of very unequal lengths side by side, host-route groups of unequal sizes, more filter rows than one grid row holds and a frame
beyond the opacity pass's 512 workgroups."""
import random

import numpy as np

# ---- JPEG decode -----------------------------------------------------------------------------------------------------------------


_PAR = []


def par_corpus():
    """tests/jpeg_par_corpus.py's files, and behind them one Gray file of Pillow's with a long scan: the corpus's own Gray scans run
    from 4096 to 29 320 bytes (7 x), with this one the class holds the 16 x the parallel passes' rows are to differ by"""
    if not _PAR:
        import jpeg_par_corpus as pc
        from test_jpeg_decode import picture, pil_jpeg
        w, h = 512, 384
        data = pil_jpeg(picture(w, h, seed=21, noise=40.0)[..., 0], quality=95)
        _PAR.extend(pc.corpus() + [pc.Case("pillow_long_gray", data, w, h, 4, None, 0, {"pillow": True})])
    return list(_PAR)


def overruns(c):
    """a file of the extra-blocks, short and cut kinds: its scan holds more blocks than its frame, ends short of them, or carries
    bytes behind them that the kernels must not decode into a neighbour"""
    return "extra_blocks" in c.props or c.name.startswith("cut_") or c.name in ("tail_after_eoi", "tail_behind_rst", "tail_noise_in_scan")


def interleaved(cases):
    """an order that alternates the sampling classes and, within its class, puts every overruns() file directly before a decodable
    file of another shape (the records of a class follow the call's order)"""
    by_class = {}
    for c in cases:
        by_class.setdefault(c.ratio, []).append(c)
    lists = []
    for ratio, cs in sorted(by_class.items()):
        bad = [c for c in cs if overruns(c)]
        spare = [c for c in cs if not overruns(c) and c.status == 0]
        rest = [c for c in cs if not overruns(c) and c.status != 0]
        out, shapes_used = [], set()
        for b in bad:
            # a decodable neighbour of another shape, a new shape each time while there is one
            pick = next((c for c in spare if (c.w, c.h) != (b.w, b.h) and (c.w, c.h) not in shapes_used), None) or \
                next(c for c in spare if (c.w, c.h) != (b.w, b.h))
            spare.remove(pick)
            shapes_used.add((pick.w, pick.h))
            out += [b, pick]
        # the others behind them, largest and smallest scans alternating
        spare.sort(key=lambda c: len(c.data))
        while spare:
            out.append(spare.pop())
            if spare:
                out.append(spare.pop(0))
            if rest:
                out.append(rest.pop())
        lists.append(out + rest)
    order = []
    while any(lists):
        for l in lists:
            if l:
                order.append(l.pop(0))
    return order


def behind_in_class(order, i):
    """the next file of order[i]'s class"""
    return next((c for c in order[i + 1:] if c.ratio == order[i].ratio), None)


def scan_spread(cases):
    """{class: (shortest, longest)} scan of the files that take the parallel route"""
    import jpeg_par_corpus as pc
    out = {}
    for c in cases:
        if c.par:
            n = pc.scan_of(c.data)[1]
            lo, hi = out.get(c.ratio, (n, n))
            out[c.ratio] = (min(lo, n), max(hi, n))
    return out


def shuffled(cases, seed):
    perm = list(range(len(cases)))
    random.Random(seed).shuffle(perm)
    return perm


def edge_mix():
    """tests/jpeg_edge_corpus.py with one Pillow file per class between its files -> [(name, bytes)]"""
    import jpeg_edge_corpus as je
    from test_jpeg_mixed_gpu import make
    twins = [("twin_" + cls, make(w, h, cls, seed=300 + k)) for k, (cls, (w, h)) in
             enumerate((("gray", (23, 45)), ("420", (70, 37)), ("422", (50, 19)), ("440", (40, 24)), ("444", (37, 21))))]
    cases = [(c.name, c.data) for c in je.corpus()]
    step = len(cases) // len(twins)
    out = []
    for k, c in enumerate(cases):
        out.append(c)
        if k % step == step - 1 and twins:
            out.append(twins.pop(0))
    return out + twins


HOST_SIZES = [(17, 17), (257, 40), (64, 48), (200, 120), (33, 15)]
HOST_CLASS = "420"


def host_route_files(reverse=False):
    """five progressive files (the host route) of one class with two baseline files between them -> (files, indices of the host files)"""
    from test_jpeg_mixed_gpu import make
    prog = [make(w, h, HOST_CLASS, seed=500 + k, progressive=True) for k, (w, h) in enumerate(HOST_SIZES)]
    if reverse:
        prog = prog[::-1]
    base = [make(129, 65, HOST_CLASS, seed=510), make(9, 7, HOST_CLASS, seed=511)]
    files = [prog[0], prog[1], base[0], prog[2], prog[3], base[1], prog[4]]
    return files, [0, 1, 3, 4, 6]


def host_group_words(sizes, group):
    """the int16 words dec_upload stages per group of host-route files: 65 per block (4:2:0: six blocks per 16 x 16 MCU)"""
    words = [((w + 15) // 16) * ((h + 15) // 16) * 6 * 65 for w, h in sizes]
    return [sum(words[g:g + group]) for g in range(0, len(words), group)]


# ---- the JPEG leg ----------------------------------------------------------------------------------------------------------------

LEG_CLASSES = ["gray", "420", "422", "440", "444"]


def leg_classes_case():
    """B1: every class x two sizes x {baseline, progressive}, interleaved -> (files, sizes)"""
    from test_jpeg_mixed_gpu import make
    files, sizes = [], []
    for i in range(20):
        cls, (w, h), prog = LEG_CLASSES[i % 5], ((33, 15), (64, 48))[(i // 5) % 2], i >= 10
        files.append(make(w, h, cls, seed=800 + i, **({"progressive": True} if prog else {})))
        sizes.append((w, h, cls))
    return files, sizes


def damage(f):
    """test_jpeg_mixed_gpu.bad_code_file's damage on any baseline file: thirty-two 1 bits in the middle of the scan"""
    from test_jpeg_mixed_gpu import entropy_segment
    b = bytearray(f)
    at = len(b) - 2 - len(entropy_segment(f)) // 2
    b[at:at + 8] = b"\xff\x00" * 4
    return bytes(b)


RUN_SIZE = (129, 65, "420")
RUN_VARIANTS = {"first": (0,), "last": (3,), "all-but-one": (0, 1, 3)}


def run_ends_case(variant):
    """B2: four files of one size and class (a run; ties sort by index) with runs of two other sizes around them, the files named by
    the variant damaged in their scans -> (files, sizes, positions of the damaged files, positions of the run)"""
    from test_jpeg_mixed_gpu import make
    w, h, cls = RUN_SIZE
    run = [make(w, h, cls, seed=900 + k) for k in range(4)]
    for k in RUN_VARIANTS[variant]:
        run[k] = damage(run[k])
    small = [make(64, 48, cls, seed=910 + k) for k in range(2)]       # sorts before the run
    large = [make(200, 120, cls, seed=920 + k) for k in range(2)]     # and behind it
    files = [large[0], run[0], small[0], run[1], run[2], large[1], run[3], small[1]]
    sizes = [(200, 120, cls), RUN_SIZE, (64, 48, cls), RUN_SIZE, RUN_SIZE, (200, 120, cls), RUN_SIZE, (64, 48, cls)]
    at = [1, 3, 4, 6]
    return files, sizes, [at[k] for k in RUN_VARIANTS[variant]], at


EMPTY_SIZE = (600, 1)


def empty_output_case(where):
    """B4: a 600 x 1 file (kept in aspect inside 64 x 48 its resize output has no rows) first, in the middle or last among files whose
    outputs have one size -> (files, sizes, its position)"""
    from test_jpeg_mixed_gpu import make
    # the leg orders a chunk's files by (width, height, class): 64 x 48 sorts before 600 x 1 and 640 x 480 behind it, and both are 64 x 48
    # after the resize, so that without the wide file the chunk's resize outputs are encoded in one launch
    before, behind = {"first": (0, 4), "middle": (2, 2), "last": (4, 0)}[where]
    sizes = [(64, 48, "420")] * before + [EMPTY_SIZE + ("420",)] + [(640, 480, "420")] * behind
    files = [make(w, h, cls, seed=950 + k) for k, (w, h, cls) in enumerate(sizes)]
    # in the call the wide file stands where it does NOT stand in the sorted chunk
    at = {"first": 4, "middle": 0, "last": 2}[where]
    files.insert(at, files.pop(before))
    sizes.insert(at, sizes.pop(before))
    return files, sizes, at


def sorted_position(sizes, at):
    """where the leg's order (width, height, class; ties by index) puts file `at`"""
    order = sorted(range(len(sizes)), key=lambda i: (sizes[i][0], sizes[i][1], i))
    return order.index(at)


# ---- PNG encode ------------------------------------------------------------------------------------------------------------------

GRID_X = 1 << 20                    # png_mixed_filter_kernel's grid: 2^20 workgroups in x, one per row
TALL = (1, 65535)                   # w, h
TALL_TIMES = 17
OPACITY_WGS = 512                   # png_mixed_opaque_kernel: min(512, ceil(pixels / 4096)) workgroups per frame
BIG = (2048, 1025)
SECOND_SWEEP = OPACITY_WGS * 256    # the first pixel beyond the first sweep of 512 workgroups of 256 lanes


def tall_frames():
    """C1's two distinct frames, 1 x 65535 premultiplied RGBA: opaque, and with one alpha byte 0xfe in the last row"""
    w, h = TALL
    y = np.arange(h)
    f = np.empty((h, w, 4), np.uint8)
    f[:, 0, 0], f[:, 0, 1], f[:, 0, 2], f[:, 0, 3] = (y >> 4) & 0xFF, (y * 7 >> 6) & 0xFF, 0x55, 0xFF
    g = f.copy()
    g[h - 1, 0] = (0x10, 0x20, 0xFE, 0xFE)
    return f, g


def grid_heights():
    """the heights of C1's call in order: 3 x 2 first, the tall frames 17 times, 1 x 1 last"""
    return [2] + [TALL[1]] * TALL_TIMES + [1]


def row0s(heights):
    out, at = [], 0
    for h in heights:
        out.append(at)
        at += h
    return out, at


def big_frame(alpha_at=None):
    """C2's 2048 x 1025 frame, gently varying; alpha_at: None (opaque), or the pixel index whose alpha is 0xfe"""
    w, h = BIG
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.uint8)
    f[..., 0], f[..., 1], f[..., 2], f[..., 3] = (yy >> 2) & 0xFF, (xx >> 3) & 0xFF, 7, 0xFF
    if alpha_at is not None:
        f.reshape(-1, 4)[alpha_at] = (0x10, 0x20, 0xFE, 0xFE)
    return f


def opacity_blocks(w, h):
    return (w * h + 4095) // 4096


# ---- PNG decode ------------------------------------------------------------------------------------------------------------------


def png_edge_mix(shipped):
    """D1: tests/png_edge_corpus.py's files between the files of the shipped mixed call, one after every fourth"""
    import png_edge_corpus as pe
    edge = [c.data for c in pe.corpus()]
    out, k = [], 0
    for i, f in enumerate(shipped):
        out.append(f)
        if i % 4 == 3 and k < len(edge):
            out.append(edge[k])
            k += 1
    return out + edge[k:], len(edge)


def png_par_mix():
    """D2: tests/png_par_corpus.py's files with the cases of its edge sizes, and five small files of other kinds (two paletted)
    between them -> ([(name, bytes, the corpus case | None)], names left out)"""
    import png_corpus as pc
    import png_edge_corpus as pe
    import png_par_corpus as ppc
    large = {c.name for c in pe.large()}
    cases = ppc.corpus(edges=True)
    keep = [c for c in cases if c.name not in large]
    left_out = [c.name for c in cases if c.name in large]
    small = [("small pal8 5x1", pc.of_type(3, 8, True, 1, 5, seed=71, kind="photo")), ("small gray16 33x7", pc.of_type(0, 16, False, 7, 33, seed=72)),
             ("small pal4 33x7", pc.of_type(3, 4, True, 7, 33, seed=73, kind="flat")), ("small rgba8 1x1", pc.of_type(6, 8, False, 1, 1, seed=74)),
             ("small rgb16 9x9", pc.of_type(2, 16, False, 9, 9, seed=75))]
    out, step = [], max(1, len(keep) // len(small))
    for k, c in enumerate(keep):
        out.append((c.name, c.data, c))
        if k % step == step - 1 and small:
            name, data = small.pop(0)
            out.append((name, data, None))
    out += [(name, data, None) for name, data in small]
    return out, left_out


ADAM7_SIZES = [(7, 33), (64, 48), (5, 1)]      # h, w


def adam7_pairs():
    """D3: Adam7 files of three sizes and kinds, each beside its non-interlaced twin -> [(interlaced, twin)]"""
    import png_adam7_corpus as ac
    types = [(2, 8, False), (6, 8, False), (0, 8, False)]
    return [(ac.of_type(*types[k], h, w, seed=40 + k), ac.of_type(*types[k], h, w, seed=40 + k, interlace=False)) for k, (h, w) in enumerate(ADAM7_SIZES)]
