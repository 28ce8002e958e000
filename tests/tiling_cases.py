"""The tilings ks_fused_plan picks by itself for wide frames: the case table of tests/test_tilings_gpu.py, with the class each case
claims per tile size, and the upload sizes whose classes the table has to cover (tests/test_ks_plan_host.py holds the two together
through tools/ks_plan_check.cpp, without a GPU).

A tile pixel has 4 bytes for RGBA frames, 2 for Gray and 8 for every other source type.  A plan's class is
(tile bytes, nacc, strips as 1 / 2 / 3 = three and more, dbuf, the float pass's dbuf, its list entries per wave, most lanes per column)."""

TILE_BYTES = (4, 8, 2)


def tile_bytes(kind):
    return 4 if kind == "rgba" else 2 if kind == "gray" else 8


# ((sw, sh, (resize w, h, keep aspect), (thumbnail size, crop to fit)), frames,
#  {tile bytes: (nacc, strips, dbuf, float pass dbuf, list entries per wave, lanes per column)})
# Wide and short: the tiling follows the width, the height only adds rows.  Every width is a multiple of 4 (the one-pass kernel's
# condition for the planar and deep types).
def _c(shape, c4, c8, c2, frames=2):
    return (shape, frames, {4: c4, 8: c8, 2: c2})


CASES = [
    # the class of 4032 x 3024 uploads; a 32-tap thumbnail on two lanes per column
    _c((4032, 48, (1024, 48, False), (3, False)), (2, 2, 1, 1, 128, 2), (2, 2, 0, 0, 128, 2), (2, 2, 1, 1, 128, 2)),
    # three natural strips; the 8-byte float layout takes 158 672 bytes with lists of 64
    _c((5000, 40, (1024, 40, False), (5, False)), (2, 3, 1, 1, 128, 1), (2, 3, 0, 1, 64, 1), (2, 3, 1, 1, 128, 1)),
    # two columns per lane on both outputs, 16 taps each
    _c((8064, 40, (1024, 40, False), (5, False)), (2, 4, 1, 1, 128, 1), (2, 4, 0, 0, 128, 1), (2, 4, 1, 1, 128, 1)),
    # a 2x upscale: four accumulators, 576 columns per strip
    _c((2000, 32, (4000, 64, False), (8, False)), (4, 7, 1, 1, 128, 1), (4, 7, 1, 1, 128, 1), (4, 7, 1, 1, 128, 1)),
    # 33 taps (odd: the second lane's padded tap); the 8-byte float64 layout takes 147 760 of 153 600 bytes
    _c((3000, 32, (1024, 32, False), (2, False)), (2, 2, 1, 1, 128, 2), (2, 2, 1, 1, 128, 2), (2, 2, 1, 1, 128, 2)),
    # eight strips; the thumbnail's 12 columns lie inside one of them; 8-byte float layout 162 688 bytes
    _c((16380, 12, (2048, 12, False), (12, True)), (2, 8, 1, 1, 128, 1), (2, 8, 0, 1, 128, 1), (2, 8, 1, 1, 128, 1)),
    # three row segments; the crop thumbnail's top-byte taps; 162 544 bytes
    _c((4032, 256, (1024, 64, False), (64, True)), (2, 2, 1, 1, 128, 1), (2, 2, 0, 1, 128, 1), (2, 2, 1, 1, 128, 1)),
    # four accumulators with one tile buffer; the 8-byte float layout takes 163 152 of 163 328 bytes
    _c((8000, 16, (2000, 32, False), (32, True)), (4, 4, 1, 1, 128, 1), (4, 4, 0, 1, 64, 1), (4, 4, 1, 1, 128, 1)),
    # stand-ins for the classes uploads reach and the cases above do not
    _c((4380, 52, (1095, 52, False), (16, False)), (2, 2, 1, 1, 128, 1), (2, 2, 0, 0, 128, 1), (2, 2, 1, 1, 128, 1)),
    _c((3800, 64, (1266, 64, False), (2, True)), (2, 2, 1, 1, 128, 2), (2, 2, 0, 1, 128, 2), (2, 2, 1, 1, 128, 2)),
    _c((6068, 16, (800, 16, False), (1, True)), (2, 3, 1, 1, 128, 2), (2, 3, 0, 0, 128, 2), (2, 3, 1, 1, 128, 2)),
    _c((7220, 52, (800, 52, False), (20, True)), (2, 4, 1, 1, 128, 2), (2, 4, 0, 1, 128, 2), (2, 4, 1, 1, 128, 2)),
    _c((6460, 36, (800, 36, False), (15, True)), (2, 4, 1, 1, 128, 2), (2, 4, 1, 1, 128, 2), (2, 4, 1, 1, 128, 2)),
    # the class of 3840 x 2160 uploads with the default operators: lists of 64 and two lanes per column
    _c((3520, 24, (800, 24, False), (2, False)), (2, 2, 1, 1, 128, 2), (2, 2, 0, 1, 64, 2), (2, 2, 1, 1, 128, 2)),
    # the class of 2560 x 1440 uploads: two strips, two tile buffers in both layouts of the 8-byte tile
    _c((2400, 24, (1024, 24, False), (4, False)), (2, 2, 1, 1, 128, 1), (2, 2, 1, 1, 128, 1), (2, 2, 1, 1, 128, 1)),
    # a mild downscale (three taps): 908 columns per strip make three strips whose tiles fit twice; the sweep's most frequent class
    _c((3600, 20, (2700, 20, False), (4, False)), (2, 3, 1, 1, 128, 1), (2, 3, 1, 1, 128, 1), (2, 3, 1, 1, 128, 1)),
]

# Sizes uploads come in, each with the operator sets below.
UPLOAD_SIZES = [(640, 480), (800, 600), (1280, 720), (1920, 1080), (2560, 1440), (3000, 2000), (3264, 2448), (3840, 2160), (4000, 3000),
                (4032, 3024), (4608, 3456), (5472, 3648), (6000, 4000), (7680, 4320), (8192, 5464), (9248, 6936),
                (1080, 1920), (2160, 3840), (3024, 4032)]
UPLOAD_OPS = [((1024, 768, keep), (200, crop)) for keep in (False, True) for crop in (True, False)] + [((800, 600, False), (150, True))]
UPLOAD_MIN_WIDTH = 2560      # the classes of uploads at least this wide must each be run by some case


# Two real files go through the batch entry at a size where the decoded planes' MCU-padded stride (4048 at 4:2:0, 4040 at 4:4:4) is
# not the width: two strips and one tile buffer in both layouts of the 8-byte tile.
JPEG_CASE = ((4036, 40, (1024, 40, False), (2, False)), (2, 2, 0, 0, 128, 2))


def klass(px, claim):
    nacc, strips, dbuf, fdbuf, per_wave, lanes = claim
    return (px, nacc, min(strips, 3), dbuf, fdbuf, per_wave, lanes)


def shape_line(tag, sw, sh, resize, thumb):
    """one line of ks_plan_check's input"""
    return "%s %d %d 1 %d %d %d 1 %d %d" % (tag, sw, sh, resize[0], resize[1], int(resize[2]), thumb[0], int(thumb[1]))


def upload_shapes():
    """-> [(tag, sw, sh, resize, thumbnail)]"""
    return [("upload:%dx%d:%d" % (w, h, i), w, h, r, t) for (w, h) in UPLOAD_SIZES for i, (r, t) in enumerate(UPLOAD_OPS)]
