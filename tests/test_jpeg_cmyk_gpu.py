"""ipx_jpeg_decode_batch_cmyk on the GPU (IPX_JPEG_CMYK=1, csrc/ipx_jpeg_dec_cmyk.hip) against tests/jpeg_cmyk_model.py, every byte.

The shapes are the smallest at which MCU padding, the quadrant mapping of K's blocks or a lane's tail of fewer than four pixels can go
wrong: vector 11 11 11 11 at 1x1, 8x8, 9x7, 65x3; vector 22 11 11 22 at 16x16, 17x15, 33x31, 1x1.  tests/test_jpeg_cmyk_model.py pins
the model.  Without the feature these tests fail: the entry does not exist.

ASSEMBLE_SHAPES are the edges of jpeg_cmyk_assemble_kernel itself: a lane takes 4 pixels of 4 rows, a workgroup 1024 columns, 16 bytes are
stored at once iff the frame's rows are 16-byte aligned and all four pixels exist, and the rows past the image load row h - 1 again.  The
group tests are the driver's: host-decoded files go up in double-buffered pinned groups of IPX_JPEG_HOST_GROUP (16) files, and from the
third group on a half is taken again after the wait for its event."""
import numpy as np
import pytest

import jpeg_cmyk_model as model
import jpeg_cmyk_writer as cw
import jpeg_prog_writer as pw

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -4
SHAPES = [(1, 1, 1), (8, 8, 1), (9, 7, 1), (65, 3, 1), (16, 16, 2), (17, 15, 2), (33, 31, 2), (1, 1, 2)]
ASSEMBLE_SHAPES = [(2, 2, 1), (3, 6, 1),            # w % 4 = 2 and 3 in a single lane, h % 4 = 2
                   (12, 5, 1), (20, 10, 1),         # the 16-byte store in a row's last lane, 4 bytes of plane padding behind its loads
                   (1028, 6, 1),                    # lane 256: the first lane of a second workgroup in x, on the 16-byte path
                   (1027, 2, 1),                    # the same pixel by pixel, with a tail of 3 pixels; two of four rows loaded past h
                   (2, 2, 2), (6, 6, 2), (19, 13, 2),   # word loads of chroma at x >> 1 with tails of 2 and 3 pixels, h % 4 = 1 and 2
                   (12, 10, 2),                     # 4:2:0 rows y >> 1, the 16-byte store before padding
                   (1028, 6, 2), (1030, 5, 2)]      # a second workgroup at 4:2:0, 16-byte stores and ragged


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("IPX_JPEG_CMYK", "1")


def case(w, h, v, transform, progressive=False, dri=0, seed=0):
    """-> (file, the model's *image.CMYK pixels)"""
    f = cw.frame4(w, h, v)
    b = cw.blocks4(f, 500 + seed + 7 * w + v)
    return cw.cmyk_file(f, b, transform=transform, progressive=progressive, dri=dri), model.from_blocks(f, b, cw.quants(), transform, progressive)["pix"]


@pytest.mark.parametrize("w,h,v", SHAPES + ASSEMBLE_SHAPES)
def test_both_transforms_at_the_edge_shapes(ctx, on, w, h, v):
    cases = [case(w, h, v, t, seed=s) for s, t in enumerate((0, 2, 1, 0))]       # one batch mixes CMYK and YCCK files
    before = ctx.jpeg_cmyk_files()
    info, st = ctx.jpeg_decode_batch_cmyk([c[0] for c in cases])
    assert st == [OK] * 4
    assert (info["w"], info["h"], info["stride"]) == (w, h, 4 * w)
    for i, (_, want) in enumerate(cases):
        np.testing.assert_array_equal(info["pix"][i], want, err_msg="file %d" % i)
    assert ctx.jpeg_cmyk_files() - before == 4


@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("transform", [0, 2])
def test_baseline_restart_intervals_and_progressive(ctx, on, v, transform):
    cases = [case(17, 15, v, transform), case(17, 15, v, transform, dri=1, seed=1), case(17, 15, v, transform, progressive=True, seed=2)]
    info, st = ctx.jpeg_decode_batch_cmyk([c[0] for c in cases], 17, 15)
    assert st == [OK] * 3
    for i, (_, want) in enumerate(cases):
        np.testing.assert_array_equal(info["pix"][i], want, err_msg="file %d" % i)


def test_a_batch_that_mixes_good_files_with_refused_ones(ctx, on):
    good = [case(17, 15, 2, 2, seed=3), case(17, 15, 2, 0, progressive=True, seed=4)]
    f = cw.frame4(17, 15, 2)
    fi = cw.frame4(17, 15, hv=cw.ILLEGAL_VECTORS["22 11 11 11"])
    f3 = pw.colour_frame(17, 15, 2, 2)
    files = [good[0][0][:len(good[0][0]) * 2 // 3],                         # truncated in its scan
             good[0][0],
             cw.cmyk_file(fi, cw.blocks4(fi, 9)),                           # Pillow's subsampling=2 vector
             cw.cmyk_file(f, cw.blocks4(f, 10), app14="absent"),
             good[1][0],
             pw.baseline(f3, pw._blocks(f3, 11))]                           # a three-component file: ipx_jpeg_decode_batch's
    before = ctx.jpeg_cmyk_files()
    info, st = ctx.jpeg_decode_batch_cmyk(files)
    assert st == [INVALID, OK, UNSUPPORTED, UNSUPPORTED, OK, UNSUPPORTED]
    np.testing.assert_array_equal(info["pix"][1], good[0][1])
    np.testing.assert_array_equal(info["pix"][4], good[1][1])
    assert ctx.jpeg_cmyk_files() - before == 4                              # the two good files, the truncated one, the one without APP14


@pytest.mark.parametrize("group", ["1", "2"])
def test_host_decoded_files_in_small_groups(ctx, on, group, monkeypatch):
    """Seven files, five of which reach the host decoder (`todo`), in groups of one and of two: five and three groups, so both pinned
    halves are taken again after the wait for their events.  The files the parse refuses come first and in between, so a decodable
    file's index in the call (its planes, tables and status) is never its index in `todo` (its pinned slot); the file that fails in
    its scan sits in a middle group, and its slot is not sent up."""
    good = {0: case(17, 15, 2, 2, seed=3), 2: case(17, 15, 2, 0, dri=1, seed=5), 5: case(17, 15, 2, 1, progressive=True, seed=6),
            6: case(17, 15, 2, 0, seed=7)}
    fi = cw.frame4(17, 15, hv=cw.ILLEGAL_VECTORS["22 11 11 11"])
    f3 = pw.colour_frame(17, 15, 2, 2)
    whole = good[0][0]
    cut = whole[:len(whole) * 2 // 3]
    assert whole.index(b"\xff\xda") + 14 < len(cut)          # truncated inside its scan, not its headers
    files = [whole,
             cw.cmyk_file(fi, cw.blocks4(fi, 9)),                           # refused by the parse: not in `todo`
             good[2][0],
             pw.baseline(f3, pw._blocks(f3, 11)),                           # a three-component file: not in `todo`
             cut,                                                           # `todo` index 2 of 0 .. 4: a middle group at either size
             good[5][0],
             good[6][0]]
    monkeypatch.setenv("IPX_JPEG_HOST_GROUP", group)
    before = ctx.jpeg_cmyk_files()
    info, st = ctx.jpeg_decode_batch_cmyk(files)
    assert st == [OK, UNSUPPORTED, OK, UNSUPPORTED, INVALID, OK, OK]
    assert (info["w"], info["h"], info["stride"]) == (17, 15, 68)
    for i, (_, want) in good.items():
        np.testing.assert_array_equal(info["pix"][i], want, err_msg="file %d in groups of %s" % (i, group))
    assert ctx.jpeg_cmyk_files() - before == 5                              # the four good files and the truncated one


def test_three_groups_of_the_default_size(ctx, on, monkeypatch):
    """33 files at the default group size: 16 + 16 + 1, the third group in the first half again."""
    monkeypatch.delenv("IPX_JPEG_HOST_GROUP", raising=False)
    cases = [case(8, 8, 1, (0, 2, 1)[s % 3], seed=s) for s in range(33)]
    assert len({c[0] for c in cases}) == 33 and len({c[1].tobytes() for c in cases}) == 33
    before = ctx.jpeg_cmyk_files()
    info, st = ctx.jpeg_decode_batch_cmyk([c[0] for c in cases])
    assert st == [OK] * 33
    for i, (_, want) in enumerate(cases):
        np.testing.assert_array_equal(info["pix"][i], want, err_msg="file %d" % i)
    assert ctx.jpeg_cmyk_files() - before == 33


def test_files_of_another_size_or_vector_are_left_to_the_caller(ctx, on):
    a, b, c = case(16, 16, 2, 0), case(16, 16, 1, 0, seed=1), case(17, 15, 2, 0, seed=2)
    info, st = ctx.jpeg_decode_batch_cmyk([a[0], b[0], c[0]])
    assert st == [OK, UNSUPPORTED, UNSUPPORTED]
    np.testing.assert_array_equal(info["pix"][0], a[1])
    info, st = ctx.jpeg_decode_batch_cmyk([a[0], b[0], c[0]], 17, 15)
    assert st == [UNSUPPORTED, UNSUPPORTED, OK]
    np.testing.assert_array_equal(info["pix"][2], c[1])


@pytest.mark.parametrize("value", [None, "0", "yes"])
def test_switch_off(ctx, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_CMYK", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_CMYK", value)
    f3 = pw.colour_frame(16, 16, 2, 2)
    three = pw.baseline(f3, pw._blocks(f3, 12))
    files = [case(16, 16, 2, 0)[0], case(16, 16, 1, 2)[0], three]
    cmyk, counts = ctx.jpeg_cmyk_files(), ctx.jpeg_decode_counts()
    info, st = ctx.jpeg_decode_batch_cmyk(files)
    assert info is None and st == [UNSUPPORTED] * 3
    info, st = ctx.jpeg_decode_batch(files)
    assert st == [UNSUPPORTED, UNSUPPORTED, OK]
    assert ctx.jpeg_cmyk_files() == cmyk
    rose = [x - y for x, y in zip(ctx.jpeg_decode_counts(), counts)]
    assert sum(rose[:3]) == 1 and rose[3] == 0, rose          # the three-component file reached a decoder, the others none


def test_the_other_decode_entry_refuses_these_files_under_the_switch_too(ctx, on):
    f3 = pw.colour_frame(16, 16, 2, 2)
    three = pw.baseline(f3, pw._blocks(f3, 12))
    info, st = ctx.jpeg_decode_batch([case(16, 16, 2, 0)[0], three])
    assert st == [UNSUPPORTED, OK]
