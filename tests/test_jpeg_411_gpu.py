"""ipx_jpeg_decode_batch on 4:1:1 and 4:1:0 files (IPX_JPEG_411=1) against tests/jpeg_411_model.py: planes, sizes, ratio and statuses,
every byte of the MCU-padded planes.  tests/test_jpeg_411_model.py pins the model.

Sizes (tests/jpeg_411_corpus.py SIZES): 1x1, 31x7, 32x8, 33x9, 65x17; widths of one MCU fewer than, exactly and one more than the MCUs a
workgroup of jpeg_idct_kernel takes (8 for the six-block MCUs of 4:1:1, 4 for the ten-block MCUs of 4:1:0), with heights either side
of an MCU row.  Every size is decoded as one baseline scan (the piece kernels), with restart intervals of one MCU and of one MCU row
(one lane per interval), as a multi-scan non-interleaved file and as a progressive file (both on the host-scans route).  Scans long
enough for the decoder that is parallel inside a scan (>= 4 KiB) go through the par_* kernels, and the byte-wise jpeg_huff_kernel is
reached with IPX_JPEG_PIECE=0.  Without the feature every file here is IPX_ERR_UNSUPPORTED under the switch too: all tests but the
switch-off ones fail."""
import numpy as np
import pytest

import jpeg_411_corpus as c4
import jpeg_411_model as model

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -4
PAR, HOST = 0, 1


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("IPX_JPEG_411", "1")


def variants(w, h, v0, seed=0):
    """-> [(name, file, the model's planes, route)] of one frame size"""
    fr = c4.frame(w, h, v0)
    out = []
    for k, (name, make, route) in enumerate((("baseline", lambda b: c4.baseline(fr, b), PAR), ("restart every MCU", lambda b: c4.baseline(fr, b, ri=1), PAR),
                                             ("restart every MCU row", lambda b: c4.baseline(fr, b, ri=fr.mxx), PAR),
                                             ("multi-scan", lambda b: c4.multiscan(fr, b), HOST), ("progressive", lambda b: c4.progressive(fr, b), HOST))):
        b = c4.blocks(fr, 1000 * v0 + 31 * w + h + k + seed)
        data = make(b)
        want = model.from_blocks(fr, b, c4.Q, progressive=True) if name == "progressive" else model.decode(data)
        out.append((name, data, want, route))
    return out


def check(ctx, cases, w, h, v0):
    counts = ctx.jpeg_decode_counts()
    info, st = ctx.jpeg_decode_batch([c[1] for c in cases])
    assert st == [OK] * len(cases)
    mxx, myy = (w + 31) // 32, (h + 8 * v0 - 1) // (8 * v0)
    assert (info["w"], info["h"], info["ratio"]) == (w, h, model.RATIO_411 if v0 == 1 else model.RATIO_410)
    assert (info["ystride"], info["cstride"]) == (32 * mxx, 8 * mxx)
    assert info["y"].shape[1:] == (8 * v0 * myy, 32 * mxx) and info["cb"].shape[1:] == info["cr"].shape[1:] == (8 * myy, 8 * mxx)
    for i, (name, _, want, _) in enumerate(cases):
        for k in ("y", "cb", "cr"):
            np.testing.assert_array_equal(info[k][i], want[k], err_msg="%s: plane %s" % (name, k))
    routes = [a - b for a, b in zip(ctx.jpeg_decode_counts(), counts)]
    assert routes[:3] == [sum(c[3] == PAR for c in cases), sum(c[3] == HOST for c in cases), 0]


@pytest.mark.parametrize("v0,w,h", [(v0, w, h) for v0 in (1, 2) for w, h in c4.SIZES[v0]])
def test_every_kind_of_file_at_the_edge_sizes(ctx, on, monkeypatch, v0, w, h):
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")              # the scan walk does not take these shapes: the progressive file stays on the host
    check(ctx, variants(w, h, v0), w, h, v0)


@pytest.mark.parametrize("v0", [1, 2])
@pytest.mark.parametrize("sub", ["128", "1024"])
def test_long_scans_through_the_parallel_decoder(ctx, on, monkeypatch, v0, sub):
    """scans of 4 KiB and more without restart markers: par_count / par_unstuff / par_sync / par_write / par_dc, with six and ten blocks
    per MCU (the DC sums of par_dc_kernel run over four or eight luma blocks)"""
    monkeypatch.setenv("IPX_JPEG_PAR_SUB", sub)
    w, h = 9 * 32 + 5, 41
    fr = c4.frame(w, h, v0)
    cases = []
    for k in range(3):
        b = c4.blocks(fr, 77 + k + v0, amp=300, ac=60, density=0.5)
        data = c4.baseline(fr, b)
        assert c4.scan_len(data) >= 4 * 1024
        cases.append(("long scan %d" % k, data, model.from_blocks(fr, b, c4.Q), PAR))
    check(ctx, cases, w, h, v0)


@pytest.mark.parametrize("v0", [1, 2])
def test_the_byte_wise_kernel(ctx, on, monkeypatch, v0):
    monkeypatch.setenv("IPX_JPEG_PIECE", "0")                 # jpeg_huff_kernel instead of the piece kernels
    w, h = 65, 17
    check(ctx, [v for v in variants(w, h, v0, seed=5) if v[3] == PAR], w, h, v0)


def mixed_batch():
    """4:1:1 files with a 4:2:0 and a 4:1:0 file of the same size among them, and a 4:1:1 file cut inside its scan"""
    w, h = 65, 17
    cases = variants(w, h, 1, seed=9)
    f420 = c4.frame(w, h, 2, h0=2)
    other = [c4.baseline(f420, c4.blocks(f420, 4)), variants(w, h, 2, seed=9)[0][1]]
    cut = c4.cut_in_scan(cases[0][1])
    files = [cases[0][1], other[0], cases[1][1], cases[3][1], other[1], cut, cases[4][1]]
    wants = {0: cases[0][2], 2: cases[1][2], 3: cases[3][2], 6: cases[4][2]}
    return w, h, files, wants, cut


def test_a_batch_is_one_shape_and_a_cut_file_takes_the_models_status(ctx, on):
    w, h, files, wants, cut = mixed_batch()
    assert model.status_of(cut) == INVALID
    info, st = ctx.jpeg_decode_batch(files)
    assert st == [OK, UNSUPPORTED, OK, OK, UNSUPPORTED, INVALID, OK]
    assert (info["w"], info["h"], info["ratio"]) == (w, h, model.RATIO_411)
    for i, want in wants.items():
        for k in ("y", "cb", "cr"):
            np.testing.assert_array_equal(info[k][i], want[k], err_msg="file %d plane %s" % (i, k))
    # the 4:2:0 file first: the batch is 4:2:0 and every 4:1:x file is handed back
    info, st = ctx.jpeg_decode_batch([files[1]] + files)
    assert st == [OK, UNSUPPORTED, OK, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, INVALID, UNSUPPORTED] and info["ratio"] == 2
    np.testing.assert_array_equal(info["y"][0], info["y"][2])


@pytest.mark.parametrize("value", [None, "0", "2"])
def test_switch_off_everything_is_unsupported(ctx, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_411", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_411", value)
    counts = ctx.jpeg_decode_counts()
    for v0 in (1, 2):
        for w, h in ((1, 1), (33, 9), (65, 17)):
            info, st = ctx.jpeg_decode_batch([c[1] for c in variants(w, h, v0)])
            assert info is None and st == [UNSUPPORTED] * 5
    w, h, files, wants, cut = mixed_batch()
    info, st = ctx.jpeg_decode_batch(files)
    # the files of the two shapes are refused at the frame header, the cut one included (UNSUPPORTED is the parser's first verdict);
    # the 4:2:0 file is the batch
    assert st == [UNSUPPORTED, OK, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, UNSUPPORTED] and info["ratio"] == 2
    assert [a - b for a, b in zip(ctx.jpeg_decode_counts(), counts)] == [1, 0, 0, 0]
