"""Branches of the JPEG decode driver (csrc/ipx_jpeg_dec_runtime.hip) that the default settings never enter: the re-use of the two
pinned halves that host-decoded files go up through (IPX_JPEG_HOST_GROUP), the stream-ordered allocation route without a lane arena
(IPX_JPEG_LANE_ARENA=0) and the hand-over of the parallel images to the byte-wise kernel when the passes do not settle
(IPX_JPEG_PAR_ROUNDS).  Each batch is compared exactly against oracle.jpeg_decode and against the same call with the variable unset.
"""
import numpy as np
import pytest

import oracle
from test_jpeg_decode import _check_batch, picture, pil_jpeg


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


def _same_planes(a, b):
    (ia, sa), (ib, sb) = a, b
    assert sa == sb
    assert (ia["w"], ia["h"], ia["ratio"]) == (ib["w"], ib["h"], ib["ratio"])
    for i, st in enumerate(sa):
        if st == 0:
            for k in ("y", "cb", "cr"):
                np.testing.assert_array_equal(ia[k][i], ib[k][i], err_msg="%s of file %d" % (k, i))


def _streams(ctx, files, w, h):
    plan = ctx.plan(w, h, resize=(64, 48, True), thumbnail=(32, True))
    try:
        return plan.run_jpeg_jpeg(files)
    finally:
        plan.close()


def _entropy_segment(f):
    """The entropy-coded bytes of a one-scan file: from the end of the SOS header to EOI."""
    sos = f.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(f[sos + 2:sos + 4], "big")
    assert f[-2:] == b"\xff\xd9"
    return f[start:-2]


@pytest.mark.gpu
def test_host_decoded_files_in_groups_of_two(ctx, monkeypatch):
    """Ten progressive files in groups of two: five groups, so each pinned half is taken again after the wait for its event, and one
    file fails in its scans inside a group."""
    w, h = 96, 64
    prog = [pil_jpeg(picture(w, h, seed=80 + i, noise=6.0 + i), quality=70 + 2 * i, subsampling=2, progressive=True, optimize=bool(i & 1)) for i in range(9)]
    base = [pil_jpeg(picture(w, h, seed=90 + i), quality=85, subsampling=2) for i in range(2)]
    whole = pil_jpeg(picture(w, h, seed=95, noise=12.0), quality=90, subsampling=2, progressive=True)
    cut = whole[:len(whole) * 2 // 3]
    assert whole.index(b"\xff\xda") + 14 < len(cut)          # truncated inside its scans, not its headers
    files = prog[:2] + [base[0]] + prog[2:5] + [cut] + prog[5:7] + [base[1]] + prog[7:]
    assert len(files) == 12
    with pytest.raises(ValueError) as verdict:
        oracle.jpeg_decode(cut)
    want_cut = -1 if "malformed" in str(verdict.value) else -4
    plain = _check_batch(ctx, files)
    plain_streams = _streams(ctx, files, w, h)
    monkeypatch.setenv("IPX_JPEG_HOST_GROUP", "2")
    grouped = _check_batch(ctx, files)
    assert grouped[1] == [0] * 6 + [want_cut] + [0] * 5
    _same_planes(grouped, plain)
    got, st = _streams(ctx, files, w, h)
    assert st == grouped[1] and (got, st) == plain_streams
    assert all(got[k][6] is None for k in got) and all(got[k][i] for k in got for i in range(12) if i != 6)


@pytest.mark.gpu
def test_decode_without_the_lane_arena(ctx, monkeypatch):
    """IPX_JPEG_LANE_ARENA=0: planes and scratch as stream-ordered allocations, for the decode entry and for the compressed-in leg."""
    w, h = 150, 97
    kws = [{}, {"restart_marker_rows": 1}, {"optimize": True}, {"progressive": True}, {"restart_marker_blocks": 5}, {"progressive": True, "optimize": True}]
    files = [pil_jpeg(picture(w, h, seed=100 + i, noise=5.0 + 2 * i), subsampling=2, **{"quality": 85, **kw}) for i, kw in enumerate(kws)]
    plain = _check_batch(ctx, files)
    plain_streams = _streams(ctx, files, w, h)
    monkeypatch.setenv("IPX_JPEG_LANE_ARENA", "0")
    direct = _check_batch(ctx, files)
    assert direct[1] == [0] * 6
    _same_planes(direct, plain)
    assert _streams(ctx, files, w, h) == plain_streams
    assert plain_streams[1] == [0] * 6


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", ["0", "1"])
def test_parallel_images_that_do_not_settle_go_to_the_bytewise_kernel(ctx, rounds, monkeypatch):
    """IPX_JPEG_PAR_ROUNDS=0 (and 1): the parallel passes are cut short, and the scans they took are handed whole to the byte-wise kernel --
    with per-lane tables here, since one file of the batch carries optimised tables.  A sixth file is short and goes the piece path."""
    w, h = 320, 200
    files = [pil_jpeg(picture(w, h, seed=110 + i, noise=25.0 + 3 * i), quality=92 + i, subsampling=2, optimize=(i == 2)) for i in range(5)]
    for f in files:
        seg = _entropy_segment(f)
        assert len(seg) >= 4096                              # four times the largest sub-sequence: decoded in parallel inside the scan
        assert not any(seg[k + 1] in range(0xd0, 0xd8) for k in range(len(seg) - 1) if seg[k] == 0xff)     # no RSTn
    small = pil_jpeg(picture(w, h, seed=120, noise=0.0), quality=20, subsampling=2)
    assert len(_entropy_segment(small)) < 4096
    files.insert(3, small)
    plain = _check_batch(ctx, files)
    monkeypatch.setenv("IPX_JPEG_PAR_ROUNDS", rounds)
    cut_short = _check_batch(ctx, files)
    assert cut_short[1] == [0] * 6
    _same_planes(cut_short, plain)
