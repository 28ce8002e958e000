"""jpeg_prog_kernel (IPX_JPEG_PROG_GPU=1, csrc/ipx_jpeg_dec_scans.hip) at the edges of what it adds to the host decoder: stuffed zeros
that open a staging chunk, scans that end at a chunk's edge, more than 24 corrections in a block, the group sizes of the DC refinement,
4:4:0, EOB runs of 32767, the places a value beyond int16 is flagged, 600 files in one launch and a batch of several geometries.  The
files are tests/jpeg_prog_edge_corpus.py's; tests/test_jpeg_prog_edge_corpus.py shows without a GPU that each reaches its edge and that
the oracle decodes it.  As in tests/test_jpeg_prog_gpu.py every plane is byte-exact against oracle.jpeg_decode, and
ipx_jpeg_decode_counts shows that the file was walked on the GPU, not handed to the host behind our back."""
import numpy as np
import pytest

import jpeg_prog_edge_corpus as ec
import jpeg_prog_writer as pw
import oracle

pytestmark = pytest.mark.gpu

PAR, HOST, GPU, ENDED = 0, 1, 2, 3
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def ctx():
    import imageprocessor_amd as ipx
    c = ipx.Context()
    yield c
    c.close()


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")


def decode(ctx, files):
    """-> (info, status, how far each count rose)"""
    before = ctx.jpeg_decode_counts()
    info, st = ctx.jpeg_decode_batch(files)
    return info, st, [a - b for a, b in zip(ctx.jpeg_decode_counts(), before)]


def same_planes(info, i, want, what=""):
    for k in ("y", "cb", "cr") if want["ratio"] != 4 else ("y",):
        np.testing.assert_array_equal(info[k][i], want[k], err_msg="%s file %d plane %s" % (what, i, k))


def _groups(wide):
    out = {}
    for name, frame, f, facts in ec.corpus():
        if facts["wide"] == wide:
            out.setdefault(facts["group"], []).append((name, f))
    return out


CLEAN, WIDE = _groups(False), _groups(True)


@pytest.mark.parametrize("group", list(CLEAN))
def test_clean_cases_are_walked_and_equal_the_oracle(ctx, on, group):
    """the files of one group (one geometry: the sixteen of a sweep, the small correction files) as one batch"""
    names, files = zip(*CLEAN[group])
    info, st, rose = decode(ctx, list(files))
    assert st == [0] * len(files), (group, st)
    assert rose == [0, 0, len(files), 0], (group, rose)
    for i, f in enumerate(files):
        same_planes(info, i, oracle.jpeg_decode(f), names[i])


def _neighbour():
    frame = pw.gray_frame(16, 8)
    return pw.progressive(frame, pw._blocks(frame, 70, density=0.3), pw.libjpeg_script(frame))


@pytest.mark.parametrize("group", list(WIDE))
def test_a_value_beyond_int16_ends_the_file_as_the_host_route_does(ctx, monkeypatch, group):
    (name, f), = WIDE[group]
    good = _neighbour()
    oracle.jpeg_decode(f)                                # (Go keeps int32: a valid file)
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False)
    _, st_off = ctx.jpeg_decode_batch([f, good])
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    info, st, rose = decode(ctx, [f, good])
    assert st == st_off == [UNSUPPORTED, 0], (name, st, st_off)
    assert rose == [0, 0, 2, 1], rose                    # both walked, one ended by the walk
    same_planes(info, 1, oracle.jpeg_decode(good), name)


def test_600_files_in_one_launch(ctx, on):
    files = ec.large_batch()
    info, st, rose = decode(ctx, files)
    assert st == [0] * 600
    assert rose == [0, 0, 600, 0], rose
    for i, f in enumerate(files):
        same_planes(info, i, oracle.jpeg_decode(f))


def test_files_of_another_geometry_between_walked_neighbours(ctx, monkeypatch):
    files, odd = ec.mixed_geometry()
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False)
    _, st_off = ctx.jpeg_decode_batch(files)
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    info, st, rose = decode(ctx, files)
    assert st == st_off == [UNSUPPORTED if i in odd else 0 for i in range(len(files))], (st, st_off)
    assert rose == [0, 0, len(files) - len(odd), 0], rose
    for i, f in enumerate(files):
        if i not in odd:
            same_planes(info, i, oracle.jpeg_decode(f))
