"""ipx_jpeg_scan_route: which decoder a JPEG file's scans reach (host only, no device).  IPX_JPEG_PROG_GPU=1 sends a progressive file
whose marker pre-pass is wholly clean to the GPU scan walk; unset, or any other value, and for every other file, nothing changes."""
import numpy as np
import pytest

import imageprocessor_amd as ipx
import jpeg_prog_writer as pw
import jpeg_writer as jw
from test_jpeg_decode import picture, pil_jpeg

PAR, HOST, GPU = 0, 1, 2


def route(f):
    return ipx.Context.jpeg_scan_route(f)


@pytest.fixture(scope="module")
def files():
    img = picture(64, 48, seed=3)
    frame = pw.colour_frame(48, 40)
    blocks = jw.all_blocks(frame, np.random.default_rng(1))
    dct, act = jw.Huff(jw.spread(16, 2, 9), list(range(16))), jw.Huff(jw.spread(256, 3, 12), sorted(range(256), key=lambda s: (s & 15, s >> 4)))
    seq = jw.soi() + jw.app0_jfif() + jw.dqt([(0, [2] * 64, 0), (1, [3] * 64, 0)]) + jw.sof(48, 40, frame.comps) + jw.dht([(0, 0, dct), (1, 0, act)])
    for c in range(3):
        seq += jw.sos(frame.comps, [(c, 0, 0)]) + jw.scan(frame, [(c, 0, 0)], blocks, ({0: dct}, {0: act}))
    seq += jw.eoi()
    script = [([0, 1, 2], 0, 0, 0, 0)] + [([c], 1, 63, 0, 0) for c in range(3)]
    prog = pw.progressive(frame, blocks, script)
    undefined = bytearray(pw.progressive(frame, blocks, script, ids="same"))
    sos = undefined.rindex(b"\xff\xda")              # the last scan decodes with AC table 0; name table 2, which no DHT defined
    assert undefined[sos + 6] == 0x00
    undefined[sos + 6] = 0x02
    return {"baseline": pil_jpeg(img, quality=85), "progressive": pil_jpeg(img, quality=85, progressive=True),
            "writer": prog, "dri": pw.progressive(frame, blocks, script, dri=4), "sequential": seq,
            "scans64": pw.progressive(frame, blocks, [([0, 1, 2], 0, 0, 0, 0)] + [([0], 1, 63, 0, 0)] * 63),
            "scans65": pw.progressive(frame, blocks, [([0, 1, 2], 0, 0, 0, 0)] + [([0], 1, 63, 0, 0)] * 64),
            "undefined": bytes(undefined)}


def test_baseline_file_takes_the_parallel_kernels(files, monkeypatch):
    for v in (None, "1"):
        monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False) if v is None else monkeypatch.setenv("IPX_JPEG_PROG_GPU", v)
        assert route(files["baseline"]) == (0, PAR)


@pytest.mark.parametrize("value", [None, "0", "yes", "2", ""])
def test_progressive_file_stays_on_the_host_without_the_switch(files, monkeypatch, value):
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False) if value is None else monkeypatch.setenv("IPX_JPEG_PROG_GPU", value)
    for k in ("progressive", "writer", "scans64"):
        assert route(files[k]) == (0, HOST), k


def test_progressive_file_is_walked_on_the_gpu_with_the_switch(files, monkeypatch):
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    for k in ("progressive", "writer", "scans64"):
        assert route(files[k]) == (0, GPU), k
    for c in pw.corpus():
        assert route(c[2]) == (0, GPU), c[0]


@pytest.mark.parametrize("k", ["dri", "sequential", "scans65", "undefined"])
def test_what_the_pre_pass_does_not_take_stays_on_the_host(files, monkeypatch, k):
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    assert route(files[k]) == (0, HOST)


def test_header_level_errors_keep_the_host_route(files, monkeypatch):
    """a bad SOS header, a missing EOI: the host decoder gives the verdict, as before"""
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    f = bytearray(files["writer"])
    sos = f.rindex(b"\xff\xda")
    f[sos + 7] = 0                                   # Ss = 0 with Se = 63
    assert route(bytes(f)) == (0, HOST)
    assert route(files["writer"][:-2]) == (0, HOST)


def test_truncated_file_has_the_same_status_either_way(files, monkeypatch):
    cuts = [files["progressive"][:n] for n in (1, 3, 20, 150, len(files["progressive"]) // 2)]
    monkeypatch.delenv("IPX_JPEG_PROG_GPU", raising=False)
    off = [route(f) for f in cuts]
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    on = [route(f) for f in cuts]
    assert [s for s, _ in on] == [s for s, _ in off]
    assert off[0][0] == -1 and off[1][0] == -1
    assert all(r != GPU for s, r in on)


def test_unused_table_definitions_cost_the_pre_pass_nothing(monkeypatch):
    """A file may carry any number of DHT segments; only the definitions a scan decodes with are kept (at most three per scan), so
    70 000 unused ones -- more than a 16-bit index holds -- neither change the route nor take long."""
    import time
    monkeypatch.setenv("IPX_JPEG_PROG_GPU", "1")
    frame = pw.colour_frame(48, 40)
    blocks = jw.all_blocks(frame, np.random.default_rng(1))
    f = pw.progressive(frame, blocks, pw.libjpeg_script(frame), extra=pw.unused_tables(70000))
    assert f.count(b"\xff\xc4") >= 20 and len(f) > 70000 * 18
    t0 = time.perf_counter()
    assert route(f) == (0, GPU)
    assert time.perf_counter() - t0 < 2.0            # (the marker walk of 1.3 MB; 70 000 tables in the device format would be 100 MB)
