"""The corpus of the GPU scan walk (tests/jpeg_prog_writer.py) is valid and the oracle alone decodes all of it: for every script,
oracle.jpeg_decode of the progressive file equals oracle.jpeg_decode of the baseline file that jpeg_writer.scan writes from the same
coefficients, wherever the image has pixels (reconstructProgressiveImage leaves blocks without image pixels alone)."""
import numpy as np
import pytest

import jpeg_prog_writer as pw
import oracle

NAMES = [c[0] for c in pw.corpus()]


def visible(d, frame):
    w, h = frame.w, frame.h
    if len(frame.comps) == 1:
        return [d["y"][:h, :w]]
    h0, v0 = frame.hv[0]
    cw, ch = (w + h0 - 1) // h0, (h + v0 - 1) // v0
    return [d["y"][:h, :w], d["cb"][:ch, :cw], d["cr"][:ch, :cw]]


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_progressive_file_decodes_like_the_baseline_file_of_the_same_coefficients(k):
    name, frame, prog, base = pw.corpus()[k]
    assert prog[:2] == b"\xff\xd8" and b"\xff\xc2" in prog and b"\xff\xc0" in base
    p, b = oracle.jpeg_decode(prog), oracle.jpeg_decode(base)
    assert (p["w"], p["h"], p["ratio"]) == (frame.w, frame.h, b["ratio"])
    for x, y in zip(visible(p, frame), visible(b, frame)):
        np.testing.assert_array_equal(x, y)
    assert np.ptp(p["y"][:frame.h, :frame.w]) > 0 or "16384" in name      # (not a flat picture that any decoder would get right)


def test_corpus_holds_what_its_names_say():
    files = {c[0]: c[2] for c in pw.corpus()}
    assert pw.scan_data_has_stuffing(files["stuffed 0xff bytes"])
    big = files["one EOB run of 16384 blocks"]
    # the AC scan: one symbol 0xE0 (run category 14) and fourteen zero bits
    assert big.count(b"\xff\xda") == 2 and len(big) - big.rindex(b"\xff\xda") < 40
    dht = [i for i in range(len(files["table ids 2 and 3"]) - 4) if files["table ids 2 and 3"][i:i + 2] == b"\xff\xc4"]
    assert {files["table ids 2 and 3"][i + 4] for i in dht} == {0x03, 0x12, 0x13}
    same = files["tables redefined under the same id"]
    assert {same[i + 4] for i in range(len(same) - 4) if same[i:i + 2] == b"\xff\xc4" and same[i + 2] == 0} <= {0x00, 0x10}
