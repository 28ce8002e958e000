"""The edge corpus of the GPU scan walk (tests/jpeg_prog_edge_corpus.py) is valid, and every case REACHES the edge its name says --
asserted from the file's bytes (staging_facts: offsets against the kernel's 1 KiB chunk grid) or from the blocks and the script it was
written from, without a GPU.  tests/test_jpeg_prog_edges_gpu.py decodes the same files with jpeg_prog_kernel."""
import numpy as np
import pytest

import jpeg_prog_edge_corpus as ec
import jpeg_prog_writer as pw
import oracle
from test_jpeg_prog_writer import visible

CASES = ec.corpus()
NAMES = [c[0] for c in CASES]


def cases(prefix):
    out = [c for c in CASES if c[0].startswith(prefix)]
    assert out, prefix
    return out


def nonzero_per_block(blocks, lo=1, hi=63):
    return [int(np.count_nonzero(b[lo:hi + 1])) for b in blocks[0].reshape(-1, 64)]


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_case_decodes_and_equals_its_baseline_twin(k):
    name, frame, f, facts = CASES[k]
    assert f[:2] == b"\xff\xd8" and b"\xff\xc2" in f and f[-2:] == b"\xff\xd9"
    p = oracle.jpeg_decode(f)
    assert (p["w"], p["h"]) == (frame.w, frame.h)
    assert len(ec.scan_extents(f)) == len(facts["script"])
    if facts["wide"]:
        assert facts["baseline"] is None                 # (a sequential file cannot hold the value either)
        return
    b = oracle.jpeg_decode(facts["baseline"])
    assert p["ratio"] == b["ratio"]
    for x, y in zip(visible(p, frame), visible(b, frame)):
        np.testing.assert_array_equal(x, y)
    assert np.ptp(p["y"][:frame.h, :frame.w]) > 0        # (not a flat picture that any decoder would get right)


def test_scan_extents_agree_with_the_script():
    for name, frame, f, facts in CASES:
        for got, want in zip(ec.scan_extents(f), facts["script"]):
            off, n, ns, ss, se, ah, al = got
            assert (ns, ss, se, ah, al) == (len(want[0]),) + tuple(want[1:5]), name
            assert n > 0 and f[off + n] == 0xFF and f[off + n + 1] != 0x00, name


def test_the_writer_corpus_has_no_straddle():
    """the state this corpus answers: in tests/jpeg_prog_writer.py's 14 files no stuffed zero opens a chunk, so nothing there reads
    `carry`.  Should someone shorten the sweeps below, this says what is lost."""
    assert sum(s["straddles"] for _, _, prog, _ in pw.corpus() for s in ec.staging_facts(prog)) == 0


def test_straddle_sweep_reaches_carry_in_first_scans():
    sweep = cases("straddle sweep")
    assert len(sweep) == 16 and len({c[2] for c in sweep}) == 16
    per_file = [sum(s["straddles"] for s in ec.staging_facts(c[2]) if s["ah"] == 0) for c in sweep]
    print("straddles per file:", per_file)
    assert sum(per_file) >= 8, per_file
    for k in range(4):
        assert {ec.staging_facts(c[2])[k]["start"] for c in sweep} == set(range(16)), k
    assert all(s["len"] > 3 * ec.CHUNK and s["chunks"] >= 4 for c in sweep for s in ec.staging_facts(c[2])[1:])


def test_refinement_sweep_reaches_carry_in_refinement_scans():
    sweep = cases("refinement sweep")
    assert len(sweep) == 16
    last = [ec.staging_facts(c[2])[2] for c in sweep]
    assert all((s["ss"], s["se"], s["ah"], s["al"]) == (1, 63, 1, 0) and s["len"] > 2 * ec.CHUNK for s in last)
    print("straddles per file:", [s["straddles"] for s in last])
    assert sum(s["straddles"] for s in last) >= 4
    assert {s["start"] for s in last} == set(range(16))
    # every correction bit is a one (odd magnitudes) and there are 40 or more per block; every third block takes a new coefficient
    nz = nonzero_per_block(sweep[0][3]["blocks"])
    b = sweep[0][3]["blocks"][0].reshape(-1, 64)
    assert min(nz) >= 40 and np.all(np.abs(b[:, 1:63][b[:, 1:63] != 0]) % 2 == 1) and np.all(np.abs(b[:, 1:63][b[:, 1:63] != 0]) >= 3)
    assert np.count_nonzero(np.abs(b[:, 63]) == 1) == 100


@pytest.mark.parametrize("what, end", [("exactly on a chunk boundary", 0), ("1 byte into a chunk", 1), ("16 bytes into a chunk", 16)])
def test_a_scan_ends_at_a_chunk_edge(what, end):
    (name, frame, f, facts), = cases("a scan ends " + what)
    s = ec.staging_facts(f)[1]
    assert s["end"] == end and s["len"] > ec.CHUNK, s
    assert s["chunks"] == (s["off"] % 16 + s["len"] - end) // ec.CHUNK + (1 if end else 0) >= 2, s
    assert (s["off"] + s["len"] - (s["off"] & ~15)) % ec.CHUNK == end


def test_a_scan_opens_with_a_zero_byte():
    (name, frame, f, facts), = cases("a scan opens with a zero byte")
    s = ec.staging_facts(f)[0]
    assert s["lead_zero"] and f[s["off"]] == 0x00 and (s["ss"], s["ah"]) == (0, 0)
    assert f[s["off"] - 1] != 0xFF                       # the byte before is the SOS header's Ah / Al: the zero is data, never a stuffed one
    assert int(facts["blocks"][0][0, 0, 0]) == 0


def test_correction_counts_per_block():
    want = {"63 and 39 corrections in a block": [63, 39], "25 corrections in a block": [25, 25], "24 corrections in a block": [24, 24],
            "62 corrections in front of a new coefficient": [63, 40],
            "63 corrections under an EOB run pending from the scan before": [63, 39, 0]}
    for name, nz in want.items():
        (_, frame, f, facts), = cases(name)
        b = facts["blocks"][0].reshape(-1, 64)
        assert nonzero_per_block(facts["blocks"]) == nz, name
        assert tuple(facts["script"][-1][1:5]) == (1, 63, 1, 0), name
        big = np.abs(b[:, 1:]) >= 4                      # corrected by the last scan: non-zero before it
        assert [int(r.sum()) for r in big] == [n - (1 if "new" in name else 0) for n in nz], name
        assert len({int(v) & 1 for v in np.abs(b[0, 1:][big[0]])}) == 2, name              # zero and one bits among the corrections
        assert (b[0, 1:] < 0).any() and (b[0, 1:] > 0).any(), name
    (_, _, _, facts), = cases("62 corrections in front of a new coefficient")
    b = facts["blocks"][0].reshape(-1, 64)
    assert abs(int(b[0, 63])) == 1 and abs(int(b[1, 30])) == 1 and np.count_nonzero(b[1, 31:]) >= 1
    (_, _, _, facts), = cases("63 corrections under an EOB run pending")
    assert facts["script"][1][5] == {"overrun": 2}
    (_, _, _, facts), = cases("36 corrections in the band 5 - 40")
    assert nonzero_per_block(facts["blocks"], 5, 40) == [36, 36] and nonzero_per_block(facts["blocks"]) == [63, 63]
    assert tuple(facts["script"][-1][1:5]) == (5, 40, 1, 0)


def test_dc_refinement_group_sizes():
    seen = []
    for name, frame, f, facts in cases("DC refinement"):
        refine = [s for s in facts["script"] if (s[1], s[3]) == (0, 1)]
        n = [len(frame.order([(c, 0, 0) for c in s[0]])) for s in refine]
        seen.append((len(frame.comps), frame.hv[0], n))
        assert ("of %d " % n[0]) in name, (name, n)
        if len(frame.comps) == 3:
            assert len(refine[0][0]) > 1, name           # interleaved
        # the bits vary: both values among the blocks of the scan
        assert {int(v) & 1 for v in facts["blocks"][refine[0][0][0]][..., 0].ravel()} == {0, 1}, name
        # the last block of the scan takes a one: the last lane of the last group (for 33 blocks, the only bit of the second read)
        _, c, by, bx = frame.order([(c, 0, 0) for c in refine[0][0]])[-1]
        assert int(facts["blocks"][c][by, bx, 0]) & 1 == 1, name
    assert sorted(n[0] for c, hv, n in seen if c == 1) == [32, 33, 63, 64, 64, 65, 128]
    assert sorted((hv, n[0]) for c, hv, n in seen if c == 3) == [((2, 1), 64), ((2, 2), 64), ((2, 2), 66)]
    (_, frame, _, _), = cases("DC refinement of 64 blocks (64 x 64)")
    assert frame.grid(0) == (8, 8)                       # the group of 64 wraps seven rows


def test_440_files_are_440():
    for name, frame, f, facts in cases("4:4:0"):
        assert frame.hv[0] == (1, 2) and oracle.jpeg_decode(f)["ratio"] == oracle.RATIO_440, name
    (_, frame, _, _), = cases("4:4:0 17x9")
    assert frame.grid(0) == (2, 3)
    (_, frame, _, _), = cases("4:4:0 9x17")
    assert frame.grid(0) == (4, 2) and (frame.h + 7) // 8 == 3           # the fourth luma block row has no pixel: no luma-only scan codes it
    assert len(frame.order([(0, 0, 0)])) == 6 and len(frame.order([(0, 0, 0), (1, 0, 0), (2, 0, 0)])) == 4 * 4
    (_, frame, _, _), = cases("4:4:0, libjpeg script")
    assert frame.grid(0) == (6, 5) and frame.myy == 3


def test_eob_runs_of_32767():
    (name, frame, f, facts), = cases("EOB runs of 32767")
    assert frame.grid(0) == (181, 182) and 181 * 182 == 32767 + 175
    for k in (1, 2):
        s = ec.staging_facts(f)[k]
        syms = ec.symbols_of(f, k)
        assert 0xE0 in syms and 0x70 in syms and len(syms) == 2, syms       # run categories 14 (16384 + 14 bits) and 7 (128 + 47)
        assert b"\xff\x00" in f[s["off"]:s["off"] + s["len"]]               # the fourteen one bits of 32767 - 16384


def test_wide_cases_leave_int16():
    (_, _, _, facts), = cases("beyond int16: a DC term")
    assert [int(v) for v in facts["blocks"][0][0, :, 0]] == [30000, 60000] and facts["script"][0][4] == 0
    for name, at in (("beyond int16: a correction", [(0, 20), (1, 41)]), ("beyond int16: corrections at positions 63 and 1", [(0, 63), (1, 1)])):
        (_, _, f, facts), = cases(name)
        assert tuple(facts["script"][1][1:5]) == (1, 63, 0, 0) and tuple(facts["script"][2][1:5]) == (1, 63, 2, 1)
        b = facts["blocks"][0][0]
        for i, z in at:
            # 32767 >> 1 is odd: the correction bit is a one, and +-32767 +- 2 is no int16
            assert abs(int(b[i, z])) == 32767 and (32767 >> 1) & 1
        assert int(b[0, 20 if at[0][1] == 20 else 63]) > 0 > int(b[1, at[1][1]])


def test_large_batch_and_mixed_geometry():
    files = ec.large_batch()
    assert len(files) == len(set(files)) == 600
    assert [len(ec.scan_extents(f)) for f in files[:6]] == [2, 3, 6, 2, 3, 6]
    for f in files:
        d = oracle.jpeg_decode(f)
        assert (d["w"], d["h"], d["ratio"]) == (16, 8, 4)
    files, odd = ec.mixed_geometry()
    geo = [(d["w"], d["h"], d["ratio"]) for d in map(oracle.jpeg_decode, files)]
    assert odd == [1, 3] and geo[1][:2] != geo[0][:2] and geo[3][2] != geo[0][2] and geo[3][:2] == geo[0][:2]
    assert all(geo[i] == geo[0] for i in (2, 4))
