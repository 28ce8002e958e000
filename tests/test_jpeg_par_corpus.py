"""tests/jpeg_par_corpus.py holds what it claims -- proven from the bytes of its files, without a GPU: where the 0xff 0x00 pairs lie,
the scans' lengths and the residues of the unstuff pass's output offsets, the decoder state at sub-sequence boundaries (from the
writer's own bit offset of every block), the MCU counts and the running DC values.  tests/jpeg_decode_model.py decodes every file to
the coefficients written, or to the stated verdict.  The seeds' conditions (the rounds a shared-table file needs) are asserted here
and nowhere else, and SpecModel -- the passes of ipx_jpeg_dec_par.hip in plain Python -- is held to the true states."""
import numpy as np
import pytest

import jpeg_decode_model as dm
import jpeg_par_corpus as pc
import jpeg_writer as jw


@pytest.fixture(scope="module")
def corpus():
    return pc.corpus()


@pytest.fixture(scope="module")
def by_name(corpus):
    return {c.name: c for c in corpus}


def scan(c):
    off, n = pc.scan_of(c.data)
    return c.data[off:off + n]


_SOLVED = {}


def solved(c, sub):
    if (c.name, sub) not in _SOLVED:
        m = pc.SpecModel(c, sub)
        _SOLVED[c.name, sub] = (m, m.solve())
    return _SOLVED[c.name, sub]


def test_every_file_is_one_baseline_scan_without_restarts(corpus):
    names = [c.name for c in corpus]
    assert len(set(names)) == len(names)
    for c in corpus:
        off, n = pc.scan_of(c.data)
        head = c.data[:off]
        assert head.count(b"\xff\xda") == 1 and b"\xff\xdd" not in head and b"\xff\xc0" in head and b"\xff\xc2" not in head, c.name
        assert (n >= pc.ROUTE_BYTES) == c.par, (c.name, n)
        assert n < 80 * 1024, (c.name, n)
        if "scan_len" in c.props:
            assert n == c.props["scan_len"], (c.name, n)


def test_trace_writes_what_the_writer_writes(corpus):
    """the bit offsets per block come from a restatement of jpeg_writer.scan: it has to give scan()'s bytes, which are the file's"""
    for c in corpus:
        if c.scan_args is None:
            continue
        body, starts = pc.trace(*c.scan_args)
        assert body == jw.scan(*c.scan_args[:4], tokens=c.scan_args[4]), c.name
        assert scan(c)[:len(body)] == body, c.name
        assert len(starts) == len(c.scan_args[0].order(c.scan_args[1])) + 1 and (starts[-1] + 7) // 8 == len(pc.unstuffed(body)), c.name


def test_the_model_decodes_what_was_written(corpus):
    for c in corpus:
        try:
            m = dm.decode(c.data, want_coefs=True)
        except ValueError as e:
            assert c.status == -1 and str(e).startswith("malformed"), (c.name, e)
            continue
        assert c.status == (-4 if m["dc_wide"] else 0), c.name
        for k, want in enumerate(c.coefs):
            np.testing.assert_array_equal(m["coefs"][k], want, err_msg="%s component %d" % (c.name, k))


# ---- unstuffing --------------------------------------------------------------------------------------------------------------------
def test_pairs_lie_on_sub_sequence_word_and_group_boundaries(by_name):
    s = scan(by_name["unstuff_pairs"])
    pairs = pc.stuffed_pairs(s)
    assert tuple(pairs) == pc.PAIRS_AT and s.count(0xFF) == len(pairs)          # and no other 0xff anywhere
    for sub in pc.SUBS:
        ends = [p for p in pairs if (p + 1) % sub == 0]                         # 0xff the last byte of a sub-sequence, 0x00 the first of the next
        assert ends and (ends[0] + 1) // sub <= 63, sub                         # inside the first wave
        inner = [p for p in pairs if p // sub == (p + 1) // sub]
        assert any(p % 4 == 3 and p % 16 != 15 for p in inner), sub             # astride a 4-byte word
        assert any(p % 16 == 15 for p in inner), sub                            # astride a 16-byte group
    for sub in (128, 256):
        assert 64 * sub - 1 in pairs and 65 * sub - 1 in pairs                  # the zero first in sub-sequence 64 (a wave's first lane), and in 65


def test_dense_scan_shifts_the_output_by_every_residue_and_leaves_empty_sub_sequences(by_name):
    s = scan(by_name["unstuff_dense"])
    u = pc.unstuffed(s)
    zeros = np.array(pc.stuffed_pairs(s)) + 1
    assert len(zeros) > 2500 and len(u) == len(s) - len(zeros)
    for sub in pc.SUBS:
        nsub = -(-len(s) // sub)
        # par_count_kernel counts a pair where its zero lies; the exclusive scan of the counts is what a sub-sequence's output is shifted by
        shift = [int((zeros < t * sub).sum()) for t in range(nsub)]
        assert {(t * sub - shift[t]) % 4 for t in range(nsub)} == {0, 1, 2, 3}, sub
        assert len(s) - len(u) > sub
        assert (nsub - 1) * sub * 8 >= len(u) * 8, sub                          # the last by stuffed length: ustart >= ubits, entry kEnd


def test_scan_lengths_sit_on_the_sub_sequence_sizes_and_the_routing_threshold(corpus, by_name):
    lens = {c.props["scan_len"] for c in corpus if c.name.startswith("len_")}
    assert lens == {4095} | set(pc.LENGTHS)
    for sub in pc.SUBS:
        assert any(all(k * sub + d in lens for d in (-1, 0, 1)) for k in range(1, 200)), sub
    assert {-(-n // 128) for n in lens} >= {63, 64, 65, 128, 129}
    # the routing rule counts the stuffed bytes up to the first marker: 4095 stays with the piece kernels, 4096 and 4097 do not
    trio = [by_name["len_%d" % n] for n in (4095, 4096, 4097)]
    assert [c.par for c in trio] == [False, True, True]
    assert all(0xFF in scan(c) for c in trio)                                    # stuffed lengths: each holds a pair
    for c in trio[1:]:
        np.testing.assert_array_equal(c.coefs[0], trio[0].coefs[0])
        assert c.data != trio[0].data


def test_tails_and_cuts(by_name):
    base = by_name["tail_none"]
    ub = pc.unstuffed(scan(base))
    a = by_name["tail_after_eoi"]
    assert a.data.startswith(base.data) and len(a.data) == len(base.data) + a.props["after_eoi"] and scan(a) == scan(base)
    for name in ("tail_behind_rst", "tail_noise_in_scan"):
        c = by_name[name]
        s = scan(c)
        assert s.startswith(scan(base)) and len(s) >= len(scan(base)) + 1500
        tail = s[6000:]
        assert tail.count(b"\xff\x00") >= 100
        for sub in pc.SUBS:
            assert -(-len(s) // sub) > -(-6000 // sub)                           # sub-sequences behind the last block
    s = scan(by_name["tail_behind_rst"])
    assert s[6000:6002] == b"\xff\xd0" and pc.unstuffed(s) == ub                # the kernels' scan ends at the marker
    assert len(pc.unstuffed(scan(by_name["tail_noise_in_scan"]))) > len(ub) + 1000
    c = by_name["cut_on_ff_no_eoi"]
    assert c.data[-1] == 0xFF and c.data[-2] != 0xFF and b"\xff\xd9" not in c.data[-4:]
    c = by_name["cut_on_ff"]
    assert c.data[-3:] == b"\xff\xff\xd9" and c.data[-4] != 0xFF
    c = by_name["cut_mid_symbol"]
    # the 0xff code of a run-15, size-15 symbol, its stuffed zero, and the first byte of its fifteen magnitude bits
    assert c.data[-2:] == b"\xff\xd9" and c.data[-5:-3] == b"\xff\x00" and c.data[-3] != 0xFF


# ---- synchronisation -----------------------------------------------------------------------------------------------------------------
def token_at(c, bit):
    """(token, its first bit) of the token of the scan that holds unstuffed bit `bit`"""
    starts = pc.block_starts(c)
    fr, sel, blocks, (dcs, acs), tokens = c.scan_args
    k = int(np.searchsorted(starts, bit, side="right")) - 1
    toks = tokens[0, k // pc.COLS, k % pc.COLS]
    p = starts[k]
    for t in toks:
        n = pc.token_bits([t], dcs[0], acs[0])
        if p <= bit < p + n:
            return t, p
        p += n
    raise AssertionError("no token at bit %d" % bit)


def test_boundaries_fall_inside_long_symbols(by_name):
    c = by_name["sync_straddles"]
    dcs, acs = c.tables
    assert dcs[0].code[16][1] == 16 and acs[0].code[0x0F][1] == 16               # both symbols have 16-bit codes
    for at, kind, bit in pc.STRADDLES:
        t, p = token_at(c, at * 8)
        assert t == (pc.AC15 if kind == "ac15" else pc.DC16) and at * 8 - p == bit, (at, t, p)
    code = {(k, b < 16) for _, k, b in pc.STRADDLES}
    assert code == {("ac15", True), ("ac15", False), ("dc16", True), ("dc16", False)}
    for sub in pc.SUBS:
        on = [(at, k, b) for at, k, b in pc.STRADDLES if at % sub == 0]
        assert {(k, b < 16) for _, k, b in on} == code, sub                      # every kind on a boundary of this size
        m, _ = solved(c, sub)
        for at, k, b in on:
            assert m.entry[at // sub][0] == at * 8 - b + (31 if k == "ac15" else 32)   # the lane starts behind the symbol
    # the end of a wave's rows and of its staged window (64 rows + 16 bytes) at 128 and 256
    for sub in (128, 256):
        assert {at for at, _, _ in pc.STRADDLES} >= {64 * sub, 64 * sub + 16}
    # one block over whole 128-byte sub-sequences: no block ends there
    t0 = pc.LONG_BLOCK_AT // 128
    m, _ = solved(c, 128)
    assert m.ends[t0] == 0 and m.entry[t0][2] > 0 and m.exit[t0][2] > 0 and m.entry[t0][1] == 0


def test_symbol_choices_and_surplus_blocks(by_name):
    stats = set()
    dm.decode(by_name["sync_symbols"].data, stats=stats)
    assert {"zrl_eob", "zrl_to_63", "run_past_63"} <= stats
    c = by_name["sync_extra_blocks"]
    coded = len(pc.block_starts(c)) - 1
    assert coded >= pc.NB + 300
    for sub in pc.SUBS:
        m, _ = solved(c, sub)
        first = np.concatenate([[0], np.cumsum(m.ends)])[:-1]
        assert sum(m.ends) == coded and (first >= pc.NB).sum() >= 3, sub          # lanes that start at g >= nblk


STATE_CASES = ["unstuff_pairs", "unstuff_dense", "len_4096", "len_8064", "len_8193", "len_16385", "tail_behind_rst", "tail_noise_in_scan",
               "sync_straddles", "sync_symbols", "sync_extra_blocks", "shared_tables_444", "own_tables_444", "dc_tile_2049_bpm4",
               "dc_tile_1025_bpm6"]


@pytest.mark.parametrize("name", STATE_CASES)
def test_the_restated_passes_end_in_the_true_states(by_name, name):
    """at the fixed point every sub-sequence is entered where the writer put a symbol: inside block number (block ends before it), in
    that block's place in its MCU, with DC expected exactly at the block's first bit"""
    c = by_name[name]
    starts = pc.block_starts(c)
    nb = len(starts) - 1
    for sub in pc.SUBS if not name.startswith("dc_tile") else (256,):
        m, rounds = solved(c, sub)
        assert rounds >= 1 and m.entry[0] == (0, 0, 0)
        first = np.concatenate([[0], np.cumsum(m.ends)])
        for t in range(m.nsub):
            p, blk, z = m.entry[t]
            b = int(first[t])
            if m.entry[t] == pc.END or b >= nb:
                continue                                                          # behind the data, or in a tail no writer coded
            assert starts[b] <= p < starts[b + 1] and blk == b % m.bpm and (z == 0) == (p == starts[b]), (sub, t, m.entry[t], b)
            assert t == 0 or p >= t * sub * 8
        if "noise" not in name:
            assert first[-1] == nb, sub


# ---- the seeds' conditions ---------------------------------------------------------------------------------------------------------------
def test_shared_tables_need_a_round_per_wave(by_name):
    """4:4:4 with one table pair: the block-in-MCU index never falls into step by itself, so most speculative exits are wrong and a
    correction travels one wave per round.  The same blocks with other tables for the chroma components settle in fewer rounds."""
    c, twin = by_name["shared_tables_444"], by_name["own_tables_444"]
    m, rounds = solved(c, 128)
    waves = -(-m.nsub // 64)
    assert waves >= 4 and rounds >= 3
    wrong = sum(a != b for a, b in zip(m.spec_exit, m.exit))
    assert wrong > m.nsub // 2
    # (rounds that change an entry at 128, 256, 512, 1024 bytes: quoted in DESIGN.md section 4.6)
    assert [solved(c, s)[1] for s in pc.SUBS] == [8, 5, 3, 2]
    assert [-(-solved(c, s)[0].nsub // 64) for s in pc.SUBS] == [9, 5, 3, 2]
    mt, rt = solved(twin, 128)
    assert rt < rounds and sum(a != b for a, b in zip(mt.spec_exit, mt.exit)) < wrong


# ---- the DC pass ---------------------------------------------------------------------------------------------------------------------------
def test_mcu_counts_sit_on_the_dc_tiles(corpus):
    seen = set()
    for c in corpus:
        if not c.name.startswith("dc_tile"):
            continue
        fr = c.scan_args[0]
        assert fr.mxx * fr.myy == c.props["nmcu"] and len(fr.order(c.sel)) == c.props["nmcu"] * c.props["bpm"]
        seen.add((c.props["nmcu"], c.props["bpm"]))
    assert seen == {(n, b) for n in (1023, 1024, 1025, 2047, 2048, 2049) for b in (1, 3, 4, 6)}


def test_dc_values_reach_and_pass_int16_beyond_the_first_tile(corpus):
    n = 0
    for c in corpus:
        if "dc_hi" not in c.props:
            continue
        n += 1
        hi, lo = c.props["dc_hi"], c.props["dc_lo"]
        for k, bl in enumerate(c.coefs):
            dc = bl[..., 0].reshape(-1)                                           # Gray / 4:4:4: scan order per component is MCU order
            d = np.diff(np.concatenate([[0], dc]))
            assert d.min() >= -32768 and d.max() <= 32767, c.name                 # every difference fits; only running values go past
            if k in c.props["peaks"]:
                a, b = c.props["peaks"][k]
                assert a >= 1024 and dc[a] == hi == dc.max() and dc[b] == lo == dc.min(), c.name
            else:
                assert abs(dc).max() < 32767
        assert c.status == (0 if (hi, lo) == (32767, -32768) else -4)
    assert n == 6


def test_a_dc_step_beyond_int16_between_values_that_fit():
    c = pc.dc_wide_step_case()
    m = dm.decode(c.data, want_coefs=True)
    assert not m["dc_wide"] and pc.scan_of(c.data)[1] >= pc.ROUTE_BYTES
    np.testing.assert_array_equal(m["coefs"][0], c.coefs[0])
    dc = c.coefs[0][..., 0].reshape(-1)
    assert np.diff(dc).min() == c.props["dc_step"] == -65535 and dc.max() == 32767 and dc.min() == -32768 and int(np.argmin(dc)) > 1024
