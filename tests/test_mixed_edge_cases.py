"""The inputs of the mixed-size edge tests (tests/mixed_edge_cases.py) reach the edges they are there for: asserted here without a GPU,
so that a corpus or a builder that changes under them fails at once instead of leaving a GPU test that passes for nothing."""
import numpy as np

import mixed_edge_cases as mx


def test_overlong_short_and_cut_scans_stand_before_another_shape():
    """A1: in the interleaved order every file whose scan holds more blocks than its frame, ends short or is cut is followed, within
    its sampling class, by a decodable file of another shape; every file of the corpus is in the order once; the classes alternate"""
    cases = mx.par_corpus()
    order = mx.interleaved(cases)
    assert sorted(c.name for c in order) == sorted(c.name for c in cases) and len({c.name for c in cases}) == len(cases)
    bad = [i for i, c in enumerate(order) if mx.overruns(c)]
    names = {order[i].name for i in bad}
    assert {"sync_extra_blocks", "cut_on_ff_no_eoi", "cut_on_ff", "cut_mid_symbol", "tail_behind_rst", "tail_noise_in_scan"} <= names
    assert any(order[i].props.get("extra_blocks", 0) >= 300 for i in bad)
    for i in bad:
        nxt = mx.behind_in_class(order, i)
        assert nxt is not None and nxt.status == 0 and (nxt.w, nxt.h) != (order[i].w, order[i].h), order[i].name
    assert len({c.ratio for c in order[:4]}) == 4                    # four classes in the first four files
    assert [c.name for c in order] != [c.name for c in cases]


def test_one_class_holds_a_sixteenfold_spread_of_scan_lengths():
    """A1: a.ends[blockIdx.y * a.max_nsub + t] with rows of very unequal use.  Measured: Gray 4096 .. 159 442 bytes (38 x; the corpus's
    own Gray files end at 29 320, 7 x, hence the Pillow file behind them), 4:4:4 32 985 .. 81 525, 4:2:2 36 972 .. 51 150, 4:2:0
    44 143 .. 64 674"""
    spread = mx.scan_spread(mx.par_corpus())
    print(spread)
    assert len(spread) == 4
    lo, hi = spread[4]
    assert lo == 4096 and hi >= 16 * lo


def test_host_groups_are_unequal():
    """A4: at IPX_JPEG_HOST_GROUP=2 the groups stage different numbers of words and the largest is not the first (a half sized by the
    first group is too small); at 1 the same; at 16 there is one group"""
    files, host = mx.host_route_files()
    assert len(files) == 7 and len(host) == 5
    for group in (1, 2):
        words = mx.host_group_words(mx.HOST_SIZES, group)
        assert len(set(words)) == len(words) and max(words) != words[0], (group, words)
        assert len(words) > 1 and words[0] != words[1]
    assert len(mx.host_group_words(mx.HOST_SIZES, 16)) == 1
    # reversed: the groups are other groups, and again unequal
    rev = mx.host_group_words(mx.HOST_SIZES[::-1], 2)
    assert len(set(rev)) == 3 and rev != mx.host_group_words(mx.HOST_SIZES, 2)[::-1]
    # the files are progressive, of the sizes given, in one class
    from test_jpeg_mixed_gpu import oracle_of
    for k, i in enumerate(host):
        assert b"\xff\xc2" in files[i]
        d = oracle_of(files[i])
        assert (d["y"].shape[1], d["ratio"]) == ((mx.HOST_SIZES[k][0] + 15) // 16 * 16, 2)
    assert all(b"\xff\xc2" not in files[i] for i in (2, 5))


def test_the_edge_corpus_is_mixed_with_a_twin_per_class():
    mix = mx.edge_mix()
    names = [n for n, _ in mix]
    assert len(mix) == 38 + 5 and sum(n.startswith("twin_") for n in names) == 5
    assert not names[0].startswith("twin_") and sum(names[i].startswith("twin_") for i in range(len(names) - 3)) >= 4


def test_leg_cases():
    files, sizes = mx.leg_classes_case()
    assert len(files) == 20 and len(set(sizes)) == 10 and sum(b"\xff\xc2" in f for f in files) == 10
    assert all(len({(b"\xff\xc2" in f) for f, s in zip(files, sizes) if s == key}) == 2 for key in set(sizes))
    # B2: the damaged files are the first, the last, or all but one of the run in the leg's order, which is the call's order there
    for variant, ks in mx.RUN_VARIANTS.items():
        files, sizes, bad, run = mx.run_ends_case(variant)
        order = sorted(range(len(files)), key=lambda i: (sizes[i][0], sizes[i][1], i))
        assert order[2:6] == run and [run.index(i) for i in bad] == list(ks)
        assert sizes[order[0]] != mx.RUN_SIZE and sizes[order[-1]] != mx.RUN_SIZE
        assert [i for i in range(8) if b"\xff\x00" * 4 in files[i]] == bad
    assert mx.RUN_VARIANTS == {"first": (0,), "last": (3,), "all-but-one": (0, 1, 3)}
    # B4: the wide file first, in the middle and last of the sorted chunk, at another place in the call
    for where, pos in (("first", 0), ("middle", 2), ("last", 4)):
        files, sizes, at = mx.empty_output_case(where)
        assert sizes[at][:2] == mx.EMPTY_SIZE and mx.sorted_position(sizes, at) == pos != at
        # 600 x 1 kept in aspect inside 64 x 48: 64 wide and 48 * 1 / 600 = 0 rows; the neighbours all come out 64 x 48
        assert 64 * 1 // 600 == 0 and all(w * 3 == h * 4 for w, h, _ in sizes if (w, h) != mx.EMPTY_SIZE)


def test_filter_rows_go_beyond_one_grid_row():
    """C1: more than 2^20 rows, a frame whose rows straddle 2^20, a total that is no multiple of 2^20"""
    heights = mx.grid_heights()
    row0, rows = mx.row0s(heights)
    assert rows > mx.GRID_X and rows % mx.GRID_X != 0
    assert any(r < mx.GRID_X <= r + h - 1 for r, h in zip(row0, heights))
    assert row0[-1] > mx.GRID_X and heights[-1] == 1                  # and a frame whose row0 the search finds beyond 2^20
    assert -(-rows // mx.GRID_X) == 2
    opaque, alpha = mx.tall_frames()
    assert opaque.shape == alpha.shape == (65535, 1, 4) and opaque.nbytes == 262140
    assert (opaque[..., 3] == 255).all() and np.argwhere(alpha[..., 3] != 255).tolist() == [[65534, 0]]
    assert (alpha[..., :3] <= alpha[..., 3:]).all()                  # premultiplied


def test_the_big_frame_is_beyond_the_opacity_cap():
    """C2: 2048 x 1025 asks for 513 workgroups of 4096 pixels, the cap is 512"""
    assert mx.opacity_blocks(*mx.BIG) == 513 > mx.OPACITY_WGS
    assert mx.opacity_blocks(2048, 1024) == 512
    n = mx.BIG[0] * mx.BIG[1]
    # pixel 512 * 256 belongs to workgroup 0's second round; in a sweep 513 workgroups wide it would be workgroup 512's, which the
    # capped grid does not have (the last pixel would be workgroup 505's there: it alone does not tell the two strides apart)
    assert mx.SECOND_SWEEP // 256 % 512 == 0 and mx.SECOND_SWEEP // 256 % 513 == 512 and (n - 1) // 256 % 513 < 512
    for at in (0, mx.SECOND_SWEEP, n - 1):
        f = mx.big_frame(at)
        assert f.nbytes == 8396800 and np.flatnonzero(f[..., 3].reshape(-1) != 255).tolist() == [at]
        assert (f[..., :3] <= f[..., 3:]).all()
    # the last pixel is reached in the stride loop's last round only: beyond 512 * 4096 pixels
    assert n - 1 >= mx.OPACITY_WGS * 4096


def test_png_decode_inputs():
    """D2: nothing of the parallel inflate's corpus is left out -- the two frames of png_edge_corpus.large() are not part of it -- and
    the cap is those two; five small files of other kinds, two paletted, stand between its files.  D3: three sizes."""
    import png_decode_model as dm
    files, left_out = mx.png_par_mix()
    assert len(left_out) <= 2 and left_out == []
    small = [(n, d) for n, d, c in files if c is None]
    assert len(small) == 5
    kinds = [dm.decode(d, fast=True)["kind"] for _, d in small]
    assert kinds.count(dm.PALETTED) == 2 and len(set(kinds)) == 4
    at = [i for i, (_, _, c) in enumerate(files) if c is None]
    assert at[0] > 0 and all(b - a > 1 for a, b in zip(at, at[1:]))
    pairs = mx.adam7_pairs()
    assert len(pairs) == 3
    for il, twin in pairs:
        assert dm.decode(il)["status"] == dm.UNSUPPORTED and dm.decode(twin, fast=True)["status"] == dm.OK
