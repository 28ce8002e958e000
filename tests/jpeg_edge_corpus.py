"""JPEG files whose streams use what libjpeg never writes (tests/jpeg_writer.py): 16-bit quantisation tables (with the entries that
make idct.go's int32 arithmetic wrap), AC sizes 11..15 and DC sizes 12..16, Huffman tables with the common symbols on 16-bit codes,
single-symbol, complete and 256-symbol tables, four table ids and several DHT / DQT segments, tables defined after SOF, ZRL runs that
reach or pass zig 63, runs past 63 whose magnitude bits are never read, DRI of 1, odd and longer than the image with RSTn numbers that
wrap, padding with 0s, arbitrary component ids, Adobe / APPn / COM segments and fill bytes, SOF1, and sequential frames split over
several scans in and out of frame order.

corpus(big=False) -> [Case]: each with the file, the coefficients the writer coded (per component, zig-zag order), the edges it carries
and the path the product takes ("gpu": the single-scan kernels, "host": the host scan decoder, then the GPU's IDCT).  big=True adds
1920 x 1080 files whose scans are long enough for the decoder that is parallel inside a scan."""
from dataclasses import dataclass, field

import numpy as np

import jpeg_writer as jw

# the edges the corpus has to keep (test_jpeg_edge_streams.py::test_corpus_covers_every_edge)
HEADER_EDGES = {"dqt16", "tq0", "tq1", "tq2", "tq3", "dqt_after_sof", "dqt_segments", "dht_segments", "four_table_ids", "sof0", "sof1",
                "ids_012", "ids_arbitrary", "jfif", "adobe0", "adobe1", "app_com", "fill_bytes", "dri0", "dri1", "dri_odd",
                "dri_beyond_mcus", "pad0", "pad1", "scans_in_order", "scans_out_of_order", "single_symbol", "complete_table",
                "incomplete_table", "sym256", "common_on_16bit", "idct_wrap"}
SCAN_EDGES = {"zrl_eob", "zrl_to_63", "run_past_63", "dc16_code16", "rst_wrap"} | {("ac_size", s) for s in range(11, 16)} | \
    {("dc_size", t) for t in range(12, 17)} | {("code_len", 16)}


@dataclass
class Case:
    name: str
    data: bytes
    w: int
    h: int
    ratio: int
    coefs: list                  # per component: (rows, cols, 64) zig-zag coefficients as coded
    edges: set = field(default_factory=set)
    path: str = "gpu"


def flat_q(v):
    return [v] * 64


STD_AC = [0x00, 0xF0] + [r << 4 | s for s in range(1, 16) for r in range(16)]        # EOB, ZRL, every run / size: 242 symbols


def tables_short():
    """ordinary tables: short codes for the small sizes, up to 15-bit codes for the rest; DC sizes 0..15 (libjpeg refuses a DC table
    that holds 16), and a second DC table with 16 as well"""
    return jw.huff(jw.spread(16, 2, 16), range(16)), jw.huff(jw.spread(242, 2, 16), STD_AC), jw.huff(jw.spread(17, 2, 16), range(17))


def tables_long():
    """the common symbols last: DC size 0..2, EOB and the small run / size pairs on 16-bit codes"""
    return jw.huff(jw.spread(17, 2, 16), list(range(16, -1, -1))), jw.huff(jw.spread(242, 2, 16), STD_AC[::-1])


def tables_complete():
    """complete tables (the all-ones codes in use, so 0xff bytes and their stuffing are common): DC 16 codes of 4 bits (sizes 0..15),
    AC 14 codes of 7 bits and 228 of 8"""
    ac = [0] * 16
    ac[6], ac[7] = 14, 228
    return jw.huff(jw.complete(4), range(16)), jw.huff(ac, STD_AC)


def tables_256():
    """256 symbols in each class: the DC table spans every byte value (only 0..16 are used), the AC table holds every value -- the
    end-of-band-run symbols included, which sends a sequential file to the host scan decoder"""
    return jw.huff(jw.spread(256, 1, 16), range(256)), jw.huff(jw.spread(256, 1, 16), STD_AC + [r << 4 for r in range(1, 15)])


def limit(blocks, dc_max=2047, ac_max=1023):
    """keeps random blocks within what the given tables can code"""
    for b in blocks:
        np.clip(b[..., 0], -dc_max, dc_max, out=b[..., 0])
        np.clip(b[..., 1:], -ac_max, ac_max, out=b[..., 1:])
    return blocks


def file(w, h, comps, blocks, tables, q, *, sel=None, ri=0, pad=1, marker=0xC0, head=None, after_sof=(), scans=None, tokens=None,
         dht_split=False, dqt_split=False, tail=b"", fill=0):
    """assembles one file: q = {tq: (values, pq)}, tables = {(tc, th): Huff}; scans = a list of sel lists (default one interleaved
    scan over all components with tables 0 / 0, 1 / 1, 1 / 1)"""
    fr = jw.Frame(w, h, comps)
    if sel is None:
        sel = [(c, min(c, 1), min(c, 1)) for c in range(len(comps))]
    scans = scans or [sel]
    head = [jw.app0_jfif()] if head is None else head
    qs = [(tq, v, pq) for tq, (v, pq) in sorted(q.items())]
    hs = [(tc, th, t) for (tc, th), t in sorted(tables.items())]
    dq = [jw.dqt([t]) for t in qs] if dqt_split else [jw.dqt(qs)]
    dh = [jw.dht([t]) for t in hs] if dht_split else [jw.dht(hs)]
    fb = b"\xff" * fill
    out = jw.soi()
    for s in head:
        out += fb + s
    pre = [s for s in dq if "dqt" not in after_sof] + [s for s in dh if "dht" not in after_sof]
    post = [s for s in dq if "dqt" in after_sof] + [s for s in dh if "dht" in after_sof]
    for s in pre:
        out += fb + s
    out += fb + jw.sof(w, h, comps, marker)
    for s in post:
        out += fb + s
    if ri:
        out += fb + jw.dri(ri)
    dcs = {th: t for (tc, th), t in tables.items() if tc == 0}
    acs = {th: t for (tc, th), t in tables.items() if tc == 1}
    for sl in scans:
        out += fb + jw.sos(comps, sl) + jw.scan(fr, sl, blocks, (dcs, acs), ri=ri, pad=pad, tokens=tokens)
    return out + tail + fb + jw.eoi()


RATIO = {(1, 1): 0, (2, 1): 1, (2, 2): 2, (1, 2): 3}


def comps3(h0=2, v0=2, ids=(1, 2, 3), tq=(0, 1, 1)):
    return [(ids[0], h0, v0, tq[0]), (ids[1], 1, 1, tq[1]), (ids[2], 1, 1, tq[2])]


def case(name, w, h, comps, blocks, tables, q, edges, path="gpu", **kw):
    ratio = 4 if len(comps) == 1 else RATIO[comps[0][1], comps[0][2]]
    return Case(name, file(w, h, comps, blocks, tables, q, **kw), w, h, ratio, blocks, set(edges), path)


def _wrap_blocks(fr, rng):
    """blocks for a 16-bit table whose zig 2 entry (natural index 8: the first term of the second row) is 20000: a coefficient of
    53 .. 200 there makes that row's only term 1.06e6 .. 4e6, beyond 2^20, where idct.go's row shortcut (s0 << 3) and its full path
    (s0 << 11 wraps) part ways; some blocks carry 0 or +-1 there"""
    b = [np.zeros(fr.grid(c) + (64,), np.int64) for c in range(len(fr.comps))]
    b[0][..., 0] = rng.integers(-40, 40, fr.grid(0))
    b[0][..., 2] = rng.choice([-1, 0, 1, 1, -1], fr.grid(0)) * rng.choice([1, 53, 120, 200], fr.grid(0))
    return b


def corpus(big=False, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    dc_s, ac_s, dc_s17 = tables_short()
    dc_l, ac_l = tables_long()
    std = {(0, 0): dc_s, (1, 0): ac_s, (0, 1): dc_s, (1, 1): ac_s}
    q8 = {0: (rng.integers(1, 40, 64), 0), 1: (rng.integers(2, 60, 64), 0)}

    # 1. 16-bit DQT: the wrap of idct.go's row pass (a 16 x 16 Gray file, zig 2 entry 20000; the issue's example), and 8-bit
    #    tables reaching the same case (DC 3, -5254 at natural index 8 = zig 2, q 255)
    g1 = [(1, 1, 1, 0)]
    fr = jw.Frame(16, 16, g1)
    qw = np.full(64, 1)
    qw[2] = 20000
    out.append(case("dqt16_wrap_gray", 16, 16, g1, _wrap_blocks(fr, rng), std, {0: (qw, 1)}, {"dqt16", "tq0", "idct_wrap", "sof0", "jfif"}))
    b = [np.zeros((2, 2, 64), np.int64)]
    b[0][..., 0] = 3
    b[0][0, 0, 2] = -5254
    b[0][1, 1, 2] = 5254
    out.append(case("dqt8_wrap_gray", 16, 16, g1, b, std, {0: (np.full(64, 255), 0)}, {"idct_wrap"}))
    for ratio, (h0, v0) in ((2, (2, 2)), (1, (2, 1)), (3, (1, 2)), (0, (1, 1))):
        c3 = comps3(h0, v0, tq=(2, 3, 1))
        fr = jw.Frame(40, 24, c3)
        bl = _wrap_blocks(fr, rng)
        bl[1][..., 0] = rng.integers(-30, 30, fr.grid(1))
        bl[2][..., 1] = rng.integers(-3, 4, fr.grid(2))
        qq = {2: (qw, 1), 3: (rng.integers(200, 65536, 64), 1), 1: (rng.integers(1, 256, 64), 1)}
        out.append(case("dqt16_wrap_%d" % ratio, 40, 24, c3, bl, std, qq, {"dqt16", "tq1", "tq2", "tq3", "idct_wrap"}))

    # 2. large magnitudes: AC sizes 11..15, DC sizes 12..16 (DC alternating so that the value stays in int16), a 16-bit DC code with
    #    16 magnitude bits (the long tables), q 1 so that the IDCT sees them whole
    for name, (dct, act) in (("big_short", (dc_s17, ac_s)), ("big_long", (dc_l, ac_l))):
        c3 = comps3(2, 2)
        fr = jw.Frame(48, 32, c3)
        bl = [np.zeros(fr.grid(c) + (64,), np.int64) for c in range(3)]
        prev = [0, 0, 0]
        for k, (m, c, by, bx) in enumerate(fr.order([(0, 0, 0), (1, 1, 1), (2, 1, 1)])):
            s = 11 + k % 5
            bl[c][by, bx, 1 + k % 63] = ((1 << (s - 1)) + (k * 37) % (1 << (s - 1))) * (1 if k % 2 else -1)
            t = 12 + k % 5                                 # the DC difference's size, towards 0 so that the value stays in int16
            prev[c] += (1 << (t - 1)) * (1 if prev[c] < 0 else -1)
            bl[c][by, bx, 0] = prev[c]
        tabs = {(0, 0): dct, (1, 0): act, (0, 1): dct, (1, 1): act}
        out.append(case(name, 48, 32, c3, bl, tabs, {0: (flat_q(1), 0), 1: (flat_q(2), 0)}, {"common_on_16bit"} if name == "big_long"
                        else {"incomplete_table"}))

    # 3. symbol choices libjpeg never makes: ZRL ZRL EOB, a ZRL that ends on zig 63, a ZRL at 47 then a coefficient on 63, a run that
    #    passes 63 (no magnitude bits follow), EOB right after the DC
    fr = jw.Frame(32, 16, g1)
    bl = [np.zeros((2, 4, 64), np.int64)]
    bl[0][..., 0] = rng.integers(-50, 50, (2, 4))
    toks = {}
    specs = [
        lambda d: [("dc", d), ("ac", 0, 5), ("sym", 0xF0), ("sym", 0xF0), ("sym", 0x00)],
        lambda d: [("dc", d), ("ac", 15, 3), ("ac", 15, -2), ("ac", 14, 7), ("sym", 0xF0)],
        lambda d: [("dc", d), ("sym", 0xF0), ("sym", 0xF0), ("ac", 14, -9), ("ac", 0, 4), ("ac", 14, 6)],
        lambda d: [("dc", d), ("ac", 3, 2), ("ac", 15, 1), ("ac", 15, 1), ("ac", 15, 1), ("sym", 13 << 4 | 1)],
        lambda d: [("dc", d), ("sym", 0x00)],
    ]
    # the coefficients each spec codes (zig-zag position: value)
    expect = [{1: 5}, {16: 3, 32: -2, 47: 7}, {47: -9, 48: 4, 63: 6}, {4: 2, 20: 1, 36: 1, 52: 1}, {}]
    prev = 0
    for k in range(8):
        by, bx = divmod(k, 4)
        j = k % len(specs)
        for pos, v in expect[j].items():
            bl[0][by, bx, pos] = v
        toks[0, by, bx] = specs[j](int(bl[0][by, bx, 0]) - prev)
        prev = int(bl[0][by, bx, 0])
    for pad in (0, 1):
        out.append(case("symbols_pad%d" % pad, 32, 16, g1, bl, std, {0: (flat_q(3), 0)}, {"pad%d" % pad}, tokens=toks))

    # 4. tables: single-symbol (DC always 0, AC only EOB: two bits per block), a single 16-bit code, complete tables, 256 symbols,
    #    four table ids per class in several DHT segments (SOF1: Th 2 / 3 allowed; the product's host path takes ids above 1)
    one = {(0, 0): jw.huff([1] + [0] * 15, [0]), (1, 0): jw.huff([1] + [0] * 15, [0])}
    one16 = {(0, 0): jw.huff([0] * 15 + [1], [0]), (1, 0): jw.huff([0] * 15 + [1], [0])}
    flat = [np.zeros((3, 5, 64), np.int64)]
    for nm, t in (("single_symbol", one), ("single_symbol_16bit", one16)):
        out.append(case(nm, 40, 24, g1, flat, t, {0: (flat_q(7), 0)}, {"single_symbol"}))
    dcc, acc = tables_complete()
    c3 = comps3(1, 1, ids=(0, 1, 2))
    fr = jw.Frame(37, 21, c3)
    out.append(case("complete_tables_444_ids012", 37, 21, c3, limit(jw.all_blocks(fr, rng), 1000, 300),
                    {(0, 0): dcc, (1, 0): acc, (0, 1): dcc, (1, 1): acc}, q8, {"complete_table", "ids_012", "dht_segments", "dqt_segments"},
                    dht_split=True, dqt_split=True))
    d256, a256 = tables_256()
    out.append(case("sym256_host", 37, 21, c3, limit(jw.all_blocks(fr, rng)), {(0, 0): d256, (1, 0): a256, (0, 1): d256, (1, 1): a256}, q8,
                    {"sym256"}, path="host"))
    c3 = comps3(2, 1, ids=(200, 17, 99))
    fr = jw.Frame(50, 19, c3)
    four = {(0, 2): dc_l, (1, 2): ac_s, (0, 3): dc_s, (1, 3): ac_l, (0, 0): dc_s, (1, 0): ac_s}
    out.append(case("four_table_ids_sof1", 50, 19, c3, limit(jw.all_blocks(fr, rng)), four, q8,
                    {"four_table_ids", "sof1", "ids_arbitrary", "dht_segments"}, path="host", marker=0xC1, sel=[(0, 2, 3), (1, 3, 2), (2, 0, 0)],
                    dht_split=True))
    out.append(case("sof1_two_ids", 50, 19, c3, limit(jw.all_blocks(fr, rng)), std, q8, {"sof1", "ids_arbitrary"}, marker=0xC1))

    # 5. segments: tables after SOF, Adobe transform 1 (YCbCr) and 0 (RGB: Go converts, the product hands it back), APPn / COM, fill
    #    bytes before every marker, garbage between segments
    c3 = comps3(2, 2)
    fr = jw.Frame(33, 17, c3)
    bl = limit(jw.all_blocks(fr, rng))
    out.append(case("tables_after_sof", 33, 17, c3, bl, std, q8, {"dqt_after_sof"}, after_sof=("dqt", "dht")))
    out.append(case("adobe1_app_com_fill", 33, 17, c3, bl, std, q8, {"adobe1", "app_com", "fill_bytes"},
                    head=[jw.app14_adobe(1), jw.app(1, b"Exif\x00\x00" + bytes(40)), jw.com(b"a comment"), jw.app(15, b"")], fill=3,
                    tail=b"\x00\x01junk"))
    out.append(case("adobe0_rgb", 33, 17, c3, bl, std, q8, {"adobe0"}, path="unsupported", head=[jw.app14_adobe(0)]))

    # 6. restart intervals: 1, odd, longer than the image, 0 (DRI present, no markers); RSTn wrapping past RST7; intervals in a
    #    Gray file with partial MCUs
    for ri, edges in ((1, {"dri1", "rst_wrap"}), (3, {"dri_odd"}), (7, {"dri_odd"}), (1000, {"dri_beyond_mcus"}), (0, {"dri0"})):
        c3 = comps3(2, 2)
        fr = jw.Frame(70, 37, c3)
        body = case("dri%d" % ri, 70, 37, c3, limit(jw.all_blocks(fr, rng)), std, q8, edges, ri=ri)
        if ri == 0:
            d = bytearray(body.data)
            k = d.index(b"\xff\xda")
            body.data = bytes(d[:k]) + jw.dri(0) + bytes(d[k:])
        out.append(body)
    fr = jw.Frame(23, 45, g1)
    out.append(case("dri5_gray", 23, 45, g1, limit(jw.all_blocks(fr, rng)), std, q8, {"dri_odd"}, ri=5, pad=0))

    # 7. several scans: a sequential frame split into one scan per component, in frame order and out of it, and a two-component
    #    scan; the host scan decoder walks them
    for nm, scans, edges in (("scans_in_order", [[(0, 0, 0)], [(1, 1, 1)], [(2, 1, 1)]], {"scans_in_order"}),
                             ("scans_out_of_order", [[(2, 1, 1)], [(0, 0, 0)], [(1, 1, 1)]], {"scans_out_of_order"}),
                             ("scans_y_then_cbcr", [[(0, 0, 0)], [(2, 1, 1), (1, 1, 1)]], {"scans_out_of_order"})):
        c3 = comps3(2, 2)
        fr = jw.Frame(32, 32, c3)
        out.append(case(nm, 32, 32, c3, limit(jw.all_blocks(fr, rng)), std, q8, edges, path="host", scans=scans))
    c3 = comps3(1, 1)
    fr = jw.Frame(32, 24, c3)
    out.append(case("single_scan_out_of_frame_order", 32, 24, c3, limit(jw.all_blocks(fr, rng)), std, q8, {"scans_out_of_order"},
                    path="host", sel=[(1, 1, 1), (0, 0, 0), (2, 1, 1)]))
    fr = jw.Frame(32, 24, c3)
    out.append(case("multi_scan_16bit_dqt", 32, 24, c3, _wrap_blocks(fr, rng), std, {0: (qw, 1), 1: (flat_q(4), 0)}, {"dqt16", "idct_wrap"},
                    path="host", scans=[[(0, 0, 0)], [(1, 1, 1), (2, 1, 1)]]))

    # 8. sizes: 1 x 1, 8 x 8, MCU-ragged
    for (w, h) in ((1, 1), (8, 8), (17, 9), (15, 31)):
        for c in (g1, comps3(2, 2)):
            fr = jw.Frame(w, h, c)
            out.append(case("size_%dx%d_%d" % (w, h, len(c)), w, h, c, limit(jw.all_blocks(fr, rng)), std, q8, set()))

    if big:
        # 1920 x 1080 4:2:0, scans long enough for the decoder that is parallel inside a scan (tens of kB and more); long codes, big
        # magnitudes and a 16-bit table with the wrap entry
        c3 = comps3(2, 2)
        fr = jw.Frame(1920, 1080, c3)
        for k, (tabs, qq) in enumerate(((std, {0: (qw, 1), 1: (flat_q(3), 0)}),
                                        ({(0, 0): dc_l, (1, 0): ac_l, (0, 1): dc_l, (1, 1): ac_l}, q8))):
            bl = jw.all_blocks(fr, rng, amp=60, ac=3, density=0.05)
            bl[0][::7, ::5, 2] = rng.choice([-1, 1], bl[0][::7, ::5].shape[:2])
            bl[0][::13, ::11, 9] = 20000 * (1 if k else -1)
            out.append(case("big_1080p_%d" % k, 1920, 1080, c3, bl, tabs, qq, set()))
    return out
