"""The parallel inflate's model and corpus on the CPU (tests/png_par_model.py, tests/png_par_corpus.py): the model's bytes are zlib's on
every clean stream at three sub-sequence sizes, every damaged twin is a redo, and the corpus reaches each edge it names -- asserted from
the model's token positions and windows; the same for the edge cases at their four sizes, the trailing twins and the files of the one
mixed launch (tests/test_png_par_edges_gpu.py runs them).  Also: the new ABI entry is declared and documented."""
import os
import re
import zlib

import pytest

import deflate_writer as dw
import png_adam7_model as a7m
import png_decode_model as dm
import png_par_corpus as ppc
import png_par_model as pm

CASES = ppc.corpus()
CLEAN = [c for c in CASES if not c.damage]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tagged(tag):
    return [c for c in CLEAN if c.tags[0] == tag]


def test_sizes():
    assert ppc.SUBS[0] == pm.SUB_DEFAULT and pm.SUB_MIN in ppc.SUBS and any(s % 8 for s in ppc.SUBS) and len(ppc.SUBS) >= 3
    assert all(len(c.raw) <= 110000 for c in CLEAN)
    assert len([c for c in CASES if c.damage]) >= 12


@pytest.mark.parametrize("sub", ppc.SUBS)
def test_model_is_zlib_on_clean_streams(sub):
    for c in CLEAN:
        r = ppc.run(c, sub)
        assert not r.redo, (c.name, r.why)
        assert r.data == zlib.decompress(c.stream) == c.raw, c.name
        assert r.lane_tokens + r.uniform_tokens == len(r.tokens), c.name
        assert sum(1 for t in r.tokens if t.kind == "eob") == sum(1 for b in r.blocks if b[0] != "stored"), c.name
        assert all(1 <= w.passes <= pm.LANES for w in r.windows), c.name


def test_token_count_does_not_depend_on_the_size():
    for c in CLEAN:
        assert len({len(ppc.run(c, sub).tokens) for sub in ppc.SUBS}) == 1, c.name


@pytest.mark.parametrize("sub", ppc.SUBS)
def test_damaged_twins_are_redone(sub):
    for c in CASES:
        if c.damage:
            assert ppc.run(c, sub).redo, c.name
            r = a7m.decode(c.data, adam7=True)
            assert r["status"] == dm.INVALID and r["stage"] == "data", (c.name, r["status"], r["why"])


# ---- the edges ----------------------------------------------------------------------------------------------------------------------
def boundaries_in(r, t):
    """the sub-sequence boundaries of its window strictly inside token t"""
    w = r.windows[t.window]
    k = (t.bit - w.first_bit) // w.sub + 1
    b = w.first_bit + k * w.sub
    return [b] if t.bit < b < t.bit + t.nbits else []


@pytest.mark.parametrize("sub", ppc.SUBS)
def test_a_boundary_inside_each_part_of_a_token(sub):
    (c,) = tagged("parts")
    r = ppc.run(c, sub)
    hit = set()
    for t in r.tokens:
        if t.kind != "match" or t.lane < 0 or not all(t.parts):
            continue
        for b in boundaries_in(r, t):
            at, part = b - t.bit, 0
            while at >= t.parts[part]:
                at -= t.parts[part]
                part += 1
            if part > 0 or at > 0:
                hit.add(part)
    assert hit == {0, 1, 2, 3}, hit


def test_eob_at_and_beside_a_boundary():
    seen = set()
    for c in tagged("eob"):
        _, sub, delta = c.tags
        r = ppc.run(c, sub)
        eob = next(t for t in r.tokens if t.kind == "eob")
        assert eob.bit + eob.nbits - (r.blocks[0][1] + 3 * sub) == delta, c.name
        seen.add((sub, delta))
    assert seen == {(s, d) for s in ppc.SUBS for d in (-1, 0, 1)}


def test_short_and_tiny_blocks():
    (c,) = tagged("short")
    r = ppc.run(c, pm.SUB_MIN)
    assert r.tokens[2].bit + r.tokens[2].nbits + 7 - r.blocks[0][1] < pm.SUB_MIN
    (c,) = tagged("tiny")
    r = ppc.run(c, pm.SUB_DEFAULT)
    per_block = {}
    for t in r.tokens:
        per_block[t.block] = per_block.get(t.block, 0) + 1
    assert sum(1 for n in per_block.values() if n == 2) >= 300          # one symbol and the end-of-block


def test_block_kinds_follow_each_other():
    (c,) = tagged("mixed")
    kinds = [b[0] for b in ppc.run(c, pm.SUB_DEFAULT).blocks]
    pairs = set(zip(kinds, kinds[1:]))
    assert ("dynamic", "fixed") in pairs and ("fixed", "dynamic") in pairs
    (c,) = tagged("stored")
    st, _ = dw.stats(c.stream)
    assert st["stored_offsets"] == set(range(8))
    kinds = [k for k, _ in st["blocks"]]
    assert all(kinds[i - 1] != "stored" and kinds[i + 1] != "stored" for i, k in enumerate(kinds) if k == "stored")


@pytest.mark.parametrize("sub", ppc.SUBS)
def test_the_8_bit_code_never_falls_into_step(sub):
    """a pass per lane: on the first window of each of the 8 blocks, whose first tokens sit at the 8 bit offsets"""
    (c,) = tagged("never")
    r = ppc.run(c, sub)
    first = {}
    for i, w in enumerate(r.windows):
        first.setdefault(w.block, w)
    dyn = [first[b] for b, (kind, _) in enumerate(r.blocks) if kind == "dynamic"]
    assert {w.first_bit % 8 for w in dyn} == set(range(8))
    assert all(w.passes == pm.LANES for w in dyn), [w.passes for w in dyn]
    assert r.uniform_tokens == 0 and all(t.kind != "match" for t in r.tokens)


def test_the_8_bit_code_with_literal_255_falls_into_step_late():
    (c,) = tagged("late")
    for sub in ppc.SUBS:
        r = ppc.run(c, sub)
        assert max(w.passes for w in r.windows) >= 3
        assert r.uniform_tokens == 0
    assert any(2 < w.passes < pm.LANES for sub in ppc.SUBS for w in ppc.run(c, sub).windows)


def test_literal_only_streams_never_reach_the_uniform_loop():
    lit_only = [c for c in CLEAN if "literal-only" in c.tags]
    assert len(lit_only) >= 4
    for c in lit_only:
        for sub in ppc.SUBS:
            r = ppc.run(c, sub)
            assert all(t.kind != "match" for t in r.tokens) and r.uniform_tokens == 0, c.name


def test_budget():
    (c,) = tagged("budget-lone")
    r = ppc.run(c, pm.SUB_DEFAULT)
    assert r.uniform_tokens > 0 and any(w.taken == 0 and w.cum[0] > pm.BUDGET for w in r.windows)
    assert all(t.lane == -1 for t in r.tokens[:r.uniform_tokens])
    assert ppc.run(c, pm.SUB_MIN).uniform_tokens == 0                    # 24 matches a lane: the rounds take them
    for c in tagged("budget-edge"):
        target = c.tags[1]
        w = ppc.run(c, pm.SUB_DEFAULT).windows[0]
        assert target in w.cum, c.name
        if target <= pm.BUDGET:
            assert w.nbytes == target and w.taken == w.cum.index(target) + 1
        else:
            assert w.nbytes < pm.BUDGET and w.taken == w.cum.index(target)


@pytest.mark.parametrize("sub", ppc.SUBS)
def test_matches_over_literals_of_the_same_round(sub):
    (c,) = tagged("same-round")
    r = ppc.run(c, sub)
    owner = {}                                                          # output byte of a literal -> (window, lane)
    for t in r.tokens:
        if t.kind == "lit":
            owner[t.out] = (t.window, t.lane)
    plain = overlap = False
    for t in r.tokens:
        if t.kind != "match" or t.lane < 1:
            continue
        src = range(t.out - t.dist, min(t.out, t.out - t.dist + t.length))
        if any(owner.get(p, (None, 99))[0] == t.window and owner[p][1] < t.lane for p in src):
            plain |= t.dist >= t.length
            overlap |= t.dist < t.length
    assert plain and overlap


def test_distance_32768_into_flushed_output():
    (c,) = tagged("far")
    for sub in ppc.SUBS:
        r = ppc.run(c, sub)
        assert any(t.kind == "match" and t.dist == 32768 and t.lane >= 0 and
                   t.out - t.dist + t.length <= r.windows[t.window].out_first // pm.BUDGET * pm.BUDGET and t.window >= 4 for t in r.tokens)


def test_unit_lengths_and_zlib_settings():
    assert {len(c.raw) for c in tagged("unit")} == {k * 16384 + d for k in (1, 2) for d in (-1, 0, 1)}
    assert len(tagged("level")) == 3 and len(tagged("strategy")) == 6 and len(tagged("adam7")) == 1
    for c in tagged("level") + tagged("strategy"):
        assert any(b[0] != "stored" for b in ppc.run(c, pm.SUB_DEFAULT).blocks), c.name
    assert all(len(ppc.run(c, pm.SUB_DEFAULT).windows) >= 10 and len(c.raw) > 4 * pm.BUDGET for c in tagged("level"))      # the ring wraps


# ---- the ring, the match list, chains, the longest token, the redo walk: the cases of EDGE_SUBS ---------------------------------------
EDGE = [c for c in ppc.corpus(edges=True) if c.tags[0] in ppc.EDGE_TAGS]
TWINS = ppc.trailing_twins()
RING = ppc.RING


def edge(tag):
    return [c for c in EDGE if c.tags[0] == tag]


def lane_matches(r):
    return [t for t in r.tokens if t.kind == "match" and t.lane >= 0]


def source(t):
    """the output bytes a match reads that were there before it began"""
    return range(t.out - t.dist, min(t.out, t.out - t.dist + t.length))


def test_edge_sizes_and_cases():
    assert ppc.EDGE_SUBS == (pm.SUB_DEFAULT, pm.SUB_MIN, 254, pm.SUB_MAX) == (256, 48, 254, 1000)
    assert {c.tags[0] for c in EDGE} == set(ppc.EDGE_TAGS) and not set(ppc.EDGE_TAGS) & {c.tags[0] for c in CASES}
    assert all(len(c.raw) <= 110000 and not c.damage and dm.parse(c.data)[1]["h"] == 1 for c in EDGE)
    with_edges = ppc.corpus(edges=True)
    assert [c for c in with_edges if c.tags[0] not in ppc.EDGE_TAGS] == CASES     # the older cases are what they were, in their order


@pytest.mark.parametrize("sub", ppc.EDGE_SUBS)
def test_model_is_zlib_on_the_edge_cases(sub):
    for c in EDGE:
        r = ppc.run(c, sub)
        assert not r.redo, (c.name, r.why)
        assert r.data == zlib.decompress(c.stream) == c.raw, c.name
        assert r.lane_tokens + r.uniform_tokens == len(r.tokens), c.name
        assert sum(1 for t in r.tokens if t.kind == "eob") == sum(1 for b in r.blocks if b[0] != "stored"), c.name


@pytest.mark.parametrize("sub", ppc.EDGE_SUBS)
def test_a_literal_lands_32_kib_ahead_of_a_byte_its_rounds_match_reads(sub):
    """what a 32 KiB ring could not hold: the literal is written before the match is copied"""
    (c,) = edge("alias")
    r = ppc.run(c, sub)
    assert len(c.raw) > 66000 and all(t.kind == "lit" for t in r.tokens[:40000])
    lit_window = {u.out: u.window for u in r.tokens if u.kind == "lit"}
    hit = [t for t in lane_matches(r) if 16384 < t.dist < 32768 and
           any(p + 32768 > t.out and lit_window.get(p + 32768) == t.window for p in source(t))]
    assert len(hit) >= 1, sub
    assert all(16500 <= t.dist <= 32767 for t in lane_matches(r)) and r.uniform_tokens == 0


@pytest.mark.parametrize("sub", ppc.EDGE_SUBS)
def test_byte_65536_is_crossed_every_way(sub):
    seen = set()
    for c in edge("wrap") + edge("alias"):
        r = ppc.run(c, sub)
        for t in lane_matches(r):
            if t.out < RING < t.out + t.length:
                seen.add("dst" if t.dist >= t.length else "overlap")
            if t.dist >= t.length and t.out - t.dist < RING < t.out - t.dist + t.length:
                seen.add("src")
            if t.dist == 32768 and t.out == RING:
                seen.add("far")
        at = {t.out: i for i, t in enumerate(r.tokens) if t.kind == "lit"}
        if RING - 1 in at and RING in at:
            a = b = at[RING]
            w = r.tokens[a].window
            while r.tokens[a - 1].kind == "lit" and r.tokens[a - 1].window == w:
                a -= 1
            while r.tokens[b + 1].kind == "lit" and r.tokens[b + 1].window == w:
                b += 1
            lanes = {t.lane for t in r.tokens[a:b + 1]}
            if r.tokens[a].out < RING - 1 and min(lanes) >= 0 and len({t.lane for t in r.tokens[a:at[RING]]}) > 1 and \
                    len({t.lane for t in r.tokens[at[RING]:b + 1]}) > 1:
                seen.add("literals")                                     # more than one lane on either side
    assert seen == {"dst", "src", "overlap", "far", "literals"}, seen


@pytest.mark.parametrize("sub", ppc.EDGE_SUBS)
def test_a_stored_block_crosses_byte_65536_and_matches_read_both_sides(sub):
    (c,) = edge("wrap-stored")
    r = ppc.run(c, sub)
    (blk, first, n), = [s for s in r.stored if s[1] <= RING - 1 and s[1] + s[2] > RING]
    assert n == 65535 and r.blocks[blk - 1][0] != "stored"
    later = [t for t in lane_matches(r) if t.block > blk and t.dist >= t.length]
    inside = [t for t in later if first <= source(t)[0] and source(t)[-1] < first + n]
    assert any(source(t)[-1] < RING for t in inside) and any(source(t)[0] >= RING for t in inside)
    assert any(source(t)[0] < RING <= source(t)[-1] for t in inside)
    assert r.tokens.index(inside[0]) == next(i for i, t in enumerate(r.tokens) if t.block > blk)       # the block's first token


def test_a_round_fills_the_match_list():
    (c,) = edge("list")
    per = {}
    for sub in ppc.EDGE_SUBS:
        r = ppc.run(c, sub)
        assert r.uniform_tokens == 0 and sum(1 for t in r.tokens if t.kind == "match") >= 12000, sub
        assert all(t.nbits == 2 and (t.length, t.dist) == (3, 1) for t in r.tokens if t.kind == "match")
        n = {}
        for t in lane_matches(r):
            n[t.window] = n.get(t.window, 0) + 1
        per[sub] = max(n.values())
        assert all(r.windows[w].nbytes >= 3 * k for w, k in n.items())
    assert pm.BUDGET // 3 == 5461
    assert per == {254: pm.BUDGET // 3, 256: 5376, 1000: 5000, 48: 64 * 24}, per
    w = next(w for w in ppc.run(c, 254).windows if w.nbytes == 3 * 5461)
    assert w.taken == 43 and w.nbytes == pm.BUDGET - 1


@pytest.mark.parametrize("sub", ppc.EDGE_SUBS)
def test_matches_over_matches_of_the_same_round(sub):
    (c,) = edge("chain")
    r = ppc.run(c, sub)
    writer = {}                                                         # output byte of a match -> the match
    for t in r.tokens:
        if t.kind == "match":
            for p in range(t.out, t.out + t.length):
                writer[p] = t

    def feeders(t):
        """the matches of its window whose bytes it reads"""
        out = []
        for p in source(t):
            s = writer.get(p)
            if s is not None and s.window == t.window and s not in out:
                out.append(s)
        return out

    deep = over = False
    for t in lane_matches(r):
        for s in feeders(t):
            deep |= bool(feeders(s))                                     # t reads s reads another match: three deep
            over |= t.dist < t.length and s.dist < s.length
    assert deep and over
    m = lane_matches(r)
    assert any(a.window == b.window and not set(source(b)) & set(range(a.out, a.out + a.length)) and not feeders(a) and not feeders(b)
               for a, b in zip(m, m[1:]))                                # two that could be copied together


@pytest.mark.parametrize("sub", [pm.SUB_DEFAULT, pm.SUB_MIN])
def test_a_48_bit_token_starts_at_every_bit_of_a_word(sub):
    (c,) = edge("long-token")
    r = ppc.run(c, sub)
    long = [t for t in lane_matches(r) if t.nbits == 48]
    assert all(t.parts == (15, 5, 15, 13) for t in long)
    assert {t.bit % 32 for t in long} == set(range(32))
    firsts = [next(t for t in r.tokens if t.block == b) for b, (kind, _) in enumerate(r.blocks) if kind == "dynamic"]
    assert len(firsts) == 2 and all(t.nbits == 48 for t in firsts) and any(t.bit % 32 for t in firsts)


def test_trailing_twins():
    """in order, with something behind the Adler-32: UNSUPPORTED, which only a walk that got the whole stream right can say"""
    clean = [c for c in ppc.corpus(edges=True) if not c.damage]
    byte = [c for c in TWINS if c.damage == "trailing byte"]
    idat = [c for c in TWINS if c.damage == "trailing idat"]
    assert [c.name.rsplit(" / ", 1)[0] for c in byte] == [c.name for c in clean]
    assert len(idat) == 3 and {c.tags[0] for c in idat} == {"alias", "stored", "adam7"} and any(len(c.raw) > RING for c in idat)
    assert not any(c.name in {d.name for d in CASES} for c in TWINS)      # not among the damaged twins, whose answer is INVALID
    assert all(c.stream[-1] == 0 and zlib.decompress(c.stream[:-1]) == c.raw for c in byte)
    for c in idat:
        sizes, i = [], 8
        while i < len(c.data):
            n = int.from_bytes(c.data[i:i + 4], "big")
            sizes += [n] if c.data[i + 4:i + 8] == b"IDAT" else []
            i += 12 + n
        assert sizes == [len(c.stream) - 4, 4]
        assert ppc.idat_of(c.data) == c.stream and zlib.decompress(c.stream[:-4]) == c.raw
    for c in TWINS:
        r = a7m.decode(c.data, adam7=True, fast=True)
        assert r["status"] == dm.UNSUPPORTED and r["stage"] == "data", (c.name, r["status"], r["why"])
    for c in byte[::9] + idat:                                           # the pure-Python inflater too, on a few
        if len(c.stream) < 40000:
            assert a7m.decode(c.data, adam7=True)["status"] == dm.UNSUPPORTED, c.name


@pytest.mark.parametrize("part", range(4))
def test_the_model_leaves_a_stream_with_a_byte_behind_it(part):
    """at its very end: every token, window and the Adler-32 went through (a quarter of the twins per row)"""
    for c in [c for c in TWINS if c.damage == "trailing byte"][part::4]:
        r = ppc.run(c, pm.SUB_DEFAULT)
        assert r.redo and r.why == "bytes after the Adler-32", (c.name, r.why)


def test_the_model_clamps_the_size():
    (c,) = tagged("parts")
    m = pm.Model(c.stream)

    def split(r):
        return r.lane_tokens, r.uniform_tokens, [(w.first_bit, w.sub, w.taken) for w in r.windows]

    for sub in (0, 47, -3):
        assert split(m.run(sub)) == split(ppc.run(c, pm.SUB_MIN))
    for sub in (1001, 10 ** 6):
        assert split(m.run(sub)) == split(ppc.run(c, pm.SUB_MAX))
    assert split(ppc.run(c, pm.SUB_MIN)) != split(ppc.run(c, 49)) and split(ppc.run(c, pm.SUB_MAX)) != split(ppc.run(c, 999))


def test_one_launch_of_many_paths():
    files = ppc.mixed_launch()
    assert len(files) >= 32 and {len(c.raw) for c in files if c.raw} == {ppc.MIXED_LENGTH}
    assert {(dm.parse(c.data)[1]["w"], dm.parse(c.data)[1]["h"], dm.parse(c.data)[1]["ctype"]) for c in files} == {(ppc.MIXED_LENGTH - 1, 1, 0)}
    clean = [c for c in files if not c.damage]
    assert {c.tags[0] for c in clean} == {"never", "list", "budget-lone", "short", "tiny", "late", "same-round", "chain", "long-token", "budget-edge"}
    assert len([c for c in clean if c.tags[0] == "budget-edge"]) == 3
    assert sum(1 for c in files if c.damage == "trailing byte") >= 3 and sum(1 for c in files if c.damage and c.damage != "trailing byte") >= 3
    assert all(files[i - 1].damage == "" or files[i - 2].damage == "" for i, c in enumerate(files) if c.damage)      # beside their clean files
    runs = {c.tags[0]: ppc.run(c, pm.SUB_DEFAULT) for c in clean if c.tags[0] in ("never", "list", "budget-lone", "short", "tiny")}
    assert max(w.passes for w in runs["never"].windows) == pm.LANES and min(w.passes for w in runs["list"].windows) == 1
    assert runs["budget-lone"].uniform_tokens > 0 and all(runs[t].uniform_tokens == 0 for t in runs if t != "budget-lone")
    assert len(runs["tiny"].blocks) > 400 and len(runs["short"].blocks) == 2
    for c in files:                                                     # the twins by zlib: in order with a byte behind, or not in order
        if c.damage == "trailing byte":
            d = zlib.decompressobj()
            assert d.decompress(c.stream) == c.raw and d.eof and d.unused_data == b"\0", c.name
        elif c.damage:
            with pytest.raises(zlib.error):
                zlib.decompress(c.stream)


# ---- the entry ----------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_and_documented():
    import ctypes as C
    from imageprocessor_amd import _lib
    res, args = _lib.SIGNATURES["ipx_png_decode_counts"]
    assert res is C.c_int and len(args) == 2 and args[1] == C.POINTER(C.c_longlong)
    header = open(os.path.join(ROOT, "include", "ipx.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ipx_png_decode_counts\(ipx_ctx \*ctx, long long counts\[5\]\);", header, re.S)
    assert m, "ipx_png_decode_counts is not declared behind a comment"
    doc = m.group(1)
    for word in ("IPX_PNG_PAR=1", "[0]", "[1]", "[2]", "[3]", "[4]", "redo"):
        assert word in doc, word
    assert header.index("int ipx_png_decode_batch(") < m.start() < header.index("int ipx_plan_run_png_png(")
