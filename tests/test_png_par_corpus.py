"""The parallel inflate's model and corpus on the CPU (tests/png_par_model.py, tests/png_par_corpus.py): the model's bytes are zlib's on
every clean stream at three sub-sequence sizes, every damaged twin is a redo, and the corpus reaches each edge it names -- asserted from
the model's token positions and windows.  Also: the new ABI entry is declared and documented."""
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
