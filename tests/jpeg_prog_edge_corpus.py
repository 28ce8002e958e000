"""Progressive JPEGs at the edges of the GPU scan walk's own machinery (csrc/ipx_jpeg_dec_scans.hip), built on tests/jpeg_prog_writer.py.

tests/jpeg_prog_writer.py's corpus pins the arithmetic of Go's processSOS / refine / refineNonZeroes.  What jpeg_prog_kernel adds to
the host decoder is reached there by accident at best: the unstuffing while staging (a stuffed 0x00 that OPENS a 1 KiB chunk is dropped
through `carry`, the last raw byte of the chunk before), the chunking itself (a scan that ends on a chunk boundary, or a few bytes
behind one), the correction loop of refine_nonzeroes that hands out 24 bits per turn, the DC refinement that takes 64 blocks per turn
as two reads of up to 32 bits, the 4:4:0 block order, the three places a value beyond int16 is flagged, an EOB run of 32767, and a
batch of more files than the card runs waves at once.

The reach helpers restate what the marker pre-pass (prescan in csrc/ipx_jpeg_dec_prog.cpp) and stage() do with OFFSETS, so that a
test can say from the file alone that a case reaches its edge.  They restate nothing of the decoding:

  scan_extents(file)     [(off, len, ns, ss, se, ah, al)]: the readable bytes of every scan, cut at the first 0xff that 0x00 does not follow
  staging_facts(file)    per scan a dict: where the chunk boundaries (off & ~15) + 1024 k fall in it (see there)
  corpus()               [(name, frame, file, facts)]; facts: "group" (files of one group share a geometry and are decoded as ONE
                         batch), "blocks" and "script" as written, "baseline" (the baseline file of the same coefficients, or None),
                         "wide" (True: a coefficient leaves int16 -- Go decodes it, the pipeline answers UNSUPPORTED)
  large_batch()          600 small files with 2, 3 or 6 scans in rotation
  mixed_geometry()       (files, the indices of those whose geometry is not the first file's)

numpy only; a helper of the tests."""
import functools

import numpy as np

import jpeg_prog_writer as pw
import jpeg_writer as jw

CHUNK = 1024        # kChunk of the kernel: raw bytes staged per turn


# ---- reach helpers -------------------------------------------------------------------------------------------------------------------
def scan_extents(f):
    """[(off, len, ns, ss, se, ah, al)] of every SOS of the file: `off` is the first entropy-coded byte, `len` runs up to the first 0xff
    that 0x00 does not follow (or the end of the file), as prescan cuts it"""
    out = []
    i = 2
    while i + 4 <= len(f):
        assert f[i] == 0xFF, "a marker was expected at %d" % i
        m = f[i + 1]
        if m == 0xFF:                                   # a fill byte
            i += 1
            continue
        if m == 0xD9:
            break
        n = f[i + 2] << 8 | f[i + 3]
        if m != 0xDA:
            i += 2 + n
            continue
        ns = f[i + 4]
        ss, se, a = f[i + 5 + 2 * ns:i + 8 + 2 * ns]
        off = end = i + 2 + n
        while True:
            end = f.find(b"\xff", end)
            if end < 0:
                end = len(f)
                break
            if end + 1 >= len(f) or f[end + 1] != 0:
                break
            end += 2
        out.append((off, end - off, ns, ss, se, a >> 4, a & 15))
        i = end
        while i + 1 < len(f) and (f[i] != 0xFF or f[i + 1] in (0x00, 0xFF) or 0xD0 <= f[i + 1] <= 0xD7):     # the marker loop's skip
            i += 1
    return out


def staging_facts(f):
    """per scan of the file, what stage() meets.  The kernel stages a scan from rpos = off & ~15 in chunks of 1024 raw bytes, so the
    chunk boundaries lie at g = (off & ~15) + 1024 k, k >= 1:

      "straddles"   the boundaries g inside the scan with file[g - 1] == 0xff and file[g] == 0x00 (g - 1 >= off): the stuffed zero
                    opens a chunk, and only `carry` says that it is one
      "start"       off % 16: where in lane 0's sixteen bytes the scan begins
      "chunks"      the chunks the scan's bytes touch
      "end"         (off + len - (off & ~15)) % 1024: how far into a chunk the scan ends.  0: it ends exactly on a boundary (the last
                    chunk is full); 1: one byte into a new chunk; 16: lane 0 of the last chunk is full and lane 1 gets nothing
      "lead_zero"   the scan's first byte is 0x00
    plus the scan's own "off", "len", "ns", "ss", "se", "ah", "al" """
    out = []
    for off, n, ns, ss, se, ah, al in scan_extents(f):
        base = off & ~15
        bounds = range(base + CHUNK, off + n, CHUNK)
        out.append({"off": off, "len": n, "ns": ns, "ss": ss, "se": se, "ah": ah, "al": al,
                    "straddles": sum(1 for g in bounds if g - 1 >= off and f[g - 1] == 0xFF and f[g] == 0x00),
                    "start": off % 16, "chunks": (off + n - base + CHUNK - 1) // CHUNK, "end": (off + n - base) % CHUNK,
                    "lead_zero": n > 0 and f[off] == 0x00})
    return out


def pad_segment(n):
    """a COM segment with n bytes of text: everything behind it moves by 4 + n bytes"""
    return jw.seg(0xFE, b"x" * n)


def _padded(frame, blocks, script, pads):
    """the file with a COM pad of each length behind the frame header.  Nothing else of the file depends on the pad, so it is written
    once and the segment exchanged"""
    f = pw.progressive(frame, blocks, script, extra=pad_segment(0))
    at = f.index(pad_segment(0))
    assert at < f.index(b"\xff\xda") and f.count(b"\xff\xfe") == 1
    return [f[:at] + pad_segment(p) + f[at + 4:] for p in pads]


def symbols_of(f, k):
    """the HUFFVAL bytes of the DHT segment in front of the file's k-th scan"""
    dht = f.rindex(b"\xff\xc4", 0, scan_extents(f)[k][0])
    n = f[dht + 2] << 8 | f[dht + 3]
    return bytes(f[dht + 4 + 17:dht + 2 + n])


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _empty(frame, seed, amp=200):
    return pw._blocks(frame, seed, amp=amp, density=0.0)


def _signed(rng, shape, lo, hi):
    """magnitudes lo .. hi with random signs"""
    return rng.integers(lo, hi + 1, shape) * rng.choice([-1, 1], shape)


def straddle_sweep():
    """160 x 120 4:4:4, magnitudes of all ones as in the writer's "stuffed 0xff bytes" case, one band scan of 1 - 63 per component: about
    3.6 KB per band scan, most bytes 0xff 0x00 pairs that huff() and receive_extend() read across; 16 COM pads move the scans byte by
    byte against the chunk grid, through every start residue"""
    frame = pw.colour_frame(160, 120)
    blocks = _empty(frame, 31)
    for b in blocks:
        b[..., 0] = 255
        b[..., 1:9] = 255
    script = [(pw._all(frame), 0, 0, 0, 0)] + pw._per_component(frame, [(1, 63, 0, 0)])
    return frame, blocks, script, _padded(frame, blocks, script, range(16))


def refinement_sweep():
    """grey 160 x 120, 300 blocks: every block has 40 to 62 coefficients that the last scan corrects with a one bit (odd magnitudes),
    and every third block a new coefficient behind them -- so the refinement scan is about 3.5 KB of mostly 0xff 0x00, read by the
    bits(k) of refine_nonzeroes, through the symbol path (zig, run) and under EOB runs (zig, -1) alike"""
    frame = pw.gray_frame(160, 120)
    rng = np.random.default_rng(32)
    blocks = _empty(frame, 32)
    b = blocks[0]
    rows, cols = b.shape[:2]
    for by in range(rows):
        for bx in range(cols):
            n = int(rng.integers(40, 63))
            b[by, bx, 1:1 + n] = (2 * rng.integers(1, 4, n) + 1) * rng.choice([-1, 1], n)        # 3, 5, 7: odd, corrected by a one
            if (by * cols + bx) % 3 == 0:
                b[by, bx, 63] = 1 if bx & 1 else -1
    script = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1), ([0], 1, 63, 1, 0, {"max_eobrun": 5})]
    return frame, blocks, script, _padded(frame, blocks, script, range(16))


def _end_search():
    """files whose band scan ends 0, 1 and 16 bytes into a chunk.  Where a scan ends against the chunk grid is (off % 16 + len) % 1024,
    so a pad reaches sixteen neighbouring values and the scan's length has to do the rest: the tail of the frame is emptied block by
    block (a block is a few bytes), and for every length the sixteen pads are tried.  -> {end: (blocks, pad, file)}"""
    frame = pw.gray_frame(160, 120)
    full = pw._blocks(frame, 33, density=0.1)
    script = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)]
    rows, cols = full[0].shape[:2]
    found = {}
    for keep in range(rows * cols, 0, -1):
        blocks = [full[0].copy()]
        blocks[0].reshape(-1, 64)[keep:, 1:] = 0
        probe = pw.progressive(frame, blocks, script, extra=pad_segment(0))
        off, n = scan_extents(probe)[1][:2]
        if n <= CHUNK + 16:
            break
        for want in (0, 1, 16):
            r = (want - n) % CHUNK                       # the start residue off % 16 that would do it
            if want not in found and r < 16:
                pad = (r - off) % 16                     # a pad moves off by one byte
                found[want] = (blocks, pad, pw.progressive(frame, blocks, script, extra=pad_segment(pad)))
        if len(found) == 3:
            break
    assert len(found) == 3, sorted(found)
    return frame, script, found


def _corrections(counts, seed, new_at=None, lo=4):
    """16 x 8 grey (or wider): block i has counts[i] non-zero AC coefficients of magnitude >= lo at random positions, mixed signs, random
    low bits; new_at: {block: position} of a coefficient of magnitude 1 (new in the last scan) -- the position is kept free"""
    frame = pw.gray_frame(8 * len(counts), 8)
    rng = np.random.default_rng(seed)
    blocks = _empty(frame, seed)
    for i, n in enumerate(counts):
        free = [z for z in range(1, 64) if not new_at or new_at.get(i) != z]
        at = np.sort(rng.choice(free, n, replace=False)) if n < len(free) else np.array(free)
        blocks[0][0, i, at] = _signed(rng, len(at), lo, 40)
        if new_at and i in new_at:
            blocks[0][0, i, new_at[i]] = -1 if i & 1 else 1
    return frame, blocks


def _dc_refinement(frame, seed):
    """random DC terms, so that the refinement bits vary; the LAST block of the scan (the last lane of its last group) takes a one"""
    blocks = pw._blocks(frame, seed, amp=1000, density=0.1)
    blocks[-1][-1, -1, 0] |= 1
    n = len(frame.comps)
    if n == 1:
        return blocks, [([0], 0, 0, 0, 1), ([0], 0, 0, 1, 0), ([0], 1, 63, 0, 0)]
    return blocks, [(pw._all(frame), 0, 0, 0, 1), (pw._all(frame), 0, 0, 1, 0)] + pw._per_component(frame, [(1, 63, 0, 0)])


def _wide(at):
    """two grey blocks, a first pass at Al = 0 that holds +-32767, then a refinement of Ah = 2, Al = 1 over it (Go only checks
    Ah == Al + 1): the correction adds 2 and the value leaves int16.  at: [(block, zig-zag position, value)]"""
    frame = pw.gray_frame(16, 8)
    blocks = _empty(frame, 39)
    blocks[0][0, :, 5] = (6, -13)                         # 6 is corrected too (6 >> 1 is odd) and stays an int16; -13 takes a zero bit
    for i, z, v in at:
        blocks[0][0, i, z] = v
    return frame, blocks, [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0), ([0], 1, 63, 2, 1)]


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, frame, file, facts)]"""
    out = []

    def case(name, frame, blocks, script, group=None, file=None, wide=False, **kw):
        f = file if file is not None else pw.progressive(frame, blocks, script, **kw)
        base = None if wide else pw.baseline(frame, blocks)
        out.append((name, frame, f, {"group": group or name, "blocks": blocks, "script": script, "baseline": base, "wide": wide}))

    frame, blocks, script, files = straddle_sweep()
    for p, f in enumerate(files):
        case("straddle sweep, pad %d" % p, frame, blocks, script, group="straddle sweep", file=f)
    frame, blocks, script, files = refinement_sweep()
    for p, f in enumerate(files):
        case("refinement sweep, pad %d" % p, frame, blocks, script, group="refinement sweep", file=f)
    frame, script, found = _end_search()
    for want, what in ((0, "exactly on a chunk boundary"), (1, "1 byte into a chunk"), (16, "16 bytes into a chunk")):
        case("a scan ends " + what, frame, found[want][0], script, group="scan ends", file=found[want][2])

    # the most frequent DC symbol is size 0 and its code is one zero bit: nine blocks of difference 0 open the scan with 0x00
    fz = pw.gray_frame(128, 8)
    bz = pw._blocks(fz, 34)
    bz[0][0, :, 0] = [0] * 9 + [5, -3, 100, 7, 7, -20, 0]
    case("a scan opens with a zero byte", fz, bz, [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)])

    last = [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1), ([0], 1, 63, 1, 0)]
    f2, b2 = _corrections([63, 39], 35)
    case("63 and 39 corrections in a block", f2, b2, last, group="corrections")
    f2, b2 = _corrections([25, 25], 36)
    case("25 corrections in a block", f2, b2, last, group="corrections")
    f2, b2 = _corrections([24, 24], 37)
    case("24 corrections in a block", f2, b2, last, group="corrections")
    # the corrections in front of a NEW coefficient: refine_nonzeroes(zig, run) of the symbol path, 62 bits in block 0; block 1 has
    # 20 of its 39 behind the new coefficient, which the EOB that follows corrects
    f2, b2 = _corrections([62, 39], 38, new_at={0: 63, 1: 30})
    case("62 corrections in front of a new coefficient", f2, b2, last, group="corrections")
    # the first pass leaves a run of three pending over a frame of three blocks of which only the last is empty: the refinement scan
    # starts inside that run, and the blocks of 63 and 39 are corrected without a symbol being read
    f3, b3 = _corrections([63, 39, 0], 40)
    case("63 corrections under an EOB run pending from the scan before", f3, b3,
         [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1, {"overrun": 2}), ([0], 1, 63, 1, 0)])
    f2, b2 = _corrections([63, 63], 41)
    case("36 corrections in the band 5 - 40 of a full block", f2, b2,
         [([0], 0, 0, 0, 0), ([0], 1, 4, 0, 0), ([0], 5, 40, 0, 1), ([0], 41, 63, 0, 0), ([0], 5, 40, 1, 0)], group="corrections")

    for w, h in ((256, 8), (264, 8), (504, 8), (512, 8), (520, 8), (1024, 8), (64, 64)):
        fd = pw.gray_frame(w, h)
        bd, sd = _dc_refinement(fd, 42 + w + h)
        case("DC refinement of %d blocks (%d x %d)" % ((w // 8) * (h // 8), w, h), fd, bd, sd)
    # interleaved: an MCU of 4:2:0 is 6 blocks, so 66 is 11 MCUs of all three components and 64 is what Cb and Cr interleaved make of
    # 32 MCUs (luma's 128 follow alone); 16 MCUs of 4:2:2 are 64 blocks of all three
    fd = pw.colour_frame(176, 16, 2, 2)
    bd, sd = _dc_refinement(fd, 50)
    case("DC refinement of 66 interleaved blocks (4:2:0)", fd, bd, sd)
    fd = pw.colour_frame(128, 64, 2, 2)
    bd, sd = _dc_refinement(fd, 51)
    sd = [sd[0], ([1, 2], 0, 0, 1, 0), ([0], 0, 0, 1, 0)] + sd[2:]
    case("DC refinement of 64 interleaved blocks (4:2:0, Cb and Cr)", fd, bd, sd)
    fd = pw.colour_frame(64, 32, 2, 1)
    bd, sd = _dc_refinement(fd, 52)
    case("DC refinement of 64 interleaved blocks (4:2:2)", fd, bd, sd)

    f440 = pw.colour_frame(40, 48, 1, 2)
    case("4:4:0, libjpeg script", f440, pw._blocks(f440, 53), pw.libjpeg_script(f440))
    f440 = pw.colour_frame(17, 9, 1, 2)
    case("4:4:0 17x9", f440, pw._blocks(f440, 54, density=0.4), pw.libjpeg_script(f440))
    # (17 x 9 is one MCU row of two block rows, both with pixels; 9 x 17 is two MCU rows, and the fourth block row has none)
    f440 = pw.colour_frame(9, 17, 1, 2)
    case("4:4:0 9x17: luma blocks only the interleaved scan carries", f440, pw._blocks(f440, 57, density=0.4), pw.libjpeg_script(f440))

    fe = pw.gray_frame(1456, 1448)
    case("EOB runs of 32767 blocks", fe, _empty(fe, 55), last)

    fw = pw.gray_frame(16, 8)
    bw = _empty(fw, 56)
    bw[0][0, :, 0] = (30000, 60000)
    case("beyond int16: a DC term", fw, bw, [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)], wide=True)
    fw, bw, sw = _wide([(0, 20, 32767), (1, 41, -32767)])
    case("beyond int16: a correction", fw, bw, sw, wide=True)
    fw, bw, sw = _wide([(0, 63, 32767), (1, 1, -32767)])
    case("beyond int16: corrections at positions 63 and 1", fw, bw, sw, wide=True)
    return out


@functools.lru_cache(maxsize=None)
def large_batch(n=600):
    """n grey 16 x 8 files, every one with its own coefficients, 2, 3 or 6 scans in rotation"""
    frame = pw.gray_frame(16, 8)
    scripts = ([([0], 0, 0, 0, 0), ([0], 1, 63, 0, 0)], [([0], 0, 0, 0, 0), ([0], 1, 63, 0, 1), ([0], 1, 63, 1, 0)], pw.libjpeg_script(frame))
    return [pw.progressive(frame, pw._blocks(frame, 1000 + i, density=0.3), scripts[i % 3]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def mixed_geometry():
    """(files, odd): the first file sets the batch's geometry (48 x 40 4:2:0); files of another size and of another subsampling stand
    between files that are walked"""
    f420, small, f444 = pw.colour_frame(48, 40, 2, 2), pw.colour_frame(40, 40, 2, 2), pw.colour_frame(48, 40)

    def one(frame, seed):
        return pw.progressive(frame, pw._blocks(frame, seed), pw.libjpeg_script(frame))

    return [one(f420, 60), one(small, 61), one(f420, 62), one(f444, 63), one(f420, 64)], [1, 3]
