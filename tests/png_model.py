"""png.Encode(w, *image.RGBA) restated in Python, with this project's own zlib stream: the model the GPU PNG encoder is held to.

Two halves:
  * Go's visible decisions, kept exactly (image/png writer.go, restated from Go 1.24 as recalled, not run -- PARITY UNPINNED against
    Go itself): colour type 2 (RGB 8) when RGBA.Opaque() holds, else 6 (RGBA 8) with the writer's fast-path un-premultiply; per row
    the filter with the smallest sum of abs8 over the filtered bytes, candidates in Go's order Up, Paeth, None, Sub, Average (the
    earlier wins a tie), the previous row of the first row all zeros.  IHDR, IDAT chunks, IEND; no other chunk.
  * The deflate stream, which is OURS and not compress/flate's: segments of whole rows compressed independently (one dynamic-Huffman
    block and an empty stored block each), matches from a fixed set of distances plus one hashed candidate, a greedy parse, every
    segment its own IDAT chunk, the Adler-32 in a last 4-byte IDAT chunk.  Any inflater decodes it to the filtered rows png.Encode
    would have compressed; the bytes are held to this model, and Go's compressed bytes are not claimed.

The constants are defined here and once in imageprocessor_amd/csrc/ipx_png.h.  A helper of the tests only: the product never imports it.
"""
import struct
import zlib

import numpy as np

SEG_MIN = 65536          # a segment is whole rows, at least this many bytes of filtered stream (the frame's last takes the remainder)
TILE = 256               # hashed candidates of position i come from positions before the start of i's tile (tiles from segment start)
HASH_BITS = 15
HASH_MUL = 0x9E3779B1    # hash(j) = (u32le(data[j:j+4]) * HASH_MUL mod 2^32) >> (32 - HASH_BITS), for j + 4 <= len(data)
WINDOW = 32768
MAX_MATCH = 258
MIN_MATCH = 3
LIMIT_LITLEN, LIMIT_CL = 15, 7

SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x9c"
IEND = b"\x00\x00\x00\x00IEND\xaeB`\x82"

# RFC 1951 3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

_LEN_SYM = np.zeros(MAX_MATCH + 1, np.int64)   # match length -> length symbol - 257
for _s in range(29):
    _LEN_SYM[LEN_BASE[_s]:] = _s
_LEN_SYM[258] = 28
_DIST_SYM = np.zeros(WINDOW + 1, np.int64)
for _s in range(30):
    _DIST_SYM[DIST_BASE[_s]:] = _s


# ---- Go's decisions --------------------------------------------------------------------------------------------------------------

def raw_rows(rgba):
    """(bpp, h x (w*bpp) uint8): the rows png.Encode filters for an *image.RGBA (h x w x 4, premultiplied)"""
    rgba = np.asarray(rgba, np.uint8)
    if rgba.ndim != 3 or rgba.shape[2] != 4 or rgba.shape[0] < 1 or rgba.shape[1] < 1:
        raise ValueError("png: invalid image size")
    h, w = rgba.shape[:2]
    if (rgba[..., 3] == 0xFF).all():           # RGBA.Opaque(): colour type 2
        return 3, np.ascontiguousarray(rgba[..., :3]).reshape(h, w * 3)
    return 4, unpremultiply(rgba).reshape(h, w * 4)


def unpremultiply(rgba):
    """the writer's cbTCA8 fast path for *image.RGBA: alpha 0 -> 0 0 0 0, 255 -> as is, else c * 0xffff * 0x101 / (a * 0x101) >> 8"""
    s = np.asarray(rgba, np.uint32)
    a = s[..., 3:4]
    q = (s[..., :3] * 0x101 * 0xFFFF) // np.maximum(a * 0x101, 1)
    c = ((q >> 8) & 0xFF).astype(np.uint8)
    out = np.empty(s.shape, np.uint8)
    out[..., :3] = np.where(a == 0xFF, s[..., :3], np.where(a == 0, 0, c))
    out[..., 3] = s[..., 3]
    return out


def _abs8(d):
    d = d.astype(np.int64)
    return np.where(d < 128, d, 256 - d)


def paeth(a, b, c):
    a, b, c = (np.asarray(v, np.int64) for v in (a, b, c))
    pa = b - c
    pb = a - c
    pc = np.abs(pa + pb)
    pa, pb = np.abs(pa), np.abs(pb)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


# Go tries Up, Paeth, None, Sub, Average in that order and keeps the first strict minimum
FILTER_ORDER = [2, 4, 0, 1, 3]


def filter_rows(raw, bpp):
    """-> (filter type per row, h x rowbytes filtered bytes)"""
    raw = np.asarray(raw, np.uint8)
    h, n = raw.shape
    x = raw.astype(np.int64)
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :-bpp]
    cand = {0: x, 1: x - a, 2: x - b, 3: x - (a + b) // 2, 4: x - paeth(a, b, c)}
    cand = {k: (v & 0xFF).astype(np.uint8) for k, v in cand.items()}
    scores = np.stack([_abs8(cand[k]).sum(axis=1) for k in FILTER_ORDER])
    types = np.array(FILTER_ORDER, np.uint8)[np.argmin(scores, axis=0)]
    out = np.empty((h, n), np.uint8)
    for k in range(5):
        out[types == k] = cand[k][types == k]
    return types, out


def filtered_stream(rgba):
    """(bpp, w, h, the bytes png.Encode hands zlib: per row the filter type then the filtered bytes)"""
    bpp, raw = raw_rows(rgba)
    types, f = filter_rows(raw, bpp)
    h, w = raw.shape[0], raw.shape[1] // bpp
    return bpp, w, h, np.concatenate([types[:, None], f], axis=1).reshape(-1)


def ihdr(w, h, bpp):
    body = b"IHDR" + struct.pack(">IIBBBBB", w, h, 8, 2 if bpp == 3 else 6, 0, 0, 0)
    return struct.pack(">I", 13) + body + struct.pack(">I", zlib.crc32(body))


def chunk(kind, data):
    body = kind + bytes(data)
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body))


# ---- segments and the stored bound -----------------------------------------------------------------------------------------------

def segments(w, h, bpp):
    """[(start, end)] byte ranges of the filtered stream: rows_per_seg = max(1, ceil(SEG_MIN / stride)) rows each, stride = 1 + w*bpp;
    max(1, h // rows_per_seg) segments, the last one taking every remaining row"""
    stride = 1 + w * bpp
    rps = max(1, -(-SEG_MIN // stride))
    nseg = max(1, h // rps)
    rows = [s * rps for s in range(nseg)] + [h]
    return [(rows[s] * stride, rows[s + 1] * stride) for s in range(nseg)]


def stored_bytes(length, first):
    """a segment of `length` bytes as stored blocks of <= 65535 bytes, then the empty stored block (whole chunk data bytes)"""
    return (2 if first else 0) + 5 * (-(-length // 65535)) + length + 5


def stream_bound(w, h, bpp):
    """the longest stream the encoder can emit for a w x h frame of this bpp: every segment stored"""
    segs = segments(w, h, bpp)
    return 8 + 25 + sum(12 + stored_bytes(e - s, k == 0) for k, (s, e) in enumerate(segs)) + 16 + 12


# ---- match candidates and the parse ----------------------------------------------------------------------------------------------

def fixed_distances(w, bpp):
    stride = 1 + w * bpp
    return sorted(d for d in {1, 2, 3, 4, bpp, stride, 2 * stride} if d <= WINDOW)


def hashes(data):
    """hash of the 4 bytes at every j with j + 4 <= len(data)"""
    d = np.asarray(data, np.uint64)
    if len(d) < 4:
        return np.zeros(0, np.int64)
    v = d[:-3] | d[1:-2] << np.uint64(8) | d[2:-1] << np.uint64(16) | d[3:] << np.uint64(24)
    return (((v * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def _words(data):
    """8 bytes little-endian starting at every position (zero padded past the end)"""
    pad = np.concatenate([np.asarray(data, np.uint8), np.zeros(MAX_MATCH + 16, np.uint8)])
    return np.ndarray((len(data) + MAX_MATCH,), np.dtype("<u8"), pad, 0, (1,))


def _common_prefix(W, i, j, cap):
    """number of equal bytes data[i + k] == data[j + k], k < cap (vectors of positions)"""
    out = np.zeros(len(i), np.int64)
    act = np.arange(len(i))
    k = 0
    while act.size and k < MAX_MATCH:
        x = W[i[act] + k] ^ W[j[act] + k]
        same = x == 0
        diff = act[~same]
        xd = x[~same]
        low = xd & (~xd + np.uint64(1))
        out[diff] = k + (np.log2(low.astype(np.float64)).astype(np.int64) >> 3)
        act = act[same]
        k += 8
        out[act] = k
    return np.minimum(out, cap)


def best_matches(data, w, bpp):
    """(len, dist) of the winning candidate at every position (len < MIN_MATCH: a literal)"""
    data = np.asarray(data, np.uint8)
    n = len(data)
    segs = segments(w, (n // (1 + w * bpp)), bpp)
    segend = np.empty(n, np.int64)
    tile0 = np.empty(n, np.int64)
    pos = np.arange(n, dtype=np.int64)
    for s, e in segs:
        segend[s:e] = e
        tile0[s:e] = s + (pos[s:e] - s) // TILE * TILE
    cap = np.minimum(MAX_MATCH, segend - pos)
    best_len = np.zeros(n, np.int64)
    best_dist = np.zeros(n, np.int64)
    for d in fixed_distances(w, bpp):
        if d >= n:
            continue
        e = data[d:] == data[:-d]                       # e[k]: data[d + k] == data[k], i.e. position i = d + k matches back d
        m = len(e)
        nf = np.minimum.accumulate(np.where(e, m, np.arange(m))[::-1])[::-1]
        ln = np.minimum(nf - np.arange(m), cap[d:])
        upd = ln > best_len[d:]
        best_len[d:][upd] = ln[upd]
        best_dist[d:][upd] = d
    hv = hashes(data)
    if len(hv):
        q = np.arange(len(hv), dtype=np.int64)
        key = hv * (n + 1) + q
        skey = np.sort(key)
        at = np.searchsorted(skey, hv * (n + 1) + tile0[: len(hv)], "left") - 1
        ok = at >= 0
        jk = np.where(ok, skey[np.maximum(at, 0)], -1)
        ok &= jk // (n + 1) == hv
        j = jk % (n + 1)
        ok &= q - j <= WINDOW
        i = q[ok]
        j = j[ok]
        ln = _common_prefix(_words(data), i, j, cap[i])
        dist = i - j
        upd = (ln > best_len[i]) | ((ln == best_len[i]) & (dist < best_dist[i]))
        best_len[i[upd]] = ln[upd]
        best_dist[i[upd]] = dist[upd]
    best_len[best_len < MIN_MATCH] = 0
    return best_len, best_dist, segs


def parse(best_len, start, end):
    """greedy from the segment's first byte: token positions in order"""
    step = np.maximum(best_len[start:end], 1).tolist()
    out = []
    p = 0
    n = end - start
    while p < n:
        out.append(p)
        p += step[p]
    return np.array(out, np.int64) + start


# ---- Huffman ---------------------------------------------------------------------------------------------------------------------

def huffman_lengths(freq, limit):
    """code lengths: two-queue Huffman over the used symbols sorted by (frequency, symbol) (a leaf goes before an internal node of the
    same weight); lengths limited to `limit` by JPEG Annex K.3's adjustment of the length counts; the lengths then go, shortest first,
    to the symbols in descending (frequency, symbol) order.  Fewer than two used symbols: the lowest unused ones get frequency 1."""
    f = [int(v) for v in freq]
    k = 0
    while sum(1 for v in f if v) < 2:
        if f[k] == 0:
            f[k] = 1
        k += 1
    syms = sorted((s for s in range(len(f)) if f[s]), key=lambda s: (f[s], s))
    m = len(syms)
    weight = [f[s] for s in syms]
    parent = [0] * (2 * m - 1)
    li = qi = 0
    for node in range(m, 2 * m - 1):
        kids = []
        for _ in range(2):
            if li < m and (qi >= node - m or weight[li] <= weight[m + qi]):
                kids.append(li)
                li += 1
            else:
                kids.append(m + qi)
                qi += 1
        weight.append(weight[kids[0]] + weight[kids[1]])
        parent[kids[0]] = parent[kids[1]] = node
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    bits = [0] * (2 * m + limit + 1)
    for leaf in range(m):
        bits[depth[leaf]] += 1
    for i in range(len(bits) - 1, limit, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    lengths = [0] * len(f)
    order = syms[::-1]
    at = 0
    for ln in range(1, limit + 1):
        for _ in range(bits[ln]):
            lengths[order[at]] = ln
            at += 1
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 codes, bit-reversed for LSB-first packing"""
    mx = max(lengths)
    count = [0] * (mx + 1)
    for ln in lengths:
        if ln:
            count[ln] += 1
    nxt = [0] * (mx + 2)
    code = 0
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1 if b > 1 else 0
        nxt[b] = code
    codes = [0] * len(lengths)
    for s, ln in enumerate(lengths):
        if ln:
            c = nxt[ln]
            nxt[ln] += 1
            codes[s] = int(format(c, "0%db" % ln)[::-1], 2)
    return codes


def rle_code_lengths(seq):
    """the code lengths as code-length symbols [(symbol, extra value, extra bits)]: per run of one value r long, zeros as 18 (11..138)
    while r >= 11, then 17 (3..10) if r >= 3, then single zeros; a non-zero value once, then 16 (3..6) while r >= 3, then singles"""
    out = []
    i = 0
    n = len(seq)
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11, 7))
                r -= k
            if r >= 3:
                out.append((17, r - 3, 3))
                r = 0
            out.extend([(0, 0, 0)] * r)
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3, 2))
                r -= k
            out.extend([(v, 0, 0)] * r)
    return out


# ---- bits ------------------------------------------------------------------------------------------------------------------------

def _pack(vals, nbits):
    """LSB-first concatenation of (vals[k], nbits[k]) -> (bytes, total bits); a partial last byte is zero-padded"""
    vals = np.asarray(vals, np.uint64)
    nbits = np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    out = []
    for c0 in range(0, len(vals), 1 << 18):
        v, nb = vals[c0:c0 + (1 << 18)], nbits[c0:c0 + (1 << 18)]
        bit = (v[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
        out.append(bit[np.arange(64)[None, :] < nb[:, None]].astype(np.uint8))
    bits = np.concatenate(out) if out else np.zeros(0, np.uint8)
    return np.packbits(bits, bitorder="little").tobytes(), total


def deflate_segment(data, best_len, best_dist, start, end, first, last):
    """the chunk data of one segment: [78 9C], a dynamic block or stored blocks, the empty stored block (BFINAL on the last)"""
    seg = data[start:end]
    pos = parse(best_len, start, end)
    ln = best_len[pos]
    di = best_dist[pos]
    is_m = ln >= MIN_MATCH
    lsym = np.where(is_m, 257 + _LEN_SYM[ln], data[pos])
    dsym = _DIST_SYM[di]
    lfreq = np.bincount(lsym, minlength=286)
    lfreq[256] += 1
    dfreq = np.bincount(dsym[is_m], minlength=30)
    llen = huffman_lengths(lfreq, LIMIT_LITLEN)
    dlen = huffman_lengths(dfreq, LIMIT_LITLEN)
    hlit = max(257, max(s for s in range(286) if llen[s]) + 1)
    hdist = max(1, max(s for s in range(30) if dlen[s]) + 1)
    cl = rle_code_lengths(llen[:hlit] + dlen[:hdist])
    cfreq = np.bincount([c for c, _, _ in cl], minlength=19)
    clen = huffman_lengths(cfreq, LIMIT_CL)
    hclen = max(4, max(k for k in range(19) if clen[CL_ORDER[k]]) + 1)
    lcode, dcode, ccode = canonical_codes(llen), canonical_codes(dlen), canonical_codes(clen)
    # the header
    hv, hn = [], []
    if first:
        hv += [0x78, 0x9C]
        hn += [8, 8]
    hv += [0, 2, hlit - 257, hdist - 1, hclen - 4] + [clen[CL_ORDER[k]] for k in range(hclen)]
    hn += [1, 2, 5, 5, 4] + [3] * hclen
    for c, x, xb in cl:
        hv.append(ccode[c] | x << clen[c])
        hn.append(clen[c] + xb)
    # the tokens: code, length extra, distance code, distance extra in one value of <= 48 bits
    la, lc = np.array(llen, np.int64), np.array(lcode, np.uint64)
    da, dc = np.array(dlen, np.int64), np.array(dcode, np.uint64)
    lx = np.where(is_m, np.array(LEN_EXTRA + [0], np.int64)[np.clip(lsym - 257, 0, 29)], 0)
    lxv = np.where(is_m, ln - np.array(LEN_BASE + [0], np.int64)[np.clip(lsym - 257, 0, 29)], 0)
    dx = np.where(is_m, np.array(DIST_EXTRA, np.int64)[dsym], 0)
    dxv = np.where(is_m, di - np.array(DIST_BASE, np.int64)[dsym], 0)
    n1 = la[lsym]
    v = lc[lsym] | (lxv.astype(np.uint64) << n1.astype(np.uint64))
    n2 = n1 + lx
    v = v | np.where(is_m, (dc[dsym] | (dxv.astype(np.uint64) << da[dsym].astype(np.uint64))) << n2.astype(np.uint64), 0).astype(np.uint64)
    nt = n2 + np.where(is_m, da[dsym] + dx, 0)
    vals = np.concatenate([np.array(hv, np.uint64), v, np.array([lcode[256], 1 if last else 0], np.uint64)])
    nbits = np.concatenate([np.array(hn, np.int64), nt, np.array([llen[256], 3], np.int64)])
    body, total = _pack(vals, nbits)
    dyn = body + b"\x00\x00\xff\xff"
    assert len(body) == (total + 7) // 8
    if stored_bytes(end - start, first) < len(dyn):
        out = bytearray(ZLIB_HEADER if first else b"")
        for k in range(0, len(seg), 65535):
            part = seg[k:k + 65535]
            out += struct.pack("<BHH", 0, len(part), len(part) ^ 0xFFFF) + part.tobytes()
        out += struct.pack("<BHH", 1 if last else 0, 0, 0xFFFF)
        return bytes(out)
    return dyn


def zlib_from_filtered(data, w, bpp):
    """the IDAT chunks (bytes) of one filtered stream"""
    data = np.asarray(data, np.uint8)
    best_len, best_dist, segs = best_matches(data, w, bpp)
    out = bytearray()
    for k, (s, e) in enumerate(segs):
        out += chunk(b"IDAT", deflate_segment(data, best_len, best_dist, s, e, k == 0, k == len(segs) - 1))
    out += chunk(b"IDAT", struct.pack(">I", zlib.adler32(data.tobytes())))
    return bytes(out)


def png_encode(rgba):
    """the whole PNG stream of one *image.RGBA frame (h x w x 4 uint8, premultiplied)"""
    bpp, w, h, data = filtered_stream(rgba)
    return SIGNATURE + ihdr(w, h, bpp) + zlib_from_filtered(data, w, bpp) + IEND


def read_chunks(stream):
    """[(kind, data)] of a PNG stream; every CRC checked"""
    assert stream[:8] == SIGNATURE
    out = []
    p = 8
    while p < len(stream):
        n, = struct.unpack(">I", stream[p:p + 4])
        kind = stream[p + 4:p + 8]
        data = stream[p + 8:p + 8 + n]
        crc, = struct.unpack(">I", stream[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(kind + data), "bad CRC in %r chunk at %d" % (kind, p)
        out.append((kind, data))
        p += 12 + n
    assert p == len(stream)
    return out
