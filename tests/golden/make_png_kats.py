"""Writes tests/golden/png_kats.json: known answers of image/png's writer for *image.RGBA derived WITHOUT tests/png_model.py, by a
scalar restatement written for this file (one byte at a time, the way writer.go's filter() and the cbTCA8 fast path read):

  * "filters": small frames whose second row is won by each of the five filters (found by a seeded search over tiny frames and
    checked to win by a strict margin), frames whose rows tie (a constant first row: Up ties None and Paeth ties Sub, and the
    earlier of Go's order Up, Paeth, None, Sub, Average wins), the zero previous row of the first row, bpp 3 (opaque) and 4;
  * "unpremultiply": for every alpha 1 .. 254 and colour values 0, 1, a/3, a/2, a-1, a: the byte the writer stores,
    uint8((c * 0x101 * 0xffff / (a * 0x101)) >> 8) in uint32; alpha 0 gives 0 0 0 0 and alpha 255 copies.

python tests/golden/make_png_kats.py   (rewrites the file; the search is seeded)"""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
ORDER = [2, 4, 0, 1, 3]   # Up, Paeth, None, Sub, Average


def unpremul(r, g, b, a):
    if a == 0:
        return [0, 0, 0, 0]
    if a == 255:
        return [r, g, b, a]
    return [((c * 0x101 * 0xFFFF) // (a * 0x101) >> 8) & 0xFF for c in (r, g, b)] + [a]


def raw_rows(pix, w, h):
    """pix: flat RGBA list -> (bpp, rows)"""
    opaque = all(pix[4 * i + 3] == 255 for i in range(w * h))
    rows = []
    for y in range(h):
        row = []
        for x in range(w):
            p = pix[4 * (y * w + x):4 * (y * w + x) + 4]
            row += p[:3] if opaque else unpremul(*p)
        rows.append(row)
    return (3 if opaque else 4), rows


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filter_row(cur, prev, bpp):
    """-> (scores by filter type, filtered bytes by filter type)"""
    out = {t: [] for t in range(5)}
    for i, x in enumerate(cur):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        out[0].append(x)
        out[1].append((x - a) & 0xFF)
        out[2].append((x - b) & 0xFF)
        out[3].append((x - (a + b) // 2) & 0xFF)
        out[4].append((x - paeth(a, b, c)) & 0xFF)
    score = {t: sum(d if d < 128 else 256 - d for d in out[t]) for t in range(5)}
    return score, out


def choose(score):
    best = None
    for t in ORDER:
        if best is None or score[t] < score[best]:
            best = t
    return best


def encode_rows(pix, w, h):
    bpp, rows = raw_rows(pix, w, h)
    prev = [0] * (w * bpp)
    types, filtered = [], []
    for row in rows:
        score, out = filter_row(row, prev, bpp)
        t = choose(score)
        types.append(t)
        filtered.append(out[t])
        prev = row
    return bpp, types, filtered


def case(name, pix, w, h):
    bpp, types, filtered = encode_rows(pix, w, h)
    return {"name": name, "w": w, "h": h, "rgba": pix, "bpp": bpp, "types": types, "filtered": filtered}


def search(target, bpp, rng):
    """a 4 x 2 frame whose second row `target` wins by a strict margin over every other filter"""
    w, h = 4, 2
    for _ in range(200000):
        base = [rng.randrange(256) for _ in range(3)]
        spread = rng.choice([2, 8, 40, 255])
        pix = []
        for _ in range(w * h):
            px = [min(255, max(0, v + rng.randrange(-spread, spread + 1))) for v in base]
            a = 255 if bpp == 3 else rng.choice([255, 128, 200])
            px = [c * a // 255 for c in px]
            pix += px + [a]
        got_bpp, rows = raw_rows(pix, w, h)
        if got_bpp != bpp:
            continue
        score, _ = filter_row(rows[1], rows[0], bpp)
        if all(score[target] < score[t] for t in range(5) if t != target):
            return pix
    raise RuntimeError("no frame found for filter %d" % target)


def main():
    rng = random.Random(20261015)
    cases = []
    names = {0: "None", 1: "Sub", 2: "Up", 3: "Average", 4: "Paeth"}
    for bpp in (3, 4):
        for t in range(5):
            cases.append(case("%s wins row 1, bpp %d" % (names[t], bpp), search(t, bpp, rng), 4, 2))
    # ties: a constant opaque row after the zero row: Up == None (the row itself) and Paeth == Sub (only the first pixel);
    # Paeth is ahead of Sub in Go's order and wins; the second, equal row is all zero under Up
    cases.append(case("constant rows: Paeth over Sub on the zero previous row, then Up", [7, 7, 7, 255] * 6, 3, 2))
    # a first row of zeros: every filter scores 0 and Up, the first tried, wins
    cases.append(case("zero first row: Up wins the five-way tie", [0, 0, 0, 255] * 5 + [9, 200, 3, 255] * 5, 5, 2))
    cases.append(case("alpha 0 pixels become 0 0 0 0", [10, 20, 30, 0, 40, 50, 60, 128, 1, 2, 3, 255], 3, 1))
    unp = []
    for a in range(1, 255):
        for c in sorted({0, 1, a // 3, a // 2, a - 1, a}):
            unp.append([c, a, unpremul(c, c, c, a)[0]])
    with open(os.path.join(HERE, "png_kats.json"), "w") as f:
        json.dump({"cases": cases, "unpremultiply": unp}, f, separators=(",", ":"))
        f.write("\n")
    print("%d filter cases, %d un-premultiply answers" % (len(cases), len(unp)))


if __name__ == "__main__":
    main()
