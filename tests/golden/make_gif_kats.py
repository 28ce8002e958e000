"""Writes tests/golden/gif_kats.json: known answers of compress/lzw's writer (LSB, literal width 8) derived WITHOUT tests/gif_model.py.

  * "four zeros" and "sixteen ones": the code sequences worked out by hand (comments below), packed LSB-first;
  * "no repeats": an index sequence in which no two adjacent bytes repeat a pair (Martin's greedy de Bruijn walk), so the dictionary never
    matches and every code is a literal -- the stream follows from the width schedule alone (9 bits until hi reaches 512, 10 until 1024,
    11 until 2048, then 12) and the clear rule (a clear code, at the current width, once hi reaches 4095; widths restart at 9).  Long
    enough to pass the first clear;
  * "sub-block boundary": the shortest prefix of that sequence whose LZW data is exactly 510 bytes (two full sub-blocks, then the lone
    0x00 terminator).

python tests/golden/make_gif_kats.py   (rewrites the file; the data are fixed by the rules, no seed involved)"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def pack(codes_widths):
    bits = nbits = 0
    out = bytearray()
    for c, w in codes_widths:
        bits |= c << nbits
        nbits += w
        while nbits >= 8:
            out.append(bits & 0xFF)
            bits >>= 8
            nbits -= 8
    if nbits:
        out.append(bits & 0xFF)
    return bytes(out)


def no_repeat_sequence(n):
    """Martin's walk over 256 symbols: append the largest symbol whose pair with the last one is unused"""
    nxt = [255] * 256          # next candidate per symbol, counting down
    seq = [0]
    while len(seq) < n:
        a = seq[-1]
        b = nxt[a]
        assert b >= 0
        nxt[a] = b - 1
        seq.append(b)
    return seq


def literal_codes(seq):
    """the writer's codes when the dictionary never matches: clear, then every byte but the first as it arrives (the previous byte goes
    out), the last byte on Close, EOF; with the widths of the rule above"""
    out = []
    width, hi, overflow = 9, 257, 512
    out.append((256, width))

    def inc_hi():
        nonlocal width, hi, overflow
        hi += 1
        if hi == overflow:
            width += 1
            overflow <<= 1
        if hi == 4095:
            out.append((256, width))
            width, hi, overflow = 9, 257, 512

    for prev in seq[:-1]:
        out.append((prev, width))
        inc_hi()
    out.append((seq[-1], width))
    inc_hi()
    out.append((257, width))
    return out


def main():
    cases = []
    # four zeros: clear(256); 0 arrives: key (0,0) misses -> 0 out, 258 = (0,0); 0: (0,0) hits -> 258; 0: (258,0) misses -> 258 out,
    # 259 = (258,0), code 0; Close: 0 out, hi 260; EOF 257.  Five 9-bit codes, 45 bits -> 6 bytes.
    four = [(256, 9), (0, 9), (258, 9), (0, 9), (257, 9)]
    cases.append({"name": "four zeros", "index": [0] * 4, "codes": [c for c, _ in four], "lzw_hex": pack(four).hex()})
    # sixteen ones: runs of 1, 2, 3, 4, 5 pixels go out as 1, 258, 259, 260, 261 (each miss adds the run one longer), the 16th pixel
    # goes out alone on Close: 1; EOF.  Eight 9-bit codes, 72 bits -> 9 bytes.
    sixteen = [(256, 9), (1, 9), (258, 9), (259, 9), (260, 9), (261, 9), (1, 9), (257, 9)]
    cases.append({"name": "sixteen ones", "index": [1] * 16, "codes": [c for c, _ in sixteen], "lzw_hex": pack(sixteen).hex()})
    seq = no_repeat_sequence(5000)
    cw = literal_codes(seq)
    assert sum(1 for c, _ in cw if c == 256) == 2     # the first clear, and the one at hi == 4095
    cases.append({"name": "no repeats, past the 4095 clear", "index": seq, "lzw_hex": pack(cw).hex()})
    for n in range(2, 1000):
        d = pack(literal_codes(seq[:n]))
        if len(d) == 510:
            cases.append({"name": "sub-block boundary (510 bytes of LZW data)", "index": seq[:n], "lzw_hex": d.hex()})
            break
    else:
        raise AssertionError("no prefix gives 510 bytes")
    with open(os.path.join(HERE, "gif_kats.json"), "w") as f:
        json.dump({"about": "compress/lzw writer (LSB, literal width 8) known answers; see make_gif_kats.py", "cases": cases}, f)
        f.write("\n")


if __name__ == "__main__":
    main()
