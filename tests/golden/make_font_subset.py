#!/usr/bin/env python3
"""Writes tests/golden/DejaVuSans-subset.ttf: the glyphs of DejaVu Sans the font tests draw, so that they need no
font installed on the machine.

DejaVu Sans is free to redistribute and modify (Bitstream Vera licence, DejaVu changes in the public domain); the
copyright and licence strings stay in the subset's name table.  The subset keeps what the tests look at: the
Unicode cmap subtables in their original order (format 4 first, then format 12 with U+1F600), the legacy 'kern'
table, the TrueType hinting programs (FreeType through Pillow reads them), and every component of the compound
glyphs (é, Å, Ǆ).

Run:  python tests/golden/make_font_subset.py [path/to/DejaVuSans.ttf]
"""
import os
import sys

from fontTools import subset
from fontTools.ttLib import TTFont

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "DejaVuSans-subset.ttf")
SOURCE = "/usr/share/fonts/truetype/dejavu/DejaVuSans.ttf"
# printable ASCII, the code points test_font.py asks the tables about, and every character the font tests draw
TEXT = "".join(chr(c) for c in range(32, 127)) + "©éЖ€\U0001F600�" + "gjQ@&%éÅЖǄ≠½" + "Grüße, Welt!"


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else SOURCE
    opts = subset.Options()
    opts.legacy_kern = True
    opts.hinting = True
    opts.notdef_outline = True
    opts.name_IDs = ["*"]
    opts.name_languages = ["*"]
    opts.name_legacy = True
    opts.glyph_names = True
    opts.drop_tables += ["GSUB", "GPOS", "GDEF", "MATH", "FFTM"]
    font = TTFont(src, recalcTimestamp=False)
    sub = subset.Subsetter(opts)
    sub.populate(text=TEXT)
    sub.subset(font)
    font.save(OUT)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
