"""Regenerates this fixture: python generate.py /path/to/reference/src/build_alignment_dict.py

Writes src.txt / dst.txt (the lines LINES of ../sample_enfa, English and Persian) and align.txt (the hand-written Pharaoh links
below, one line per pair) and runs the reference's script on them with the tokenizer of ../marshal_kat/tok to produce
expected.txt.  The script looks whole whitespace words up in the vocabulary (``token_id(word)``): with this 90-entry vocabulary
only a few short English words have an id of their own ("in" 48, "at" 73, "or" 86, "use" 56, "a" 8, "be" 41, "he" 85) and every
other word, all Persian ones included, is id 0.  So the links below give
  * a word on both sides: id 0 linked to id 0 (the script tests one direction, then sets both);
  * a key with more than five translations: 0 is linked to 0, 48, 73, 86, 56, 8, 41 and 85;
  * probability ties: 73, 86, 56, 8, 41 and 85 are each linked to 0 once, so the five best of key 0 are decided by the order in
    which they were first seen;
  * a pair without links (an empty alignment line)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "..", "sample_enfa")
TOK = os.path.join(HERE, "..", "marshal_kat", "tok")
LINES = [3, 5, 9, 7, 12, 35, 46]
ALIGN = [
    "0-0 16-3 16-4 24-5 1-1",   # 0-0, in-0, in-0, at-0, 0-0
    "7-0 15-1 17-2 21-3 0-4",   # in-0 x 3, or-0, 0-0
    "1-0 0-1",                  # use-0, 0-0
    "",
    "8-2",                      # a-0
    "2-0 4-1",                  # be-0, in-0
    "11-3",                     # he-0
]


def main(script):
    for name, out in (("en.txt", "src.txt"), ("fa.txt", "dst.txt")):
        with open(os.path.join(SAMPLE, name), encoding="utf-8") as fp:
            lines = fp.read().split("\n")
        with open(os.path.join(HERE, out), "w", encoding="utf-8") as w:
            for i in LINES:
                w.write(lines[i].strip() + "\n")
    with open(os.path.join(HERE, "align.txt"), "w") as w:
        for a in ALIGN:
            w.write(a + "\n")
    subprocess.run([sys.executable, script, "--src", os.path.join(HERE, "src.txt"), "--dst", os.path.join(HERE, "dst.txt"),
                    "--align", os.path.join(HERE, "align.txt"), "--output", os.path.join(HERE, "expected.txt"), "--tok", TOK],
                   check=True)


if __name__ == "__main__":
    main(sys.argv[1])
