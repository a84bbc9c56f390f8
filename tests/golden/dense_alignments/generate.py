"""Regenerates this fixture: python generate.py /path/to/reference/src/scripts/extract_dense_alignments.py

Writes src.txt / dst.txt (the lines LINES of ../sample_enfa) and align.txt (hand-written Pharaoh links, one line per pair) and
runs the reference's script on them with min_density MIN to produce expected.txt (``src ||| dst`` of the pairs it keeps).
(English words, Persian words, links) per line and what it exercises:
  43: (7, 7, 4)    density 0.57, kept
   9: (8, 7, 4)    density exactly 0.5, kept
  11: (6, 8, 4)    ratio 0.75 outside 0.9..1.1, kept through the second branch of len_condition (difference 2, both >= 5)
  38: (12, 12, 5)  density 0.42: fails the density alone
  62: (6, 17, 9)   density 0.53, both sides >= 5, fails len_condition alone (ratio 0.35, difference 11)
  17: (4, 4, 4)    density 1 and ratio 1: fails the two ``>= 5`` conditions only
  40: (3, 5, 3)    source below 5 words (no ratio within 0.9..1.1 exists for 4 against 5 or more, so len_condition fails with it)
  70: (7, 4, 4)    target below 5 words
  25: (15, 15, -)  an empty alignment line: the script counts it as ONE link (density 0.07), the port as none; dropped either way"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "..", "sample_enfa")
MIN = 0.5
LINES = [43, 9, 11, 38, 62, 17, 40, 70, 25]
ALIGN = [
    "0-0 1-2 3-3 6-6",
    "0-0 1-1 2-3 7-6",
    "0-1 2-2 3-5 5-7",
    "0-0 2-1 4-4 7-8 11-11",
    "0-0 0-1 1-3 1-4 2-6 3-8 4-10 5-13 5-16",
    "0-0 1-1 2-2 3-3",
    "0-0 1-2 2-4",
    "0-0 2-1 4-2 6-3",
    "",
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
    subprocess.run([sys.executable, script, os.path.join(HERE, "src.txt"), os.path.join(HERE, "dst.txt"),
                    os.path.join(HERE, "align.txt"), str(MIN), os.path.join(HERE, "expected.txt")], check=True)


if __name__ == "__main__":
    main(sys.argv[1])
