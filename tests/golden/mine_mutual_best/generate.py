"""Regenerates this fixture: python generate.py /path/to/reference/src/comparable/extract_best_comparable.py

Writes the candidate table (src.txt, dst.txt, scores.txt: one candidate pair per line, every pair of 6 x 7 one-token sentences
in (source, target) order, so "first seen" is "lowest index" and the script's division by the sentence length is by 1) and runs
the reference's script on it with --min 0.3 to produce expected.txt.  The table holds repeated sentences with equal scores (s0
and s1 tie for t0, t0 and t1 tie for s0, likewise s2 / s3 and t2 / t3, t5 / t6), two kept pairs of equal score, and a mutual
best pair (s4, t4) below --min.  All scores are multiples of 1/8: they print and parse exactly."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MIN = 0.3
SIM = [
    [0.875, 0.875, 0.125, 0.0, 0.125, 0.125, 0.0],
    [0.875, 0.25, 0.5, 0.125, 0.0, 0.25, 0.125],
    [0.125, 0.25, 0.75, 0.75, 0.125, 0.0, 0.25],
    [0.0, 0.125, 0.75, 0.625, 0.125, 0.125, 0.0],
    [0.125, 0.0, 0.125, 0.125, 0.25, 0.125, 0.125],
    [0.125, 0.5, 0.0, 0.125, 0.125, 0.75, 0.75],
]


def main(script):
    with open(os.path.join(HERE, "src.txt"), "w") as fs, open(os.path.join(HERE, "dst.txt"), "w") as fd, \
            open(os.path.join(HERE, "scores.txt"), "w") as fc:
        for s, row in enumerate(SIM):
            for t, v in enumerate(row):
                fs.write("s%d\n" % s)
                fd.write("t%d\n" % t)
                fc.write("%s\n" % v)
    subprocess.run([sys.executable, script, "--src", os.path.join(HERE, "src.txt"), "--dst", os.path.join(HERE, "dst.txt"),
                    "--scores", os.path.join(HERE, "scores.txt"), "--output", os.path.join(HERE, "expected.txt"), "--min", str(MIN)],
                   check=True)


if __name__ == "__main__":
    main(sys.argv[1])
