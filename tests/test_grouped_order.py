"""Tile order of the grouped weight-gradient launch (imt_gemm_grouped_tile_order: the host evaluation of the mapping the
kernel uses, csrc/gemm.hip grouped_tile).  No GPU.

The mapping hardware workgroup -> (problem, tile row, tile column) must be a bijection onto the group's tile list for every
group the launch takes: 1 to 16 problems (two layers' worth), grids from 1 x 1 to 16 x 16 tiles, totals that are no multiple
of the 8 XCDs; and XCD x must get the x-th contiguous run of the concatenated row-major lists.

(An order that walks each problem in bands, so that an XCD's share of a problem is a compact block of tiles, was measured and
not kept: it touches fewer operand strips -- summed over the 8 XCDs 88 against 113 for an encoder layer of the flagship model,
104 against 116 for a decoder layer, 144 against 168 and 184 against 184 for the pairs -- and moves fewer bytes, but the
launch is no faster.  DESIGN.md section 5.)"""
import random

import pytest

from imagetranslate_amd import hip_ops as O

# dW2, dW1, out-proj, q|k|v of an encoder layer; dW2, dW1, cross out-proj, cross q, cross k|v, out-proj, q|k|v of a decoder layer
# of the flagship model (d = 512, ff = 2048) in 128 x 128 tiles
ENC = [(4, 16), (16, 4), (4, 4), (12, 4)]
DEC = [(4, 16), (16, 4), (4, 4), (4, 4), (8, 4), (4, 4), (12, 4)]


def _tall(grids):
    """The same products in tiles of 256 rows."""
    return [(r // 2, c) for r, c in grids]


def _row_major(grids):
    return [(p, i, j) for p, (r, c) in enumerate(grids) for i in range(r) for j in range(c)]


def _sweep():
    rng = random.Random(7)
    groups = [[(r, c)] for r in range(1, 17) for c in range(1, 17)]  # one problem, every grid from 1 x 1 to 16 x 16
    while len(groups) < 256 + 400:
        n = rng.randint(1, 16)
        g = []
        for _ in range(n):
            r, c = rng.randint(1, 16), rng.randint(1, 16)
            if sum(a * b for a, b in g) + r * c + (n - len(g) - 1) > 640:
                r, c = 1, 1
            g.append((r, c))
        groups.append(g)
    groups += [ENC, DEC, ENC + ENC, DEC + DEC, _tall(ENC + ENC), _tall(DEC + DEC), [(1, 1)] * 16, [(16, 16), (16, 16), (8, 16)]]
    return groups


@pytest.mark.parametrize("plain", [False, True])
def test_tile_order_is_a_bijection(plain):
    groups = _sweep()
    assert any(sum(r * c for r, c in g) % 8 for g in groups) and {len(g) for g in groups} == set(range(1, 17))
    for g in groups:
        tiles = _row_major(g)
        got = O.grouped_tile_order(g, plain=plain)
        assert sorted(got) == tiles, g
        if plain:  # IMT_GROUPED_PLAIN_ORDER: workgroup w takes tile w of the row-major lists
            assert got == tiles, g
            continue
        # XCD x (workgroups x, x + 8, ...) walks the x-th contiguous run of the list; the first total % 8 runs are one longer
        q, rem = divmod(len(tiles), 8)
        start = 0
        for x in range(8):
            n = q + (1 if x < rem else 0)
            assert got[x::8] == tiles[start:start + n], (g, x)
            start += n


def test_tile_order_rejects_bad_groups():
    from imagetranslate_amd import _lib as L
    for g in ([(1, 1)] * 17, [(0, 4)], [(26, 26)]):
        with pytest.raises(L.ImtError):
            O.grouped_tile_order(g)
