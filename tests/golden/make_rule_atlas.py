#!/usr/bin/env python3
"""Regenerate tests/golden/rule_atlas.json: tiny grids of small integers that between them fire every reachable id-source rule
of the vertices lying on a grid point (plan_visit of mc33_cell.h; tests/atlas_cases.py says what the atlas is for).  Uses the
project's own host emulator with its MC33_RULE_HOOK counters, nothing else:

    python tests/golden/make_rule_atlas.py

A seeded search over random grids (values in {-1, 0, 1} or {-2 .. 2}, isovalue 0; every 2 x 2 x 2 grid over {-1, 0, 1}
exhaustively) of the SHAPES below; the universe is every (face flags, rule word) and (face flags, edge, end point) fall-through
the search fires, and a greedy cover of it is kept.  Prints the universe per face-flag value and checks that the degenerate
fixtures of the GPU suite fire nothing outside it."""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import atlas_cases as ac  # noqa: E402
import fixtures as fx  # noqa: E402
from mc33_emu import Emu  # noqa: E402

SEED, PER_SHAPE = 50, 10000
# (nz, ny, nx) points.  Several rules read samples outside the cell or ask for x + 1 < nx, y + 1 < ny: lines and slabs of 3 .. 5
# cells; interior cells (face flags 0) need 3 x 3 x 3 points, and 4 along x or y for
# rule words 37, 38, 43 (36 samples: without these two shapes the fixtures check at the end of main() fails).
SHAPES = [(2, 2, 2), (3, 3, 3)] + \
    [s for n in (3, 4, 6) for s in ((2, 2, n), (2, n, 2), (n, 2, 2))] + \
    [s for a, b in ((3, 3), (3, 4), (4, 3)) for s in ((2, a, b), (a, 2, b), (a, b, 2))] + \
    [(3, 3, 4), (3, 4, 3)]
NOTES = {50: "Word 50 is the fourth id source of edge 7 (corners 4-7, owned where y = 0) when corner 4 equals the isovalue: it "
              "applies when corner 5 lies on the other side of the isovalue than corner 4, after word 48 (edge 4 of this cell already "
              "visited: share its id) and word 49 (corner 0 on the other side) did not.  Then edge 4 (corners 4-5) is cut too, and "
              "in every pattern the table can choose for such a sign index that names edge 7, edge 4 is named before it "
              "(word50_is_shadowed() of the generator walks all of them): word 48 always answers first."}


def word50_is_shadowed():
    """Every (sign index, pattern start) pattern_offset_word can return in which corner 4 counts as not above the isovalue (it
    equals it), corners 5 and 7 lie above and corner 0 does not, and whose pattern names edge 7: does it name edge 4 first?"""
    import make_case_atlas as mca
    lut = mca.read_lut()
    n = 0
    for i, starts in mca.structural_starts().items():
        above = [(i >> (7 - k)) & 1 for k in range(8)]  # (sign bit of v = isovalue - sample)
        if above[4] or above[0] or not above[5] or not above[7]:
            continue
        for p in starts:
            order, pos = [], p
            while True:
                pos += 1
                order += [e for e in ((lut[pos] >> s) & 15 for s in (0, 4, 8)) if e not in order]
                if not lut[pos] >> 12:
                    break
            if 7 in order:
                n += 1
                if 4 not in order or order.index(7) < order.index(4):
                    return False
    return n > 0


def units_of(rules, falls):
    u = [("r", int(f), int(r)) for f, r in zip(*np.nonzero(rules))]
    return u + [("f", int(f), int(e), int(k)) for f, e, k in zip(*np.nonzero(falls))]


def main():
    emu = Emu("f32")

    def fire(a):
        emu.rule_counts_reset()
        emu.isosurface(a, 0.0)
        return units_of(*emu.rule_counts())

    rng = np.random.Generator(np.random.PCG64(SEED))
    seen, kept = {}, []

    def consider(a):
        u = fire(a)
        rare = False
        for k in u:
            seen[k] = seen.get(k, 0) + 1
            rare |= seen[k] <= 12
        if rare:
            kept.append((a.copy(), frozenset(u)))

    for v in itertools.product((-1, 0, 1), repeat=8):
        consider(np.array(v, np.float32).reshape(2, 2, 2))
    for shape in SHAPES:
        for k in range(PER_SHAPE):
            top = 1 if k % 2 else 2
            a = rng.integers(-top, top + 1, shape)
            a[rng.random(shape) < 0.25] = 0  # (more samples equal to the isovalue than a uniform draw gives)
            consider(a.astype(np.float32))
    universe = set(seen)
    # greedy cover: the grid that fires most units still missing, the smaller grid on a tie
    missing, cover = set(universe), []
    while missing:
        a, u = max(kept, key=lambda c: (len(c[1] & missing), -c[0].size))
        assert u & missing
        cover.append(a)
        missing -= u
    # what the suite's degenerate fixtures fire lies inside the universe
    outside = set()
    for data in [fx.noise_quant(32, s) - np.float32(iso) for s, iso in ((1, 0.0), (1, 1.0), (2, 0.0), (3, -1.0), (7, 2.0))] + \
            [fx.noise_quant(0, 9, L=3, shape=(7, 9, 300)), fx.noise_quant(0, 4, L=2, shape=(20, 20, 20))]:
        outside |= set(fire(data)) - universe
    assert not outside, "fired by the fixtures, missed by the search: %s" % sorted(outside)
    rules = sorted([k[1], k[2]] for k in universe if k[0] == "r")
    falls = sorted([k[1], k[2], k[3]] for k in universe if k[0] == "f")
    for f in range(8):
        print("flags %d: %2d rules, %2d fall-throughs" % (f, sum(r[0] == f for r in rules), sum(r[0] == f for r in falls)))
    words = sorted(set(range(81)) - set(r[1] for r in rules))
    print("rule words fired nowhere: %s" % words)
    assert words == [50] and word50_is_shadowed(), "the note on word 50 no longer holds"
    print("%d grids, at most %d samples each" % (len(cover), max(a.size for a in cover)))
    doc = {"generator": "tests/golden/make_rule_atlas.py", "iso": 0.0,
           "unreached": {str(w): NOTES.get(w, "not fired by the search") for w in words},
           "rules": rules, "falls": falls,
           "grids": [{"shape": list(a.shape), "values": [int(x) for x in a.ravel()]} for a in cover]}
    with open(ac.RULE_ATLAS, "w") as f:
        f.write(json.dumps(doc, indent=None, separators=(",", ":"), sort_keys=True).replace('{"shape"', '\n{"shape"').replace('"iso"', '\n"iso"') + "\n")


if __name__ == "__main__":
    main()
