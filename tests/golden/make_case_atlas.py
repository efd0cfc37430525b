#!/usr/bin/env python3
"""Regenerate tests/golden/case_atlas.npz: one witness cell per (sign index, pattern offset) pair that the oracle's
mc33o_classify reaches (tests/atlas_cases.py says what the atlas is for).  Nothing but the project's own oracle is used:

    make -C oracle oracle && python tests/golden/make_case_atlas.py

The universe is what a seeded search over SEARCH uniform random cells finds, united with the pairs the float fixtures of the GPU
suite reach.  Per pair the witness kept is the one whose smallest |sample| is largest among those that keep their pair as
float32, as float64 and as uint16 (rint(32768 + 30000 v) at isovalue 32768), so the cells survive quantisation.  Prints the
universe size, the hit count of the rarest pair, and the pattern starts pattern_offset_word can return by its structure next to
the ones reached."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import atlas_cases as ac  # noqa: E402
import fixtures as fx  # noqa: E402
from mc33_oracle import Oracle  # noqa: E402

SEARCH, CHUNK, SEED = 4_000_000, 500_000, 33


def fixture_cells():
    """every cell of the float fixtures of the GPU suite that have no sample equal to the isovalue, as samples minus isovalue"""
    grids = [(fx.noise_f32(32, s), 0.0) for s in (1, 2, 3, 7)]
    grids += [(fx.noise_f32(0, 11, shape=s), 0.05) for s in ((2, 2, 2), (2, 3, 5), (3, 2, 2), (9, 17, 33), (5, 70, 3), (4, 3, 600), (66, 65, 258))]
    f = fx.cos_field(120)[0].astype(np.float64) + np.random.default_rng(5).uniform(-0.35, 0.35, (120,) * 3)
    grids += [(f.astype(np.float32), 0.0), (f.astype(np.float32), -1.25)]
    rng = np.random.RandomState(2024)  # the float half of test_random_shapes_fuzz
    for case in range(40):
        kind = case % 4
        if kind == 0:
            shape = tuple(int(x) for x in rng.randint(2, 40, 3))
        elif kind == 1:
            shape = (int(rng.randint(2, 6)), int(rng.randint(2, 6)), int(rng.randint(250, 600)))
        elif kind == 2:
            shape = (int(rng.randint(60, 200)), int(rng.randint(2, 5)), int(rng.randint(2, 5)))
        else:
            shape = (int(rng.randint(2, 5)), int(rng.randint(60, 140)), int(rng.randint(2, 9)))
        seed = int(rng.randint(1, 1000))
        if case % 2:
            rng.randint(-1, 2)
        else:
            grids.append((fx.noise_f32(0, seed, shape=shape), 0.0))
    for nx, ny, nz in ((2, 2, 2), (3, 2, 5), (5, 9, 2), (17, 3, 4)):  # tests/test_gpu_face_records.py
        grids.append((np.random.default_rng(nx * 100 + ny * 10 + nz).standard_normal((nz, ny, nx)).astype(np.float32), 0.05))
    z, y, x = np.meshgrid(np.arange(17), np.arange(65), np.arange(33), indexing="ij")
    face = np.sin(0.61 * x + 0.3) + np.sin(0.37 * y + 1.1) + np.sin(0.83 * z + 0.7) + 0.05 * np.cos(0.29 * x * y / 7.0)
    grids.append((face.astype(np.float32), 0.1))
    for data, iso in grids:
        c = np.lib.stride_tricks.sliding_window_view(data - np.float32(iso), (2, 2, 2)).reshape(-1, 2, 2, 2)
        top = np.abs(c).reshape(len(c), 8).max(axis=1)
        c = c[(top > 0) & np.isfinite(top)]
        top = np.abs(c).reshape(len(c), 8).max(axis=1)
        # into [-1, 1] by a power of two: signs and the tests' comparisons are kept
        yield (c * np.exp2(-np.ceil(np.log2(np.maximum(top, 1.0)))).astype(np.float32)[:, None, None, None]).astype(np.float32)


def read_lut():
    """the words of mc33_lut (mc33_c_library_amd/csrc/mc33_lut_data.h)"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "mc33_c_library_amd", "csrc", "mc33_lut_data.h")).read()
    body = text[text.index("{", text.index("mc33_lut[")):]
    return [int(t, 0) for t in re.findall(r"0x[0-9A-Fa-f]+|\b\d+\b", body[:body.index("}")])]


def structural_starts():
    """{sign index: the pattern starts pattern_offset_word (mc33_cell.h) can return for its table word} for sign indices 1..254, by
    the function's structure alone: every branch of every group taken as possible."""
    lut = read_lut()
    out = {}
    for i in range(1, 255):
        c = lut[i ^ 0xFF if i & 0x80 else i]
        k, g = c & 0x7FF, c >> 12
        if g == 0:
            s = [k]
        elif g == 1:
            s = [183 + 2 * k, 159 + k]
        elif g == 2:
            s = [239 + 6 * k, 231 + 2 * k]
        elif g == 3:
            s = [575 + 5 * k, 407 + 7 * k, 335 + 3 * k]
        elif g == 4:
            s = [695 + 3 * k] + [b + 5 * k for b in (759, 799, 719)] + [b + 9 * k for b in (983, 839, 911)] + [1095 + 9 * k, 1055 + 5 * k]
        elif g == 5:
            s = [1213 + 8 * k, 1189 + 4 * k, 1261 + 8 * k, 1285 + 8 * k, 1237 + 8 * k, 1201 + 4 * k]
        elif g == 6:
            s = [1453 + 8 * k, 1357 + 4 * k, 1645 + 8 * k, 1741 + 8 * k, 1549 + 8 * k, 1405 + 4 * k]
        else:
            s = []  # case 13: all six faces are ambiguous, every vector of six face-test signs and every interior-test result
            for bits in range(64):
                f = [1 if (bits >> q) & 1 else -1 for q in range(6)]
                t = abs(sum(f))
                if t == 0:
                    kk = ((f[1] < 0) << 1) | (f[5] < 0)
                    s += [2157 + 12 * kk] if f[0] * f[1] == f[5] else [2285 + 6 * kk, 2285 + 10 * kk - 40, 2285 + 10 * kk - 80]
                elif t == 2:
                    s.append(1917 + 10 * (((f[2] > 0) if f[0] < 0 else 12 + (f[2] < 0)) + ((f[3] < 0) if f[1] < 0 else 6 + (f[3] > 0))) +
                             (30 if f[4] > 0 else 0))
                elif t == 4:
                    kk = 21 + 11 * f[0] + 4 * f[1] + 3 * f[2] + 2 * f[3] + f[4]
                    if kk >> 4:
                        kk -= 20 if kk & 32 else 10
                    s.append(1845 + 3 * kk)
                else:
                    s.append(1839 + 2 * f[0])
        out[i] = sorted(set(s))
    return out


def main():
    orcs = {d: Oracle(d) for d in ac.ROW_DTYPES}
    best = {}  # pair key -> (score, cell)
    hits = {}

    def take(cells, count):
        idx, pat = ac.classify_cells(orcs["f32"], cells, 0.0)
        key = ac.pair_keys(idx, pat)
        stable = np.ones(len(cells), bool)
        for d in ("f64", "u16"):
            data, iso = ac.as_dtype(cells, d)
            i2, p2 = ac.classify_cells(orcs[d], data, iso)
            stable &= ac.pair_keys(i2, p2) == key
        score = np.abs(cells).reshape(len(cells), 8).min(axis=1).astype(np.float64) + 10.0 * stable
        active = (idx != 0) & (idx != 255)
        order = np.lexsort((score, key))
        order = order[active[order]]
        last = np.r_[key[order][1:] != key[order][:-1], True]
        for k in order[last]:
            if key[k] not in best or score[k] > best[key[k]][0]:
                best[int(key[k])] = (float(score[k]), cells[k].copy())
        if count:
            u, c = np.unique(key[active], return_counts=True)
            for a, b in zip(u.tolist(), c.tolist()):
                hits[a] = hits.get(a, 0) + b

    for chunk in range(SEARCH // CHUNK):
        take(ac.random_cells(SEED + chunk, CHUNK), True)
    searched = set(best)
    for cells in fixture_cells():
        for at in range(0, len(cells), CHUNK):
            take(cells[at:at + CHUNK], False)
    keys = sorted(best)
    index = np.array([k // 4096 for k in keys], np.uint8)
    pattern = np.array([k % 4096 for k in keys], np.uint16)
    cells = np.stack([best[k][1] for k in keys]).astype(np.float32)
    nhits = np.array([hits.get(k, 0) for k in keys], np.int64)
    unstable = [k for k in keys if best[k][0] < 10.0]
    assert not unstable, "no witness keeps its pair in every type: %s" % unstable
    assert np.abs(cells).min() * ac.U16_AMP > 1.0  # no uint16 sample equals the isovalue
    np.savez_compressed(ac.ROW_ATLAS, index=index, pattern=pattern, cells=cells, hits=nhits)
    rows = set(pattern.tolist())
    print("universe: %d pairs, %d distinct rows (%d pairs from the random search of %d cells, %d more from the fixtures)" % (
        len(keys), len(rows), len(searched), SEARCH, len(keys) - len(searched)))
    rare = int(np.argmin(np.where(nhits > 0, nhits, nhits.max())))
    print("rarest pair of the search: index %d pattern %d, %d hits; smallest |sample| of a witness %.4g" % (
        index[rare], pattern[rare], nhits[rare], np.abs(cells).min()))
    by_index = structural_starts()
    pairs = set(i * 4096 + p for i, s in by_index.items() for p in s)
    print("pairs by structure: %d; reached: %d; structural but unreached: %s" % (
        len(pairs), len(keys), sorted((k // 4096, k % 4096) for k in pairs - set(keys))))
    st = set(p for s in by_index.values() for p in s)
    print("pattern starts by structure: %d; reached: %d; reached but not structural: %s" % (len(st), len(rows), sorted(rows - st)))
    print("structural but unreached: %s" % sorted(st - rows))


if __name__ == "__main__":
    main()
