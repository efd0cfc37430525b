"""CPU census of the case atlas (tests/atlas_cases.py): the committed witnesses provably reach every (sign index, pattern offset)
pair at every grid-face position and every reachable id-source rule of the vertices on grid points, and the host emulator of
the device's per-cell logic (tests/host_emu) equals the oracle bit for bit on every atlas grid.  These are conditions on the
INPUTS of tests/test_gpu_atlas.py, met by the oracle and the emulator alone: 100 %, no allowance."""
import os

import numpy as np
import pytest

import atlas_cases as ac
from parity import bits_equal

ATLAS = ac.load_row_atlas()
UNIVERSE = set(ac.pair_keys(ATLAS[0], ATLAS[1]).tolist())
RULES = ac.load_rule_atlas()


@pytest.fixture(scope="module")
def emus():
    from mc33_emu import Emu
    return {"f32": Emu("f32"), "u16": Emu("u16")}


def _same(a, b):
    return (a.nV, a.nT) == (b.nV, b.nT) and np.array_equal(a.T, b.T) and bits_equal(a.V, b.V) and bits_equal(a.N, b.N)


# ---- row atlas ----------------------------------------------------------------------------------------------------------------

def test_the_committed_universe():
    """766 pairs over 383 table rows, sorted, one witness each; the generator found the rarest pair 9 times in 4 000 000 cells"""
    index, pattern, cells, hits = ATLAS
    keys = ac.pair_keys(index, pattern)
    assert len(keys) == 766 and np.all(np.diff(keys) > 0) and len(set(pattern.tolist())) == 383
    assert cells.shape == (766, 2, 2, 2) and cells.dtype == np.float32 and np.abs(cells).max() <= 1.0
    assert hits.min() == 9


@pytest.mark.parametrize("dtype", ac.ROW_DTYPES)
def test_every_witness_has_its_pair_in_every_type(oracles, dtype):
    data, iso = ac.as_dtype(ATLAS[2], dtype)
    assert not np.any(data == iso)
    idx, pat = ac.classify_cells(oracles[dtype], data, iso)
    assert np.array_equal(idx, ATLAS[0]) and np.array_equal(pat, ATLAS[1])


def test_a_fresh_search_finds_no_pair_outside_the_universe(oracles):
    """300 000 uniform random cells of a seed the generator did not use"""
    idx, pat = ac.classify_cells(oracles["f32"], ac.random_cells(20240607, 300000), 0.0)
    active = (idx != 0) & (idx != 255)
    found = set(ac.pair_keys(idx[active], pat[active]).tolist())
    assert len(found) > 700 and found <= UNIVERSE, sorted(found - UNIVERSE)


@pytest.mark.parametrize("dtype", ac.ROW_DTYPES)
@pytest.mark.parametrize("flags", range(7))
def test_row_layout_reaches_every_pair_at_its_face_flags(oracles, flags, dtype):
    grid, pos = ac.row_layout(flags, ATLAS[2])
    data, iso = ac.as_dtype(grid, dtype)
    assert data.shape == {0: (21, 21, 17), 1: (57, 57, 2), 2: (57, 2, 57), 4: (2, 57, 57), 3: (1533, 2, 2), 5: (2, 1533, 2), 6: (2, 2, 1533)}[flags]
    assert not np.any(data == iso)
    assert np.all(ac.flags_of(data.shape)[tuple(pos.T)] == flags)
    reached = ac.pairs_at_flags(oracles[dtype], data, iso, flags)
    assert UNIVERSE <= reached, "flags %d %s: %d of %d pairs" % (flags, dtype, len(UNIVERSE & reached), len(UNIVERSE))
    idx, pat = oracles[dtype].classify(data, iso)  # ... each by its own witness, where the layout put it
    assert np.array_equal(idx[tuple(pos.T)], ATLAS[0]) and np.array_equal(pat[tuple(pos.T)], ATLAS[1])


@pytest.mark.parametrize("dtype", ac.ROW_DTYPES)
def test_corner_grids_reach_every_pair(oracles, dtype):
    """face flags 7: the one cell of a 2 x 2 x 2 grid, a grid per witness"""
    data, iso = ac.as_dtype(ATLAS[2], dtype)
    reached = set()
    for cell in data:
        idx, pat = oracles[dtype].classify(cell, iso)
        assert idx.shape == (1, 1, 1)
        reached |= set(ac.pair_keys(idx.ravel(), pat.ravel()).tolist())
    assert reached == UNIVERSE


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("flags", range(7))
def test_emulator_equals_oracle_on_row_layouts(emus, oracles, flags, dtype):
    data, iso = ac.as_dtype(ac.row_layout(flags, ATLAS[2])[0], dtype)
    got = emus[dtype].isosurface(data, iso)
    assert emus[dtype].violations == 0
    assert got.nT > 766 and _same(got, oracles[dtype].isosurface(data, iso))


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_emulator_equals_oracle_on_corner_grids(emus, oracles, dtype):
    data, iso = ac.as_dtype(ATLAS[2], dtype)
    for k, cell in enumerate(data):
        got = emus[dtype].isosurface(cell, iso)
        assert got.nT > 0 and _same(got, oracles[dtype].isosurface(cell, iso)), (k, int(ATLAS[0][k]), int(ATLAS[1][k]))


def test_face_records_of_every_witness_at_every_face_flags(emus):
    """766 witnesses x face flags 0..7 (tests/host_emu/emu.cpp, emu_check_atlas_records): the record k_cells makes from the pattern
    tables and the owned slots (make_face_entry) equals the generic plan's, and the device's own classification of each witness -
    tests on register-held values - is the oracle's pair."""
    import ctypes as C
    lib = emus["f32"].lib
    lib.emu_check_atlas_records.restype = C.c_long
    lib.emu_check_atlas_records.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    cells = np.ascontiguousarray(ATLAS[2], np.float32)
    idx, pat = np.zeros(len(cells), np.uint8), np.zeros(len(cells), np.uint16)
    n = lib.emu_check_atlas_records(cells.ctypes.data, len(cells), idx.ctypes.data, pat.ctypes.data)
    assert n == 8 * len(cells), "witness %d (sign index %d, pattern %d) at face flags %d" % (
        (-n - 1) // 8, ATLAS[0][(-n - 1) // 8], ATLAS[1][(-n - 1) // 8], (-n - 1) % 8)
    assert np.array_equal(idx, ATLAS[0]) and np.array_equal(pat, ATLAS[1])


# ---- rule atlas ---------------------------------------------------------------------------------------------------------------

def test_the_committed_rule_universe():
    """per face flags 0..7 the rules and fall-throughs the generator's search fired; word 50 alone fires nowhere (the fixture says why)"""
    rules, falls = RULES["rules"], RULES["falls"]
    assert [sum(r[0] == f for r in rules) for f in range(8)] == [16, 28, 27, 40, 24, 37, 35, 40]
    assert [sum(r[0] == f for r in falls) for f in range(8)] == [6, 10, 10, 16, 10, 16, 16, 24]
    assert sorted(set(range(81)) - set(r[1] for r in rules)) == [50] and list(RULES["unreached"]) == ["50"]
    assert all(np.prod(g["shape"]) <= 36 and len(g["values"]) == np.prod(g["shape"]) for g in RULES["grids"])
    assert all(0 in g["values"] and set(g["values"]) <= {-2, -1, 0, 1, 2} for g in RULES["grids"])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_rule_grids_fire_the_whole_universe(emus, oracles, dtype):
    """Through the hooked emulator the committed grids fire exactly the committed (face flags, rule word) and (face flags, edge,
    end point) sets; emulator, oracle and - where it is built - the unmodified reference agree bit for bit on each grid."""
    from mc33_capi import MC33Lib, ref_path
    ref = MC33Lib(ref_path(dtype), dtype) if os.path.exists(ref_path(dtype)) else None
    emu = emus[dtype]
    emu.rule_counts_reset()
    for k, g in enumerate(RULES["grids"]):
        data, iso = ac.rule_grid(g, dtype)
        assert np.any(data == iso)
        got, want = emu.isosurface(data, iso), oracles[dtype].isosurface(data, iso)
        assert _same(got, want), "rule grid %d: emulator and oracle differ" % k
        if ref is not None:
            assert _same(ref.isosurface(data, iso), want), "rule grid %d: oracle and reference differ" % k
    rules, falls = emu.rule_counts()
    assert sorted([int(f), int(r)] for f, r in zip(*np.nonzero(rules))) == RULES["rules"]
    assert sorted([int(f), int(e), int(k)] for f, e, k in zip(*np.nonzero(falls))) == RULES["falls"]
