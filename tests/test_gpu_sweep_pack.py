"""GPU tests of the packed live list and of the plan sized by the live count: the list k_live_compact packs for
k_sweep_live against a numpy restatement of its order rule, the surfaces of packed blocks, the size of the plan, and lanes swept
under one size of plan while another comes into force.

Every surface is compared with the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit, with the fields,
helpers and comparison of tests/sweep_harness.py.  There is no tolerance in this file.

Shapes (points z, y, x): A = 48 x 200 x 520 (no grouped block), B = 40 x 70 x 1030 (a group of four segments and a fifth), and
BIG = 160 x 130 x 1030 with MC33_HIP_SWEEP_BLOCKS_PER_CU=1, whose plan is one round of a device of 256 compute units at its
default size and which can have more packed blocks than such a device holds."""
import numpy as np
import pytest

import sweep_pack_rules as pr
from sweep_harness import (A, B, BIG, HIGH, LOW, MANY, STEEP_ISO, banded, by_the_rule, check_packed, grid_of, live_everywhere,  # noqa: F401
                           live_list_always, mixed_field, mixed_whole, numpy_table, numpy_verdicts, one_bump, packed_of, plan_of, ramp,
                           reference, same, steep, table_of, to_device, two_slab_case, typed_ramp)   # (live_list_always: the module's fixture)

pytestmark = pytest.mark.gpu

# ---- 1. the packed list against numpy ---------------------------------------------------------------------------------------------------

LIST_CASES = {
    "steep A": (lambda: steep(A), STEEP_ISO[A], ("steep", A), 0),
    "steep B": (lambda: steep(B), STEEP_ISO[B], ("steep", B), 0),
    "mixed": (mixed_whole, 0.5, ("pack", "mixed whole"), 2),
    "all dead": (lambda: steep(B), 1e6, None, 2),
    "all live": (lambda: live_everywhere(B), 100.5, ("pack", "live B"), 2),
    "one live tile": (one_bump, 0.5, ("pack", "bump"), 2),
}


@pytest.mark.parametrize("case", list(LIST_CASES))
def test_packed_list_is_numpys(reflibs, monkeypatch, case):
    make, iso, key, rz = LIST_CASES[case]
    if rz:
        monkeypatch.setenv("MC33_HIP_RZ", str(rz))
        monkeypatch.setenv("MC33_HIP_MIN_DEPTH", str(rz))
    data = make()
    ref = reference(reflibs, key, "f32", data, iso) if key else None
    tab = numpy_table(data, "f32")
    g = grid_of(to_device(data))
    for rep in range(3):
        got = g.extract(iso)
        if ref is not None:
            same(got, ref, (case, rep))
        else:
            assert (got[3].nV, got[3].nT) == (0, 0)
    tiles, dead, grouped, e = check_packed(g, tab, (iso,), case)
    whole = (e[:, 0] & pr.GROUP) != 0 if len(e) else np.zeros(0, bool)
    if case == "all dead":
        assert dead.all() and len(e) == 0
    elif case == "all live":
        assert not dead.any() and grouped.any() and not grouped.all()
        # every entry is a block of the plan, and a whole group exactly where the plan grouped it
        full = len(tiles) // 4
        assert np.array_equal(e[:full, 0] & ~np.uint32(pr.GROUP), 4 * np.arange(full, dtype=np.uint32)) and np.array_equal(whole[:full], grouped[:full])
    elif case == "one live tile":
        assert int((~dead).sum()) == 1 and e.shape == (1, 4) and (e[0, 1:] == pr.NONE).all()
    elif case == "mixed":
        nd = {int(dead[4 * b:4 * b + 4].sum()) for b in np.flatnonzero(grouped)}
        assert {0, 1, 2, 3} <= nd, nd   # whole, 1-, 2- and 3-dead blocks
        assert whole.any() and not whole.all()
    else:
        assert dead.any() and not dead.all()
    if case == "steep A":
        assert not grouped.any() and not whole.any()
    if case in ("steep A", "steep B") and int((~dead).sum()) % 4 == 0:   # a live count that is no multiple of four
        iso2 = iso
        for iso2 in (iso + 37.0, iso - 61.0, iso + 113.0, iso - 171.0):
            g.extract(iso2)
            if packed_of(g)[1] % 4:
                break
        tiles, dead, grouped, e = check_packed(g, tab, (iso2,), (case, iso2))
    if case in ("steep A", "steep B"):
        assert int((~dead).sum()) % 4 != 0 and (e == pr.NONE).any()
    g.close()


# ---- 2. packed blocks over the same samples as the table-less sweep ------------------------------------------------------------------

FOUR = {A: MANY[("f32", A)], B: MANY[("f32", B)], BIG: LOW[:4]}


@pytest.mark.parametrize("ni", [1, 2, 4])
@pytest.mark.parametrize("shape", [A, B, BIG], ids=["A", "B", "BIG"])
def test_packed_blocks_give_the_reference(reflibs, monkeypatch, shape, ni):
    if shape == BIG:
        monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
        monkeypatch.setenv("MC33_HIP_TABLE_TILES", "100000")   # (as fine as the grid allows: tiles one plane deep)
    data = banded() if shape == BIG else steep(shape)
    isos = FOUR[shape][:ni]
    refs = [reference(reflibs, ("pack", "banded") if shape == BIG else ("many", shape), "f32", data, iso) for iso in isos]
    tab = numpy_table(data, "f32")
    t = to_device(data)
    g = grid_of(t)
    for rep in range(3):   # (the second pass over the grid builds the table)
        g.sweep_many(isos)
        if rep:
            tiles, dead, grouped, e = check_packed(g, tab, isos, (shape, ni, rep))
        for k in reversed(range(ni)):
            same(g.extract(isos[k]), refs[k], (shape, ni, rep, k))
    resident = plan_of(g)[1]
    if shape == BIG:
        assert len(e) > resident, (len(e), resident)   # more packed blocks than the device holds
    if shape == B:
        assert grouped.any() and (tiles[:, 0] == 4).any()   # a group, and the fifth segment
    g.close()
    monkeypatch.setenv("MC33_HIP_RANGES", "0")
    g = grid_of(t)
    g.sweep_many(isos)
    for k in range(ni):
        same(g.extract(isos[k]), refs[k], (shape, ni, "MC33_HIP_RANGES=0", k))
    assert table_of(g, "f32") is None
    g.close()


@pytest.mark.parametrize("dtype", ["u16", "u8"])
def test_narrow_samples_on_b(reflibs, dtype):
    data = typed_ramp("u16", B) if dtype == "u16" else (ramp(B) // 6).astype(np.uint8)
    isos = MANY[("u16", B)] if dtype == "u16" else (100.5, 90.5, 120.5, 107.0)
    refs = [reference(reflibs, ("pack", "narrow B"), dtype, data, iso) for iso in isos]
    assert all(r.nV > 200 for r in refs)
    tab = numpy_table(data, dtype)
    g = grid_of(to_device(data))
    for ni in (1, 1, 2, 4):
        g.sweep_many(isos[:ni])
        for k in reversed(range(ni)):
            same(g.extract(isos[k]), refs[k], (dtype, ni, k))
    g.sweep_many(isos)
    tiles, dead, grouped, e = check_packed(g, tab, isos, dtype)
    g.extract(isos[0] + 1.0)             # (an isovalue no lane holds: a sweep of its own)
    tiles, dead, grouped, e = check_packed(g, tab, (isos[0] + 1.0,), (dtype, "one"))
    assert dead.any() and not dead.all()
    g.close()


def test_a_strip_with_a_nan(reflibs):
    data = steep(A).copy()
    iso = STEEP_ISO[A]
    data[5, 10, 17] = np.nan       # in strips that lie wholly below / above the isovalue: their tiles are live all the same
    data[12, 150, 519] = np.nan
    data[12, 189, 512] = np.nan    # the shared row and the halo column of its neighbours
    ref = reference(reflibs, ("pack", "nan"), "f32", data, iso)
    tab = numpy_table(data, "f32")
    clean = numpy_table(steep(A), "f32")
    g = grid_of(to_device(data))
    for rep in range(3):
        same(g.extract(iso), ref, ("nan", rep))
    tiles, dead, grouped, e = check_packed(g, tab, (iso,), "nan")
    assert (~dead & numpy_verdicts(tiles, clean, (iso,))[0]).any()   # a tile that is live by its NaN alone
    g.close()


def test_sub_range_with_a_ghost_plane(reflibs):
    """the upper z-slab of B as a window with plane0 > 0 and a ghost slice; the two slabs together are the whole surface"""
    def the_list_is_numpys(g, window, lo_plane, zs, cnts):
        check_packed(g, table_of(g, "f32"), (STEEP_ISO[B],), ("slab", lo_plane), zs=zs, plane0=lo_plane)
    two_slab_case(reflibs, the_list_is_numpys)


# ---- 3. the size of the plan ---------------------------------------------------------------------------------------------------------------

def test_plan_is_sized_by_the_live_count(reflibs, monkeypatch):
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    data = banded(96)   # (0.6 of the tiles live, then 0.4: a size inside the band, then the finest the grid allows)
    refs = {iso: reference(reflibs, ("pack", "banded 96"), "f32", data, iso) for iso in (LOW[0], HIGH)}
    assert all(r.nV > 1000 for r in refs.values())
    g = grid_of(to_device(data))
    sizes = []
    for iso in (LOW[0], HIGH, LOW[0]):
        for rep in range(6):   # (a count is published by one call, asks for a size in the next, and is obeyed when the one after agrees)
            same(g.extract(iso), refs[iso], ("sizing", iso, rep))
        sizes.append(by_the_rule(g, ("sizing", iso)))
        same(g.extract(iso), refs[iso], ("sizing", iso, "kept"))
        assert len(plan_of(g)[0]) == sizes[-1], "a plan inside its band was replaced"
    assert sizes[1] >= 1.2 * sizes[0] and abs(sizes[2] - sizes[0]) <= 0.1 * sizes[0], sizes   # fewer tiles live: a finer plan, and back
    assert pr.keeps(packed_of(g)[1], plan_of(g)[1]), "0.6 of the tiles live: the packed blocks lie inside the band"
    g.close()


def test_a_large_live_share_keeps_its_list_and_is_sized_again(reflibs, monkeypatch):
    """with nobody forcing a list (MC33_HIP_LIVE not set): four tiles in five live would ask for less than one round, and a plan
    of less than one round goes without a list - no count would ever be published again.  The plan stays one round, keeps its
    list, and moves when the isovalue moves to one with one tile in five live."""
    monkeypatch.delenv("MC33_HIP_LIVE")
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    data = banded(128)
    refs = {iso: reference(reflibs, ("pack", "banded 128"), "f32", data, iso) for iso in (LOW[0], HIGH)}
    g = grid_of(to_device(data))
    for rep in range(6):
        same(g.extract(LOW[0]), refs[LOW[0]], ("large share", rep))
    tiles, resident, which = plan_of(g)
    e, live, ntiles = packed_of(g)       # (there is a list)
    assert which == 1 and ntiles == len(tiles) >= 4 * resident and 0.72 * ntiles < live < 0.9 * ntiles, (ntiles, live, resident)
    assert pr.target(live, ntiles, resident, pr.unit_of(BIG), 1.0) == 4 * resident
    n_large = by_the_rule(g, "large share")
    for rep in range(6):
        same(g.extract(HIGH), refs[HIGH], ("small share", rep))
    n_small = by_the_rule(g, "small share")
    assert n_small >= 1.2 * n_large, (n_large, n_small)
    g.close()


def test_table_tiles_is_obeyed_and_a_depth_switches_sizing_off(reflibs, monkeypatch):
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    data = banded()
    refs = {iso: reference(reflibs, ("pack", "banded"), "f32", data, iso) for iso in (LOW[0], HIGH)}
    t = to_device(data)
    for asked in (700, 1300):
        monkeypatch.setenv("MC33_HIP_TABLE_TILES", str(asked))
        g = grid_of(t)
        for iso in (LOW[0], LOW[0], HIGH, HIGH, LOW[0]):
            same(g.extract(iso), refs[iso], ("MC33_HIP_TABLE_TILES", asked, iso))
        tiles, resident, which = plan_of(g)
        assert which == 1 and abs(len(tiles) - asked) <= 8, (asked, len(tiles))
        g.close()
    monkeypatch.delenv("MC33_HIP_TABLE_TILES")
    monkeypatch.setenv("MC33_HIP_RZ_TABLE", "2")
    g = grid_of(t)
    sizes = set()
    for iso in (LOW[0], LOW[0], LOW[0], LOW[0], HIGH, HIGH, HIGH, LOW[0]):
        same(g.extract(iso), refs[iso], ("MC33_HIP_RZ_TABLE", iso))
        if plan_of(g)[2] == 1:
            sizes.add(len(plan_of(g)[0]))
    assert len(sizes) == 1, sizes
    g.close()


# ---- 4. a re-target under swept lanes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("many", ["sweep_many", "prepare_many"])
def test_retarget_under_swept_lanes(reflibs, monkeypatch, many):
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    data = banded(96)
    refs = [reference(reflibs, ("pack", "banded 96"), "f32", data, iso) for iso in LOW]
    ref_high = reference(reflibs, ("pack", "banded 96"), "f32", data, HIGH)
    g = grid_of(to_device(data))
    getattr(g, many)(LOW)                # two passes of four: the table is built in front of the second, which goes by the default plan
    assert table_of(g, "f32") is not None
    n1 = len(plan_of(g)[0])
    for rep in range(4):                 # 0.6 of the tiles live, then 0.4: the plan is sized, and sized again
        same(g.extract(LOW[0] + 1.0), reference(reflibs, ("pack", "banded 96"), "f32", data, LOW[0] + 1.0), (many, "re-target", rep))
    n2 = len(plan_of(g)[0])
    for rep in range(4):
        same(g.extract(HIGH), ref_high, (many, "re-target again", rep))
    n3 = len(plan_of(g)[0])
    assert n2 != n1 and n3 != n2 and plan_of(g)[2] == 1, (n1, n2, n3)
    for k in reversed(range(8)):         # lanes 7 .. 4 were swept by the default plan with the table, 3 .. 1 without; lane 0 is swept again
        same(g.extract(LOW[k]), refs[k], (many, k))
    g.close()


# ---- 5. the places of the quads in memory ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", ["mixed", "steep B"])
def test_quad_places_behind_the_entries(reflibs, monkeypatch, field):
    """k_live_compact keeps the places of the quads in LDS for plans of up to 4 096 blocks and in memory behind the entries for larger
    ones; MC33_HIP_LIST_LDS=0 sends these small plans the second way"""
    monkeypatch.setenv("MC33_HIP_LIST_LDS", "0")
    make, iso, key, rz = LIST_CASES[field]
    if rz:
        monkeypatch.setenv("MC33_HIP_RZ", str(rz))
        monkeypatch.setenv("MC33_HIP_MIN_DEPTH", str(rz))
    data = make()
    ref = reference(reflibs, key, "f32", data, iso)
    g = grid_of(to_device(data))
    for rep in range(3):
        same(g.extract(iso), ref, (field, "quad places in memory", rep))
    tiles, dead, grouped, e = check_packed(g, numpy_table(data, "f32"), (iso,), (field, "quad places in memory"))
    assert dead.any() and not dead.all() and len(e) > 4
    g.close()


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_leaves_the_same_bytes(reflibs):
    data = mixed_field()
    g = grid_of(to_device(data))
    g.extract(0.5)
    g.extract(0.5)
    runs = []
    for rep in range(2):
        V, N, T, cnt = g.extract(0.5)
        e, live, ntiles = packed_of(g)
        runs.append((e.tobytes(), live, ntiles, V.cpu().numpy().tobytes(), N.cpu().numpy().tobytes(), T.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] and runs[0][1] > 0
    same(g.extract(0.5), reference(reflibs, "mixed", "f32", data, 0.5), "mixed")
    g.close()
