"""GPU tests of the sweep with a range table as it is scheduled: the verdicts k_tile_verdicts writes in front of the
sweep, the live list k_sweep goes by, the two plans - one for a sweep without a table, a finer one for a sweep with one - and the
lanes that are swept under one plan while the other comes into force.

Every surface is compared with the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit, with the fields,
helpers and comparison of tests/sweep_harness.py.  There is no tolerance in this file.

Shapes (points z, y, x): A = 48 x 200 x 520 (no grouped block), B = 40 x 70 x 1030 (a group of four segments and a fifth), and
BIG = 160 x 130 x 1030 (85 MB of float samples), which with MC33_HIP_SWEEP_BLOCKS_PER_CU=1 and tiles one plane deep is more blocks
than a device of up to 272 compute units holds at once, and on which the plan with a table (MC33_HIP_RZ_TABLE=1) differs from the one
without."""
import ctypes as C

import numpy as np
import pytest

from sweep_harness import (A, B, BIG, EINVAL, STEEP_ISO, check_live, depth_fixture, emit_slab, grid_of, live_everywhere, live_list_always,  # noqa: F401
                           live_of, mixed_field, numpy_table, numpy_verdicts, plan_of, reference, same, skipped, slabs_are_the_surface, steep,
                           switching, table_of, to_device, words)   # (live_list_always, switching: the module's fixtures)

pytestmark = pytest.mark.gpu

depth = depth_fixture([0, 1, 2, 16], ids=["default", "rz1", "rz2", "rz16"])


# ---- 1. verdicts against numpy ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_verdicts_are_numpys(reflibs, depth, shape):
    data = steep(shape)
    iso = STEEP_ISO[shape]
    ref = reference(reflibs, ("steep", shape), "f32", data, iso)
    tab = numpy_table(data, "f32")
    g = grid_of(to_device(data))
    g.set_timing(1)
    same(g.extract(iso), ref, ("no table", depth))
    for rep in range(2):
        same(g.extract(iso), ref, ("table", depth, rep))
        tiles, dead, below, above = check_live(g, tab, (iso,), (shape, depth, rep))
        assert skipped(g) == (len(tiles), int(below.sum()), int(above.sum())), (shape, depth, rep)
        assert below.sum() > 0 and above.sum() > 0 and not dead.all()
    assert np.array_equal(words(table_of(g, "f32")), words(tab))
    g.close()


# ---- 2. more blocks than the device holds ----------------------------------------------------------------------------------------------

BIG_FIELDS = {"steep": (lambda: steep(BIG), 2600.5), "dead": (lambda: steep(BIG), 1e6), "live": (lambda: live_everywhere(BIG), 100.5)}


@pytest.mark.parametrize("field", ["steep", "dead", "live"])
def test_more_blocks_than_the_device_holds(reflibs, monkeypatch, field):
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("MC33_HIP_RZ", "1")
    monkeypatch.setenv("MC33_HIP_MIN_DEPTH", "1")
    make, iso = BIG_FIELDS[field]
    data = make()
    ref = reference(reflibs, ("steep", BIG) if field == "steep" else ("big", field), "f32", data, iso)
    tab = numpy_table(data, "f32")
    g = grid_of(to_device(data))
    g.set_timing(1)
    for rep in range(3):
        same(g.extract(iso), ref, (field, rep))
    tiles, resident, which = plan_of(g)
    assert (len(tiles) + 3) // 4 >= 1.5 * resident, (len(tiles), resident)
    tiles, dead, below, above = check_live(g, tab, (iso,), field)
    assert skipped(g) == (len(tiles), int(below.sum()), int(above.sum()))
    if field == "steep":
        assert ref.nV > 1000 and dead.any() and not dead.all()
    elif field == "dead":
        assert ref.nV == 0 and dead.all() and live_of(g)[1] == 0
    else:
        assert ref.nV > 1000 and not dead.any() and live_of(g)[1] == (len(tiles) + 3) // 4
    g.close()


# ---- 3. the plan changes while lanes are swept and not yet counted ----------------------------------------------------------------

EIGHT = {B: (1930.5, 1700.5, 2100.25, 1800.0, 1650.5, 2000.75, 1875.5, 2050.0),
         BIG: (2600.5, 2300.5, 2900.25, 2450.0, 2200.5, 2750.75, 2525.5, 2825.0)}


def test_plan_switch_under_swept_lanes(reflibs, switching):
    shape = switching
    data = steep(shape)
    isos = EIGHT[shape]
    refs = [reference(reflibs, ("steep", shape), "f32", data, iso) for iso in isos]
    assert all(r.nV > 500 for r in refs)
    t = to_device(data)
    for many in ("sweep_many", "prepare_many"):
        g = grid_of(t)
        getattr(g, many)(isos)           # two passes of four: the table is built in front of the second
        assert table_of(g, "f32") is not None
        n1 = len(plan_of(g)[0])
        for k in reversed(range(8)):     # lanes 7 .. 4 were swept with the table, 3 .. 0 without
            same(g.extract(isos[k]), refs[k], (many, shape, k))
        n0 = len(plan_of(g)[0])          # (sweep_many: the plan in force is now the one lane 0's tail went by; the tails of
        if shape == BIG and many == "sweep_many":  # prepare_many were made behind their passes, the second pass's last)
            assert n1 >= 1.5 * n0, (n0, n1)
        getattr(g, many)(isos)           # ... and once more, every pass with the table
        for k in (3, 6, 0, 5):
            same(g.extract(isos[k]), refs[k], (many, shape, "again", k))
        g.close()


def test_count_then_a_table_then_extract_into(reflibs, switching):
    import torch
    shape = switching
    data = steep(shape)
    isos = EIGHT[shape]
    refs = [reference(reflibs, ("steep", shape), "f32", data, iso) for iso in isos[:2]]
    g = grid_of(to_device(data))
    c0 = g.count(isos[0])                # sweep one: no table, the plan without
    assert (c0.nV, c0.nT) == (refs[0].nV, refs[0].nT)
    c1 = g.count(isos[1])                # sweep two builds the table and goes by the plan with it
    assert table_of(g, "f32") is not None and (c1.nV, c1.nT) == (refs[1].nV, refs[1].nT)
    for k in (0, 1, 0):
        V = torch.empty((refs[k].nV + 8, 3), dtype=torch.float32, device="cuda")
        N = torch.empty_like(V)
        T = torch.empty((refs[k].nT + 8, 3), dtype=torch.int32, device="cuda")
        c, ok = g.extract_into(isos[k], V, N, T)
        assert ok
        same((V[:c.nV], N[:c.nV], T[:c.nT], c), refs[k], ("extract_into", shape, k))
    g.close()


def test_sub_range_with_a_ghost_plane_across_the_switch(reflibs, switching):
    """the upper z-slab of the grid as a window with plane0 > 0 and a ghost slice: count without a table, with the table just built,
    with it kept - every count the same - then sweep_many over the slab and the emits.  (Not two_slab_case of the harness: the upper
    window is counted and checked before the lower one exists and stays open beside it, and each slab is swept for two isovalues
    twice in front of the one count its emit goes by.)"""
    from mc33_c_library_amd import DeviceGrid, Range
    shape = switching
    data = steep(shape)
    iso = EIGHT[shape][0]
    ref = reference(reflibs, ("steep", shape), "f32", data, iso)
    t = to_device(data)
    nz_total = shape[0] - 1
    zb = 17
    p_lo = zb - 2
    g = DeviceGrid(t[p_lo:], nz_total=nz_total, plane0=p_lo)
    rng = Range(zb, nz_total, 1, 0)
    cnts = [g.count(iso, rng) for rep in range(3)]
    assert len({(c.nV, c.nT) for c in cnts}) == 1
    tab = table_of(g, "f32")
    assert tab is not None
    check_live(g, tab, (iso,), ("slab", shape), zs=zb - 1, plane0=p_lo)
    lower = DeviceGrid(t[:zb + 2], nz_total=nz_total, plane0=0)
    parts = []
    for gg, r in ((lower, Range(0, zb, 0, 0)), (g, rng)):
        gg.sweep_many([iso, EIGHT[shape][1]], r)
        gg.sweep_many([iso, EIGHT[shape][1]], r)
        parts.append(emit_slab(gg, gg.count(iso, r), sum(p[3] for p in parts)))
        gg.close()
    slabs_are_the_surface(parts, ref)


# ---- 4. blocks with dead and live waves ------------------------------------------------------------------------------------------------

def test_mixed_blocks(reflibs, monkeypatch):
    monkeypatch.setenv("MC33_HIP_RZ", "2")
    monkeypatch.setenv("MC33_HIP_MIN_DEPTH", "2")
    data = mixed_field()
    tab = numpy_table(data, "f32")
    isos = (2.5, 0.5, 2.75, 0.25)   # (a tile with a bump of 1.0 and none of 3.0 is dead for the first and live for the second)
    refs = [reference(reflibs, "mixed", "f32", data, iso) for iso in isos]
    assert all(r.nV > 50 for r in refs)
    g = grid_of(to_device(data))
    g.set_timing(1)
    same(g.extract(0.5), refs[1], "no table")
    same(g.extract(0.5), refs[1], "table")
    tiles, dead, below, above = check_live(g, tab, (0.5,), "mixed")
    # the grouped blocks (y tile 0, segments 0 .. 3 over the same planes) and how many of their waves are dead
    ndead = set()
    for b in range(len(tiles) // 4):
        q = tiles[4 * b:4 * b + 4]
        if q[0, 1] == 0 and (q[:, 0] == np.arange(4)).all() and (q[:, 2] == q[0, 2]).all() and (q[:, 3] == q[0, 3]).all():
            ndead.add(int(dead[4 * b:4 * b + 4].sum()))
    assert {1, 2, 3} <= ndead, ndead
    for ni in (2, 4):
        g.sweep_many(isos[:ni])
        tiles, dead, _, _ = check_live(g, tab, isos[:ni], ("mixed", ni))
        one = numpy_verdicts(tiles, tab, isos[:1])[0]
        assert (one & ~dead).any()      # a tile dead for the first isovalue and live for another of the pass
        for k in reversed(range(ni)):
            same(g.extract(isos[k]), refs[k], ("mixed", ni, k))
    g.close()


# ---- 5. the per-tile buffers follow the plan ---------------------------------------------------------------------------------------------

def test_buffers_follow_the_plan(reflibs, monkeypatch):
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("MC33_HIP_RZ_TABLE", "1")
    data = steep(BIG).copy()
    iso = EIGHT[BIG][0]
    ref = reference(reflibs, ("steep", BIG), "f32", data, iso)
    t = to_device(data)
    g = grid_of(t)
    sizes = []
    for what in ("coarse", "fine", "fine kept"):
        same(g.extract(iso), ref, what)
        sizes.append((len(plan_of(g)[0]), plan_of(g)[2]))
    t.data[80, 5, 5] = 9000.0  # (inside a tile the table leaves out: a stale table would miss the new surface)
    data[80, 5, 5] = 9000.0
    g.changed()
    ref2 = reflibs["f32"].isosurface(data, iso)
    assert ref2.nV > ref.nV
    for what in ("coarse after changed()", "fine again"):
        same(g.extract(iso), ref2, what)
        sizes.append((len(plan_of(g)[0]), plan_of(g)[2]))
    assert [w for _, w in sizes] == [0, 1, 1, 0, 1], sizes
    assert sizes[1][0] >= 1.5 * sizes[0][0] and sizes[3] == sizes[0] and sizes[4] == sizes[1], sizes
    g.close()


# ---- 6. who gets a live list when nobody says ----------------------------------------------------------------------------------------------

def test_who_gets_a_live_list(reflibs, monkeypatch):
    """a plan of less than one round of the device: the verdicts stay in k_sweep, there is no list; one round and more: the list"""
    monkeypatch.delenv("MC33_HIP_LIVE")
    data = steep(B)
    ref = reference(reflibs, ("steep", B), "f32", data, STEEP_ISO[B])
    g = grid_of(to_device(data))
    g.set_timing(1)
    for rep in range(3):
        same(g.extract(STEEP_ISO[B]), ref, ("B", rep))
    info = (C.c_ulonglong * 2)()
    assert table_of(g, "f32") is not None and g.lib.mc33hip_sweep_live(g.ctx, None, 0, C.byref(info)) == EINVAL
    tiles, resident, which = plan_of(g)
    assert len(tiles) < 4 * resident
    dead, below, above = numpy_verdicts(tiles, numpy_table(data, "f32"), (STEEP_ISO[B],))
    assert skipped(g) == (len(tiles), int(below.sum()), int(above.sum()))
    g.close()
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("MC33_HIP_RZ_TABLE", "1")
    data = steep(BIG)
    iso = EIGHT[BIG][0]
    ref = reference(reflibs, ("steep", BIG), "f32", data, iso)
    g = grid_of(to_device(data))
    for rep in range(3):
        same(g.extract(iso), ref, ("BIG", rep))
    tiles, resident, which = plan_of(g)
    assert which == 1 and len(tiles) >= 4 * resident
    check_live(g, numpy_table(data, "f32"), (iso,), "BIG by itself")
    g.close()


# ---- 7. a sweep that leaves little out sends the next ones back to the one-round plan ---------------------------------------------------

def test_fall_back_when_little_is_left_out(reflibs, monkeypatch):
    """BIG with two different plans; every tile live at 100.5: the sweep by the finer plan finds all its blocks live (> 90 %) and the
    following ones go by plan 0, with the table and its list; every tile dead at 1e6: the first sweep by plan 0 that finds fewer
    than 75 % live sends the following ones to the finer plan again.  changed() starts over from the finer plan."""
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("MC33_HIP_RZ_TABLE", "1")
    data = live_everywhere(BIG)
    tab = numpy_table(data, "f32")
    ref = reference(reflibs, ("big", "live"), "f32", data, 100.5)
    g = grid_of(to_device(data))
    which = []
    for rep in range(5):
        same(g.extract(100.5), ref, ("live everywhere", rep))
        which.append(plan_of(g)[2])
        if rep:
            check_live(g, tab, (100.5,), ("live everywhere", rep))
    assert which == [0, 1, 0, 0, 0], which
    for rep in range(3):
        V, N, T, cnt = g.extract(1e6)
        assert (cnt.nV, cnt.nT) == (0, 0)
        which.append(plan_of(g)[2])
        assert live_of(g)[1] == 0
    assert which[5:] == [0, 1, 1], which
    same(g.extract(100.5), ref, "live again, by the finer plan")   # (its count sends the next one back)
    same(g.extract(100.5), ref, "live again, by plan 0")
    assert plan_of(g)[2] == 0
    g.changed()
    for rep in range(2):
        same(g.extract(100.5), ref, ("after changed()", rep))
    assert plan_of(g)[2] == 1
    g.close()
