"""GPU tests of the sweep with a range table as it is scheduled: the verdicts k_tile_verdicts writes in front of the
sweep, the live list k_sweep goes by, the two plans - one for a sweep without a table, a finer one for a sweep with one - and the
lanes that are swept under one plan while the other comes into force.

Every surface is compared with the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit, as in
tests/test_gpu_range_skip.py, whose helpers and fields these tests use.  There is no tolerance in this file.

Shapes (points z, y, x): A = 48 x 200 x 520 (no grouped block), B = 40 x 70 x 1030 (a group of four segments and a fifth), and
BIG = 160 x 130 x 1030 (85 MB of float samples), which with MC33_HIP_SWEEP_BLOCKS_PER_CU=1 and tiles one plane deep is more blocks
than a device of up to 272 compute units holds at once, and on which the plan with a table (MC33_HIP_RZ_TABLE=1) differs from the one
without."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_range_skip as rs
from test_gpu_range_skip import A, B, STEEP_ISO, grid_of, numpy_table, reference, same, skipped, steep, table_of, to_device

pytestmark = pytest.mark.gpu

BIG = (160, 130, 1030)


@pytest.fixture(autouse=True)
def live_list_always(monkeypatch):
    """by itself a sweep goes by a live list only under a plan of at least one round of the device (test_who_gets_a_live_list); the
    grids of this file are small, and MC33_HIP_LIVE=1, read when a context is made, gives every sweep with a table one"""
    monkeypatch.setenv("MC33_HIP_LIVE", "1")


# ---- the plan and the live list, and numpy's own verdicts -------------------------------------------------------------------------------

def plan_of(g):
    """(tiles [n][4] = seg, yt, z_lo, z_hi in launch order, blocks the device holds at once, which plan: 0 without a table, 1 with)"""
    info = (C.c_ulonglong * 3)()
    assert g.lib.mc33hip_sweep_plan(g.ctx, None, 0, C.byref(info)) == 0
    t = np.zeros((int(info[0]), 4), np.uint32)
    assert g.lib.mc33hip_sweep_plan(g.ctx, C.c_void_p(t.ctypes.data), t.shape[0], C.byref(info)) == 0
    return t, int(info[1]), int(info[2])


def live_of(g):
    """(entries, count word, blocks of the plan) of the last sweep with a table"""
    info = (C.c_ulonglong * 2)()
    assert g.lib.mc33hip_sweep_live(g.ctx, None, 0, C.byref(info)) == 0
    e = np.zeros(max(int(info[1]), 1), np.uint32)
    assert g.lib.mc33hip_sweep_live(g.ctx, C.c_void_p(e.ctypes.data), e.shape[0], C.byref(info)) == 0
    return e[:int(info[0])], int(info[0]), int(info[1])


def numpy_verdicts(tiles, tab, isos, zs=0, plane0=0):
    """per tile: (dead for every isovalue, below the FIRST isovalue, above it) - the planes a tile would read are z_lo + 1 .. z_hi, and
    z_lo too in the lowest tile of a column; both comparisons strict"""
    dead, below, above = np.zeros(len(tiles), bool), np.zeros(len(tiles), bool), np.zeros(len(tiles), bool)
    for i, (seg, yt, z_lo, z_hi) in enumerate(tiles.tolist()):
        p0 = z_lo if z_lo == zs else z_lo + 1
        s = tab[p0 - plane0:z_hi + 1 - plane0, yt, seg]
        lo = [bool((s[:, 1] < iso).all()) for iso in isos]
        hi = [bool((s[:, 0] > iso).all()) for iso in isos]
        dead[i] = all(x or y for x, y in zip(lo, hi))
        below[i], above[i] = dead[i] and lo[0], dead[i] and hi[0] and not lo[0]
    return dead, below, above


def expected_live(dead):
    """the live list of a plan whose tiles have these verdicts: a word per block with a live tile, in plan order"""
    n = len(dead)
    out = []
    for b in range((n + 3) // 4):
        mask = sum(1 << k for k in range(4) if 4 * b + k >= n or dead[4 * b + k])
        if mask != 15:
            out.append(b << 4 | mask)
    return np.array(out, np.uint32)


def check_live(g, tab, isos, what, zs=0, plane0=0):
    tiles, resident, which = plan_of(g)
    dead, below, above = numpy_verdicts(tiles, tab, isos, zs, plane0)
    want = expected_live(dead)
    got, count, blocks = live_of(g)
    assert blocks == (len(tiles) + 3) // 4, what
    assert count == len(want) and np.array_equal(got, want), (what, "live list", count, len(want))
    return tiles, dead, below, above


# ---- 1. verdicts against numpy ------------------------------------------------------------------------------------------------------------

@pytest.fixture(params=[0, 1, 2, 16], ids=["default", "rz1", "rz2", "rz16"])
def depth(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("MC33_HIP_RZ", str(request.param))
        monkeypatch.setenv("MC33_HIP_MIN_DEPTH", str(request.param))
    return request.param


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
    assert np.array_equal(rs.words(table_of(g, "f32")), rs.words(tab))
    g.close()


# ---- 2. more blocks than the device holds ----------------------------------------------------------------------------------------------

def live_everywhere(shape):
    """every strip straddles 100.5 and few cells are cut: x mod 256 in the whole segments, 50 (x - 1024) in the narrow last one"""
    x = np.arange(shape[2])
    row = np.where(x < 1024, x % 256, 50 * (x - 1024)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(row, shape))


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


@pytest.fixture(params=[B, BIG], ids=["B", "BIG-two-plans"])
def switching(request, monkeypatch):
    """B as it comes; BIG with a device of one block per CU and a plan with a table of tiles one plane deep: the two plans differ"""
    if request.param == BIG:
        monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
        monkeypatch.setenv("MC33_HIP_RZ_TABLE", "1")
    return request.param


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
    with it kept - every count the same - then sweep_many over the slab and the emits"""
    import torch
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
        c = gg.count(iso, r)
        V = torch.empty((max(c.nV, 1), 3), dtype=torch.float32, device="cuda")
        N = torch.empty_like(V)
        T = torch.empty((max(c.nT, 1), 3), dtype=torch.int32, device="cuda")
        gg.emit_into(V, N, T, sum(p[3] for p in parts))
        torch.cuda.synchronize()
        parts.append((V[:c.nV].cpu().numpy(), N[:c.nV].cpu().numpy(), T[:c.nT].cpu().numpy().view(np.uint32), c.nV))
        gg.close()
    assert np.array_equal(np.concatenate([p[2] for p in parts]), ref.T)
    assert np.array_equal(rs.words(np.concatenate([p[0] for p in parts])), rs.words(ref.V))
    assert np.array_equal(rs.words(np.concatenate([p[1] for p in parts])), rs.words(ref.N))


# ---- 4. blocks with dead and live waves ------------------------------------------------------------------------------------------------

def mixed_field():
    """shape B, y tile 0: below 0.5 everywhere, but for one cell-sized bump per chosen (segment, plane) - planes 1 .. 12: segment 0
    only (three waves of the group of four dead), 14 .. 25: segments 0 and 2 (two), 27 .. 38: segments 0, 1 and 3 (one).  A block of
    the sweep is any four consecutive tiles of the plan, and with the fifth segment in between only every fourth z level's block is
    the group itself: every band is longer than that period at tiles two planes deep.  The bumps are 1.0, but for 3.0 in segment
    0, planes 4 .. 7 - the only thing above 2.5: every other tile with a bump is dead for 2.5 and live for 0.5."""
    data = np.zeros(B, np.float32)
    for planes, segs in ((range(1, 13), (0,)), (range(14, 26), (0, 2)), (range(27, 39), (0, 1, 3))):
        for p in planes:
            for s in segs:
                data[p, 20:24, 256 * s + 100:256 * s + 104] = 3.0 if (s == 0 and 4 <= p <= 7) else 1.0
    return data


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
    assert table_of(g, "f32") is not None and g.lib.mc33hip_sweep_live(g.ctx, None, 0, C.byref(info)) == rs.EINVAL
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
