"""GPU tests of the sweep's range table (include/mc33_hip.h: mc33hip_grid_stable): k_ranges, the tiles k_sweep leaves
out, and who has to say what when samples change.

Every surface is compared with the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit: counts, T as uint32,
V and N by bit pattern (a NaN must be a NaN in the same place).  There is no tolerance in this file.  The one exception is the isovalue -0.0 on a grid that holds zeros,
where the reference is not a function of its input: that surface is compared with the one a context without a table
(MC33_HIP_RANGES=0) gives.

Shapes (points z, y, x): A = 48 x 200 x 520 - three row segments, the last one 8 cells wide, so no block of the sweep is grouped;
four y tiles, the last of 11 sample rows.  B = 40 x 70 x 1030 - a whole group of four segments and a fifth; a second y tile of 7
rows.  Both with tiles 1, 2 and 16 planes deep (MC33_HIP_RZ / MC33_HIP_MIN_DEPTH, read when a context is made).
Each case extracts three times - without a table, with the table just built, with the table kept - and once more in a context
that never builds one.  Fields, helpers and the comparison are those of tests/sweep_harness.py."""
import ctypes as C

import numpy as np
import pytest

from sweep_harness import (A, B, DEPTHS, MANY, NP, STEEP_ISO, dead_columns, depth_fixture, four_runs, grid_of, numpy_table, planned_tiles, ramp,
                           ramp_isos, reference, same, same_arrays, skipped, steep, table_of, to_device, two_slab_case, typed_ramp, words)

pytestmark = pytest.mark.gpu

depth = depth_fixture(DEPTHS)   # (no live_list_always here: these tests run without MC33_HIP_LIVE)


# ---- integer-valued ramps, isovalues on the strips' own ends ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_float_ramp(reflibs, monkeypatch, depth, shape):
    data = typed_ramp("f32", shape)
    isos = ramp_isos("f32", data)
    refs = [reference(reflibs, ("ramp", shape), "f32", data, iso) for iso in isos]
    assert all(r.nV > 1000 for r in refs)
    t = to_device(data)
    four_runs(monkeypatch, lambda: grid_of(t), isos, refs, "f32", data, ("f32", shape, depth))


@pytest.mark.parametrize("dtype", ["u8", "u16", "u32", "f64"])
def test_typed_ramp(reflibs, monkeypatch, depth, dtype):
    data = typed_ramp(dtype, A)
    isos = ramp_isos(dtype, data)
    refs = [reference(reflibs, "ramp", dtype, data, iso) for iso in isos]
    assert all(r.nV > 1000 for r in refs)
    t = to_device(data)
    four_runs(monkeypatch, lambda: grid_of(t), isos, refs, dtype, data, (dtype, depth))


def test_either_zero_on_a_ramp_through_zero(reflibs, monkeypatch, depth):
    data = ramp(A, off=-500).astype(np.float32)
    assert (data == 0).sum() > 1000
    ref = reference(reflibs, "zero", "f32", data, 0.0)
    t = to_device(data)
    four_runs(monkeypatch, lambda: grid_of(t), (0.0,), (ref,), "f32", data, ("+0.0", depth))
    monkeypatch.setenv("MC33_HIP_RANGES", "0")
    plain = grid_of(t)
    want = plain.extract(-0.0)
    monkeypatch.delenv("MC33_HIP_RANGES")
    g = grid_of(t)
    for rep in range(3):
        same_arrays(g.extract(-0.0), want, ("-0.0", depth, rep))
        same(g.extract(0.0), ref, ("+0.0 between", depth, rep))
    assert table_of(g, "f32") is not None
    g.close(); plain.close()


# ---- a steep ramp: whole columns of tiles on one side ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_skipping_really_happens(reflibs, depth, shape):
    data = steep(shape)
    iso = STEEP_ISO[shape]
    nb, na, ncol = dead_columns(data, iso)
    assert 4 * nb >= ncol and 4 * na >= ncol, (nb, na, ncol)  # a quarter of the columns on each side
    ref = reference(reflibs, ("steep", shape), "f32", data, iso)
    assert ref.nV > 1000
    plan = planned_tiles(shape, depth)
    tab = numpy_table(data, "f32")
    col_below, col_above = (tab[..., 1] < iso).all(axis=0), (tab[..., 0] > iso).all(axis=0)
    tb = sum(n for (yt, seg), n in plan.items() if col_below[yt, seg])
    ta = sum(n for (yt, seg), n in plan.items() if col_above[yt, seg])
    assert tb >= nb and ta >= na and (depth > 2 or (tb >= 4 * nb and ta >= 4 * na)), (tb, ta)  # (shallow tiles: many per column)
    g = grid_of(to_device(data))
    g.set_timing(1)
    same(g.extract(iso), ref, "no table")
    assert skipped(g)[1:] == (0, 0)
    for rep in range(2):
        same(g.extract(iso), ref, ("table", rep))
        tiles, below, above = skipped(g)
        print("depth %d: %d tiles, %d left out below, %d above (%d + %d of %d columns dead)" % (depth, tiles, below, above, nb, na, ncol))
        # all tiles of a dead column are dead: at least the tiles plan_sweep gives those columns before it deals out its remainder
        assert tiles >= sum(plan.values())
        assert below >= tb and above >= ta and below + above < tiles, (below, tb, above, ta, tiles)
    # every strip straddles the isovalue: x runs through the whole range in every row
    wavy = np.broadcast_to((np.arange(shape[2]) % 2).astype(np.float32), shape).copy()
    g2 = grid_of(to_device(wavy))
    g2.set_timing(1)
    for rep in range(3):
        same(g2.extract(0.5), reference(reflibs, ("wavy", shape), "f32", wavy, 0.5), ("wavy", rep))
    assert table_of(g2, "f32") is not None and skipped(g2)[1:] == (0, 0)
    # the whole grid on one side: every tile left out, an empty surface
    for iso1, side in ((1e6, 1), (-1.0, 2)):
        for rep in range(2):
            V, N, T, cnt = g.extract(iso1)
            assert (cnt.nV, cnt.nT) == (0, 0) and V.shape[0] == 0 and T.shape[0] == 0
        s = skipped(g)
        assert s[side] == s[0] and s[3 - side] == 0, s
    g.close(); g2.close()


def test_nan_and_infinities_in_dead_strips(reflibs, monkeypatch, depth):
    data = steep(A).copy()
    iso = STEEP_ISO[A]
    t0 = numpy_table(data, "f32")
    # (plane, row, column) in strips that lie wholly below / above the isovalue
    assert t0[5, 0, 0, 1] < iso and t0[30, 1, 0, 1] < iso and t0[40, 3, 2, 0] > iso and t0[12, 2, 2, 0] > iso
    data[5, 10, 17] = np.nan
    data[30, 100, 200] = np.inf
    data[40, 195, 515] = -np.inf
    data[12, 150, 519] = np.nan
    data[12, 189, 512] = np.nan   # the shared row and the halo column of its neighbours
    ref = reference(reflibs, "nan", "f32", data, iso)
    t = to_device(data)
    four_runs(monkeypatch, lambda: grid_of(t), (iso,), (ref,), "f32", data, ("nan", depth))
    tab = numpy_table(data, "f32")
    assert tuple(tab[5, 0, 0]) == (-np.inf, np.inf) and tab[30, 1, 0, 1] == np.inf and tab[40, 3, 2, 0] == -np.inf
    assert tuple(tab[12, 2, 1]) == (-np.inf, np.inf) and tuple(tab[12, 3, 2]) == (-np.inf, np.inf)


# ---- several isovalues per pass: dead for one, live for another ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,shape", [("f32", A), ("u8", A), ("u16", A), ("f32", B), ("u16", B)], ids=["f32-A", "u8-A", "u16-A", "f32-B", "u16-B"])
def test_several_isovalues_per_pass(reflibs, monkeypatch, depth, dtype, shape):
    data = steep(shape) if dtype == "f32" else typed_ramp(dtype, shape)
    isos = MANY[(dtype, shape)]
    refs = [reference(reflibs, ("many", shape), dtype, data, iso) for iso in isos]
    tab = numpy_table(data, dtype)
    dead = [((tab[..., 1] < iso) | (tab[..., 0] > iso)) for iso in isos]
    assert all(r.nV > 500 for r in refs)
    if shape == A:
        assert (dead[0] & ~dead[1]).any() and (dead[1] & ~dead[0]).any()
    else:  # a grouped block with dead and live tiles, for the pair and for the four
        for n in (2, 4):
            col = np.all([(tab[..., 1] < iso).all(axis=0) | (tab[..., 0] > iso).all(axis=0) for iso in isos[:n]], axis=0)
            assert col[0, :4].any() and (~col[0, :4]).any() and not col[0, 1], col

    def rounds(g, reps, what):
        for rep in range(reps):  # (the second pass over the grid builds the table)
            g.sweep_many(isos[:2])
            for k in (1, 0):
                same(g.extract(isos[k]), refs[k], (dtype, depth, what, "pair", rep, isos[k]))
            g.prepare_many(isos)
            for k in (3, 0, 2, 1):
                same(g.extract(isos[k]), refs[k], (dtype, depth, what, "four", rep, isos[k]))
    t = to_device(data)
    g = grid_of(t)
    rounds(g, 3, "table")
    assert table_of(g, dtype) is not None
    g.close()
    monkeypatch.setenv("MC33_HIP_RANGES", "0")
    g = grid_of(t)
    rounds(g, 1, "MC33_HIP_RANGES=0")
    assert table_of(g, dtype) is None
    g.close()
    monkeypatch.delenv("MC33_HIP_RANGES")


# ---- ranges and slabs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_sub_range_with_a_ghost_plane_and_a_slab_above_plane_zero(reflibs, depth, shape):
    """two z-slabs as windows of one tensor: the upper one with plane0 > 0 and a ghost slice below its range"""
    def the_table_is_numpys(g, window, lo_plane, zs, cnts):
        tab = table_of(g, "f32")
        assert tab is not None and np.array_equal(words(tab), words(numpy_table(window, "f32")))
    two_slab_case(reflibs, the_table_is_numpys, shape)


@pytest.mark.parametrize("dtype", ["f32", "u8", "f64"])
def test_table_of_a_buffer_on_no_boundary(reflibs, monkeypatch, dtype):
    """base one sample off, an odd pitch, a slice with rows to spare: k_ranges sample by sample"""
    import torch
    data = steep(A).astype(NP[dtype]) if dtype != "u8" else typed_ramp("u8", A)
    iso = {"f32": 1840.0, "f64": 1840.0, "u8": 100.5}[dtype]
    ref = reference(reflibs, "odd", dtype, data, iso)
    pitch, slc = A[2] + 3, (A[2] + 3) * (A[1] + 2) + 1
    flat = torch.full((1 + slc * A[0] + 64,), 77, dtype=to_device(data[:1, :1, :2]).dtype, device="cuda")
    view = torch.as_strided(flat, A, (slc, pitch, 1), 1)
    view.copy_(to_device(data))
    assert view.data_ptr() % 16 != 0 or (pitch * data.dtype.itemsize) % 16 != 0
    four_runs(monkeypatch, lambda: grid_of(view), (iso,), (ref,), dtype, data, ("odd layout", dtype))


# ---- rows of 256 k + 1 points: the last strip's last column is the grid's last -------------------------------------------------------------

@pytest.mark.parametrize("padded", [False, True], ids=["dense", "pitch16"])
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("npx", [257, 513, 1025, 1281])
def test_the_deciding_samples_are_the_last_column(reflibs, monkeypatch, depth, npx, dtype, padded):
    """nx a multiple of 256: the last strip of a row is 257 samples wide and its last column has no strip to its right.  The field is
    below the isovalue everywhere but in that column, so a table without it calls every tile dead and the second extraction is
    empty.  padded: rows on 16-byte boundaries (k_ranges in 16-byte pieces), dense: 256 k + 1 samples apart (sample by sample)."""
    import torch
    shape = (20, 70, npx)
    data = ramp(shape, 0, 1, 1).astype(NP[dtype])             # y + z: 0 .. 88
    data = np.ascontiguousarray(np.broadcast_to(data, shape)).copy()
    data[:, :, -1] += 150                                     # 150 .. 238 in x = nx alone
    iso = 120.5
    tab = numpy_table(data, dtype)
    nseg = tab.shape[2]
    assert (npx - 1) % 256 == 0 and (tab[:, :, :nseg - 1, 1] < iso).all() and (tab[:, :, nseg - 1, 1] > iso).all() and (data[:, :, :-1] < iso).all()
    ref = reference(reflibs, ("lastcol", npx), dtype, data, iso)
    assert ref.nV >= shape[0] * shape[1]
    if padded:
        pitch = (npx + 15) // 16 * 16
        flat = torch.full((shape[0], shape[1], pitch), 99, dtype=to_device(data[:1, :1, :2]).dtype, device="cuda")
        t = flat[:, :, :npx]
        t.copy_(to_device(data))
        assert t.data_ptr() % 16 == 0 and (pitch * data.dtype.itemsize) % 16 == 0
    else:
        t = to_device(data)
    four_runs(monkeypatch, lambda: grid_of(t), (iso,), (ref,), dtype, data, ("last column", npx, dtype, padded, depth))


# ---- staleness: who must say what ----------------------------------------------------------------------------------------------------------------

def test_torch_writes_are_seen_and_uncounted_ones_after_changed(reflibs):
    data = steep(A).copy()
    iso = STEEP_ISO[A]
    t = to_device(data)
    g = grid_of(t)
    g.set_timing(1)
    for rep in range(3):
        same(g.extract(iso), reference(reflibs, ("steep", A), "f32", data, iso), ("before", rep))
    assert table_of(g, "f32") is not None and skipped(g)[1] > 0
    # 1. an in-place write inside a tile that is left out: seen by the next call, nothing said
    assert numpy_table(data, "f32")[10, 0, 0, 1] < iso
    t[10, 5, 5] = 5000.0
    data[10, 5, 5] = 5000.0
    ref1 = reflibs["f32"].isosurface(data, iso)
    assert ref1.nV > reference(reflibs, ("steep", A), "f32", steep(A), iso).nV
    for rep in range(3):
        same(g.extract(iso), ref1, ("t[z, y, x] = big", rep))
    # 2. the whole tensor negated in place
    t.neg_()
    data = -data
    ref2 = reflibs["f32"].isosurface(data, -iso)
    for rep in range(3):
        same(g.extract(-iso), ref2, ("neg_", rep))
    assert np.array_equal(words(table_of(g, "f32")), words(numpy_table(data, "f32")))
    # 3. a write torch does not count: seen after changed()
    v = t._version
    t.data[20, 190, 100] = -9000.0   # (a tile of the negated ramp that lies wholly above -1840 and is left out: a sample below it)
    assert t._version == v
    data[20, 190, 100] = -9000.0
    assert numpy_table(-steep(A), "f32")[20, 3, 0, 0] > -iso and skipped(g)[2] > 0
    g.changed()
    ref3 = reflibs["f32"].isosurface(data, -iso)
    assert ref3.nV > ref2.nV  # (the write makes new surface: a changed() that did nothing would leave it out)
    for rep in range(3):
        same(g.extract(-iso), ref3, ("t.data + changed()", rep))
    g.close()


def test_a_volatile_grid_never_has_a_table(reflibs):
    data = steep(A).copy()
    iso = STEEP_ISO[A]
    t = to_device(data)
    g = grid_of(t, volatile=True)
    for rep in range(3):
        same(g.extract(iso), reference(reflibs, ("steep", A), "f32", data, iso), ("volatile", rep))
    assert table_of(g, "f32") is None
    t.data[10, 5, 5] = 5000.0
    data[10, 5, 5] = 5000.0
    ref = reflibs["f32"].isosurface(data, iso)
    for rep in range(2):
        same(g.extract(iso), ref, ("volatile, t.data write", rep))
    assert table_of(g, "f32") is None
    g.close()


def test_c_api_in_place_edit_with_a_table_in_between(products, reflibs):
    """the library's own copy: calculate_isosurface three times (a table is built), G->F rewritten inside a tile that was left out,
    MC33_grid_changed, and three more"""
    from parity import assert_surface_parity
    lib, ref = products["f32"], reflibs["f32"]
    L = lib.lib
    a = steep(A).copy()
    iso = STEEP_ISO[A]
    G, keep = lib.make_grid(a)
    M = L.create_MC33(G)
    assert M
    try:
        def surf():
            S = L.calculate_isosurface(M, C.c_float(iso))
            assert S
            try:
                return lib.copy_surface(S)
            finally:
                L.free_surface_memory(S)
        want = reference(reflibs, ("steep", A), "f32", a, iso)
        for rep in range(3):
            assert_surface_parity(surf(), want, 1.0, "before %d" % rep, bit_exact=True)
        a[10, 5, 5] = 5000.0
        keep[10, 5, 5] = 5000.0
        L.MC33_grid_changed(M)
        want2 = ref.isosurface(a, iso)
        assert want2.nV > want.nV
        for rep in range(3):
            assert_surface_parity(surf(), want2, 1.0, "after the change %d" % rep, bit_exact=True)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
