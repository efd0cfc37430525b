"""GPU tests of the case atlas (tests/atlas_cases.py; tests/test_atlas_cpu.py proves what the inputs reach): every (sign index,
pattern offset) pair of the table at every grid-face position - FACE records are a function of (table row x face flags) - and
every reachable id-source rule of the vertices on grid points, each against the unmodified reference (oracle/_ref), bit for bit."""
import time

import numpy as np
import pytest

import atlas_cases as ac
import layouts as lo
from parity import assert_surface_parity

pytestmark = pytest.mark.gpu

ATLAS = ac.load_row_atlas()
RULES = ac.load_rule_atlas()
SWITCHES = ["MC33_HIP_TRI_FIRST=0", "MC33_HIP_TRI_FIRST=1", "MC33_HIP_NO_FORK=0", "MC33_HIP_NO_FORK=1",
            "MC33_HIP_TRI_FIRST=0,MC33_HIP_NO_FORK=1", "MC33_HIP_TRI_FIRST=1,MC33_HIP_NO_FORK=1", "MC33_HIP_NO_PACK=1", "MC33_HIP_NO_STAGE=1",
            "MC33_HIP_SLOW_SLOTS=0,MC33_HIP_NO_FORK=0"]  # those of test_every_emit_order_and_code_path_switch

_layouts, _refs = {}, {}


def row_grid(flags, dtype):
    """(data, isovalue, witness positions) of the row layout at `flags`, built once"""
    if (flags, dtype) not in _layouts:
        grid, pos = ac.row_layout(flags, ATLAS[2])
        _layouts[flags, dtype] = ac.as_dtype(grid, dtype) + (pos,)
    return _layouts[flags, dtype]


def reference(lib, key, data, iso):
    """the expected surface, once per key"""
    key = (lib.path,) + key
    if key not in _refs:
        _refs[key] = lib.isosurface(data, iso)
    return _refs[key]


def setenv(monkeypatch, switch):
    for kv in switch.split(",") if switch else ():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)  # (read when a context is made)


def same_surface(got, ref, label, pos=None):
    """bit-exact parity; a mismatch on a row layout names the witnesses (atlas index, sign index, pattern offset) next to the first
    vertex that differs"""
    try:
        assert_surface_parity(got, ref, 2048.0, label, bit_exact=True)
    except AssertionError as e:
        who = ""
        if pos is not None and ref.nV and got.nV:
            n = min(got.nV, ref.nV)
            bad = np.nonzero(np.any(got.V[:n].view(np.uint8) != ref.V[:n].view(np.uint8), axis=1) | np.any(got.N[:n].view(np.uint8) != ref.N[:n].view(np.uint8), axis=1))[0]
            if not len(bad):  # the vertices agree: the first triangle that differs, by its first vertex
                m = min(got.nT, ref.nT)
                tri = np.nonzero(np.any(got.T[:m] != ref.T[:m], axis=1))[0]
                bad = [int(ref.T[tri[0], 0])] if len(tri) else [n - 1]
            at = ref.V[bad[0]].astype(np.float64)[::-1]  # (z, y, x) in cells: unit spacing, origin 0
            near = np.nonzero(np.all(np.abs(pos + 0.5 - at) <= 1.5, axis=1))[0]
            who = "; first difference at (z, y, x) = %s, witnesses there (atlas index, sign index, pattern): %s" % (
                at.tolist(), [(int(k), int(ATLAS[0][k]), int(ATLAS[1][k])) for k in near])
        raise AssertionError(str(e) + who)


# ---- row atlas ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ac.ROW_DTYPES)
@pytest.mark.parametrize("flags", range(7))
def test_row_layouts_three_times_on_one_context(products, reflibs, flags, dtype):
    """(three times: the first sweep of a context has no block table, and the emit path of a call follows the call before it)"""
    data, iso, pos = row_grid(flags, dtype)
    ref = reference(reflibs[dtype], ("row", flags, dtype), data, iso)
    assert ref.nT > 766
    ctx = ac.OneContext(products[dtype], data)
    try:
        for rep in range(3):
            same_surface(ctx.surface(iso), ref, "row atlas flags %d %s call %d" % (flags, dtype, rep), pos)
    finally:
        ctx.close()


@pytest.mark.parametrize("fresh_every", [1, 50])
@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_corner_atlas(products, reflibs, dtype, fresh_every):
    """face flags 7: a 2 x 2 x 2 grid per witness, 766 extractions - a context per witness (every sweep is a context's first), and
    one context whose samples are exchanged with MC33_grid_changed (every call follows another), a fresh one for every 50th"""
    data, iso = ac.as_dtype(ATLAS[2], dtype)
    t0, ctx = time.perf_counter(), None
    try:
        for k, cell in enumerate(data):
            if k % fresh_every == 0:
                if ctx is not None:
                    ctx.close()
                ctx = ac.OneContext(products[dtype], cell)
            else:
                ctx.set_data(cell)
            got = ctx.surface(iso)
            ref = reflibs[dtype].isosurface(cell, iso)
            assert ref.nT > 0
            same_surface(got, ref, "corner atlas %s witness %d (sign index %d, pattern %d, flags 7)" % (dtype, k, ATLAS[0][k], ATLAS[1][k]))
    finally:
        if ctx is not None:
            ctx.close()
    print("corner atlas %s, a context per %d: %d extractions in %.2f s" % (dtype, fresh_every, len(data), time.perf_counter() - t0))


@pytest.mark.parametrize("switch", SWITCHES)
def test_row_layouts_under_every_switch(products, reflibs, switch, monkeypatch):
    setenv(monkeypatch, switch)
    for flags in (0, 3, 6):
        data, iso, pos = row_grid(flags, "f32")
        ref = reference(reflibs["f32"], ("row", flags, "f32"), data, iso)
        ctx = ac.OneContext(products["f32"], data)
        try:
            for rep in range(2):  # (the second call decides by the first one's counts)
                same_surface(ctx.surface(iso), ref, "row atlas flags %d %s call %d" % (flags, switch, rep), pos)
        finally:
            ctx.close()


@pytest.mark.parametrize("ortho,nneg", [(False, True), (True, False), (True, True)])
def test_row_layouts_through_the_flavours(reflibs, ortho, nneg):
    """the _nneg (winding m / n exchanged per row, normals negated) and _ortho builds against the reference built the same way"""
    from mc33_capi import MC33Lib, product_path, ref_path
    P = MC33Lib(product_path("f32", ortho=ortho, nneg=nneg), "f32", ortho=ortho)
    R = MC33Lib(ref_path("f32", ortho=ortho, nneg=nneg), "f32", ortho=ortho)
    for flags in (0, 6):
        data, iso, pos = row_grid(flags, "f32")
        ref = reference(R, ("row", flags, "f32"), data, iso)
        same_surface(P.isosurface(data, iso), ref, "row atlas flags %d ortho %d nneg %d" % (flags, ortho, nneg), pos)
        plain = reference(reflibs["f32"], ("row", flags, "f32"), data, iso)
        assert np.array_equal(ref.T[:, [1, 0, 2]] if nneg else ref.T, plain.T)  # ... and really the (mirror image of the) default build


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_row_layouts_over_z_slabs(products, reflibs, dtype, monkeypatch):
    """three z-slabs behind the C API: witness rows sit on the slab interfaces"""
    monkeypatch.setenv("MC33_HIP_DEVICES", "0,0,0")
    for flags in (0, 3):
        data, iso, pos = row_grid(flags, dtype)
        ref = reference(reflibs[dtype], ("row", flags, dtype), data, iso)
        same_surface(products[dtype].isosurface(data, iso), ref, "row atlas flags %d %s, 3 slabs" % (flags, dtype), pos)


def test_row_layout_in_an_adopted_buffer(reflibs):
    """the x-line (face flags 6, five row segments) through DeviceGrid at a padded odd pitch, padded slice and offset"""
    from mc33_c_library_amd import DeviceGrid
    from mc33_capi import Surface
    data, iso, pos = row_grid(6, "f32")
    ref = reference(reflibs["f32"], ("row", 6, "f32"), data, iso)
    lay = lo.layout("all", data.shape, data.dtype.itemsize)
    flat = lo.to_device(lo.place(data, lay, [iso]))
    g = DeviceGrid(lo.device_view(flat, data.shape, lay), npx=data.shape[2])
    try:
        for rep in range(2):
            V, N, T, cnt = g.extract(iso)
            got = Surface(cnt.nV, cnt.nT, V.cpu().numpy().reshape(-1, 3), N.cpu().numpy().reshape(-1, 3),
                          T.cpu().numpy().view(np.uint32).reshape(-1, 3), None, iso)
            same_surface(got, ref, "row atlas flags 6, layout all, call %d" % rep, pos)
    finally:
        g.close()


# ---- rule atlas ---------------------------------------------------------------------------------------------------------------

def _name(k):
    return "rule grid %d %s" % (k, RULES["grids"][k]["shape"])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("switch", [None, "MC33_HIP_SLOW_SLOTS=0", "MC33_HIP_SLOW_SLOTS=1", "MC33_HIP_SLOW_COUNT=0", "MC33_HIP_SLOW_COUNT=1"])
def test_rule_grids(products, reflibs, switch, dtype, monkeypatch):
    """every witness grid of the on-point rules, with either slow emit kernel and with / without the identity count's own launch"""
    setenv(monkeypatch, switch)
    for k, g in enumerate(RULES["grids"]):
        data, iso = ac.rule_grid(g, dtype)
        ref = reference(reflibs[dtype], ("rule", k, dtype), data, iso)
        same_surface(products[dtype].isosurface(data, iso), ref, "%s %s %s" % (_name(k), dtype, switch))


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_rule_grids_as_a_miss_after_a_call_without_on_point_corners(products, reflibs, dtype):
    """the second extraction of a context whose first isovalue no sample equals: the tail left the slow kernels out and repeats"""
    for k, g in enumerate(RULES["grids"]):
        data, iso = ac.rule_grid(g, dtype)
        assert not np.any(data == iso + 0.5)
        ctx = ac.OneContext(products[dtype], data)
        try:
            same_surface(ctx.surface(iso + 0.5), reference(reflibs[dtype], ("rule+", k, dtype), data, iso + 0.5), "%s %s first" % (_name(k), dtype))
            same_surface(ctx.surface(iso), reference(reflibs[dtype], ("rule", k, dtype), data, iso), "%s %s second" % (_name(k), dtype))
        finally:
            ctx.close()
