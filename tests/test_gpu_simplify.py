"""GPU tests of the vertex clustering (include/mc33_hip.h: mc33hip_simplify_surface; include/marching_cubes_33.h:
MC33_calculate_simplified_isosurface; DeviceGrid.simplify / extract_simplified).

V and T come from the reference twin (oracle/_ref) or are made up (tests/simplify_cases.py); the expected arrays come from
tests/simplify_oracle.py, the definition in numpy, and the normals from tests/smooth_oracle.py applied to the oracle's output.
Everything is compared bit for bit - oV, oN, oT, both attributes, oMap and the eight counts; nothing here has a tolerance.  Every
output of every call is canaried (tests/mesh_harness.py: CanariedCall)."""
import ctypes as C

import numpy as np
import pytest

from capi_slab_refusals import refusal
import fixtures as fx
import measure_oracle as mo
import mesh_pieces as mp
import property_oracle as po
import simplify_cases as sc
import simplify_oracle as sp
from mc33_capi import MC33Lib, ref_path
from mesh_checks import reference_mesh as mesh
from mesh_harness import SPARE, SimplifyCall as Call, bits, capi, c_palette, ctx, device_grid, normals_of, once_per_key, palette, to_device, words  # noqa: F401 (ctx: the module's fixture)
from simplify_cases import CELLS, MODES, TABLE, csimp, simplified

pytestmark = pytest.mark.gpu

COUNTS = sp.Simplified.COUNTS


def check_topology(g, call):
    """mc33hip_surface_topology on the output: no invalid triangle (it would raise), none degenerate, every vertex named"""
    nV2, nT2 = call.counts[0], call.counts[1]
    if nT2:
        t = g.topology(call.oT[:nT2].contiguous(), nV2)
        assert t.degenerate_triangles == 0 and t.referenced_vertices == nV2


@once_per_key
def uploaded(reflibs, name):
    """a fixture's surface and two attribute arrays on the device, uploaded once"""
    data, r0, d, iso, s = mesh(reflibs, name)
    A = (words(s.nV, 11), words(s.nV, 12))
    return (to_device(s.V), to_device(s.T), A, [to_device(x) for x in A])


# ---- the five fixtures x the two cells x both modes x duplicates dropped and kept ------------------------------------------------

@pytest.mark.parametrize("drop", [True, False], ids=["drop", "keep"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cell", list(CELLS))
@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_fixtures_f32(reflibs, ctx, name, cell, mode, drop):
    data, r0, d, iso, s = mesh(reflibs, name)
    want = simplified(reflibs, name, cell, mode, drop)
    if drop:
        assert want.counts()[:6] == TABLE[(name, cell)]
    V, T, A, dA = uploaded(reflibs, name)
    c = tuple(CELLS[cell][k] * d[k] for k in range(3))
    first = Call(ctx, V, T, c, r0, MODES[mode], drop, attrs=dA)
    assert first.rc == 0, first.message
    first.check(want, A)
    check_topology(ctx, first)
    again = Call(ctx, V, T, c, r0, MODES[mode], drop, attrs=dA)
    assert again.rc == 0 and again.all_bytes() == first.all_bytes(), "two calls on the same inputs differ"


@pytest.mark.parametrize("name", ["sphere", "quant"])
def test_tiny_cells_against_the_compaction_and_one_cell(reflibs, ctx, name):
    """cells of d / 1024, the first vertex of each, duplicates kept, on meshes where no two vertices share such a cell: what
    mc33hip_compact_components leaves with every root selected, computed on the device on the same mesh.  Then one cell that
    holds the whole bounding box, and no triangles at all."""
    import torch
    data, r0, d, iso, s = mesh(reflibs, name)
    V, T, A, dA = uploaded(reflibs, name)
    labels = ctx.label_components(T, s.nV)[0]
    N = to_device(s.N)
    V2, N2, T2, (A2,), vmap, kept = ctx.compact_components(V, N, T, labels, [], invert=True, attrs=dA[:1])
    cell = tuple(x / 1024.0 for x in d)
    call = Call(ctx, V, T, cell, r0, sp.FIRST, False, attrs=dA[:1])
    assert call.rc == 0, call.message
    nV2, nT2 = call.counts[0], call.counts[1]
    assert (nV2, nT2) == (V2.shape[0], T2.shape[0]) and call.counts[2:6] == (nV2, 1, 0, 0)
    assert torch.equal(call.oV[:nV2].view(torch.int32), V2.view(torch.int32)) and torch.equal(call.oT[:nT2], T2)
    assert torch.equal(call.oMap[:s.nV], vmap) and torch.equal(call.oA[0][:nV2], A2)
    call.check(sp.simplify(s.V, s.T, cell, r0, sp.FIRST, False), A[:1])
    lo, hi = s.V.min(axis=0).astype(np.float64), s.V.max(axis=0).astype(np.float64)
    one = Call(ctx, V, T, (hi - lo) * 2.0 + 1.0, lo - 0.5, sp.MEAN, True, attrs=dA)
    assert one.rc == 0 and one.counts == (0, 0, 1, s.nV - (25 if name == "quant" else 0), s.nT, 0, 0, 0), (one.counts, one.message)
    one.check(sp.simplify(s.V, s.T, (hi - lo) * 2.0 + 1.0, lo - 0.5, sp.MEAN, True), A)
    assert np.all(one.host(one.oMap[:s.nV]).view(np.uint32) == sp.NONE)
    empty = Call(ctx, V, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), cell, r0, sp.MEAN, True, attrs=dA)
    assert empty.rc == 0 and empty.counts == (0,) * 8
    empty.check(sp.simplify(s.V, np.zeros((0, 3), np.uint32), cell, r0), A)


# ---- made-up meshes: where the kernels can still go wrong ---------------------------------------------------------------------------

LADDER = [1, 2, 63, 64, 65, 255, 256, 257, 1024, 5000]


def run_made_up(ctx, V, T, cell, origin, modes=(sp.MEAN, sp.FIRST), drops=(True,)):
    A = (words(V.shape[0], 21), words(V.shape[0], 22))
    dV, dT, dA = to_device(V), to_device(T), [to_device(x) for x in A]
    out = []
    for mode in modes:
        for drop in drops:
            want = sp.simplify(V, T, cell, origin, mode, drop)
            call = Call(ctx, dV, dT, cell, origin, mode, drop, attrs=dA)
            assert call.rc == 0, call.message
            call.check(want, A)
            check_topology(ctx, call)
            out.append(want)
    return out


@pytest.mark.parametrize("order", ["consecutive", "scattered", "scattered-permuted"])
def test_cluster_sizes(ctx, order):
    """clusters of 1 .. 5000 members, twice each: the members in a row - whole waves fall into one cluster and one lane adds for
    them - and scattered over the array, the representative far from its lanes: every member adds for itself"""
    V, T = sc.clustered(LADDER * 2, 7, order != "consecutive", vertex_order="permuted" if order.endswith("permuted") else "identity")
    for want in run_made_up(ctx, V, T, sc.CELL, sc.ORIGIN, drops=(True, False)):
        assert (want.clusters, want.max_cluster) == (2 * len(LADDER), 5000) and want.clamped_vertices == 0
        assert want.nT_out > 100


def test_65000_clusters(ctx):
    V, T = sc.clustered([4] * 65000, 8, True)
    (want,) = run_made_up(ctx, V, T, sc.CELL, sc.ORIGIN, modes=(sp.MEAN,))
    assert (want.clusters, want.max_cluster) == (65000, 4) and want.nV_out > 60000


@pytest.mark.parametrize("nV", [n for n in mp.TILE_EDGE_SIZES if n not in (1026, 262146)])
def test_scan_tiles(ctx, nV):
    """vertex counts around 1 and 256 tiles of the scans, clusters of three scattered over them"""
    nref = nV - 5
    V, T = sc.clustered([3] * (nref // 3) + ([nref % 3] if nref % 3 else []), nV, True)
    assert V.shape[0] == nV
    (want,) = run_made_up(ctx, V, T, sc.CELL, sc.ORIGIN, modes=(sp.MEAN,))
    assert want.max_cluster == 3 and want.nT_out > nV // 2


def test_edge_of_the_lattice(ctx):
    """keys that differ only in the top bits of an axis, cells at k = 2097151, and clamped vertices: negative, at and beyond the
    far end, infinite, NaN - the count and the arrays follow the definition"""
    V, T, clamped = sc.edge_of_the_lattice(5)
    for want in run_made_up(ctx, V, T, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), drops=(True, False)):
        assert want.clamped_vertices == clamped and want.clusters > 500
    k, t, c = sp.keys(V[:4000], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert np.any(k == 2097151) and np.any(k >= 1048576 + 3) and np.any(t == 1.0) and np.any(np.isnan(V[:4000]))


def test_planted_duplicates(ctx):
    """300 copies of triangles, every second with the opposite winding, all rotated, anywhere in T: with drop_duplicates each
    set's smallest index survives - the copies lie before or behind their originals"""
    V, T = sc.clustered([1] * 6000, 8, True)
    T2, where = sc.plant_duplicates(T, 300, 9)
    keep, drop = run_made_up(ctx, V, T2, sc.CELL, sc.ORIGIN, modes=(sp.MEAN,), drops=(False, True))
    assert (keep.collapsed_triangles, keep.duplicate_triangles, keep.nT_out) == (0, 0, T2.shape[0])
    assert (drop.duplicate_triangles, drop.nT_out) == (300, T.shape[0])
    lost = np.setdiff1d(np.arange(T2.shape[0]), drop.survivors)
    srt = np.sort(T2.astype(np.int64), axis=1)
    for i in lost.tolist():  # what went has a twin with a smaller index that stayed
        twins = np.nonzero((srt == srt[i]).all(axis=1))[0]
        assert twins[0] < i and twins[0] in drop.survivors
    assert np.count_nonzero(np.isin(where, lost)) > 50 and np.count_nonzero(~np.isin(where, lost)) > 50  # copies went, and originals behind copies


def test_invalid_triangles_are_counted_not_read(reflibs, ctx):
    """mesh_pieces.spoil(..., "invalid"): 300 triangles name row nV.  V is the first nV rows of a tensor with spare rows behind
    them, so that not even a wrong kernel could touch memory this test does not own."""
    import torch
    from mc33_c_library_amd.api import ERUNTIME
    data, r0, d, iso, s = mesh(reflibs, "blobs")
    room = torch.zeros((s.nV + SPARE, 3), dtype=torch.float32, device="cuda")
    room[:s.nV] = to_device(s.V)
    V = room[:s.nV]
    badT = mp.spoil(s.T, s.nV, 3, "invalid")
    c = tuple(2.0 * x for x in d)
    want = sp.simplify(s.V, badT, c, r0, sp.MEAN, True)
    assert want.invalid_triangles == mp.SPOILED_EACH
    A = (words(s.nV, 11),)
    bad = Call(ctx, V, to_device(badT), c, r0, sp.MEAN, True, attrs=[to_device(A[0])])
    assert bad.rc == ERUNTIME and "300 triangles " in bad.message, (bad.rc, bad.message)
    bad.check(want, A)  # the outputs are the oracle's without those triangles
    check_topology(ctx, bad)
    good = Call(ctx, V, to_device(s.T), c, r0, sp.MEAN, True)  # the next call on the context succeeds
    assert good.rc == 0, good.message
    good.check(simplified(reflibs, "blobs", "2x2x2", "mean", True))


def test_capacity_and_the_size_query(reflibs, ctx):
    from mc33_c_library_amd.api import ECAPACITY
    data, r0, d, iso, s = mesh(reflibs, "sheet")
    want = simplified(reflibs, "sheet", "3x2x5", "mean", True)
    V, T, A, dA = uploaded(reflibs, "sheet")
    c = tuple(CELLS["3x2x5"][k] * d[k] for k in range(3))
    for capV, capT in ((want.nV_out - 1, want.nT_out), (want.nV_out, want.nT_out - 1), (0, want.nT_out), (want.nV_out, 0)):
        short = Call(ctx, V, T, c, r0, sp.MEAN, True, attrs=dA, capV=capV, capT=capT)
        assert short.rc == ECAPACITY and short.counts == want.counts(), (short.rc, short.message)
        assert str(want.nV_out) in short.message and str(want.nT_out) in short.message
        short.spare_intact(written=False)  # nothing is written, the map included
    query = Call(ctx, V, T, c, r0, sp.MEAN, True, capV=0, capT=0, with_map=False, with_normals=False, change=dict(oV=None, oT=None))
    assert query.rc == ECAPACITY and query.counts == want.counts()
    exact = Call(ctx, V, T, c, r0, sp.MEAN, True, attrs=dA, capV=want.nV_out, capT=want.nT_out)
    assert exact.rc == 0, exact.message
    exact.check(want, A)


def test_invalid_arguments(reflibs, ctx):
    import torch
    from mc33_c_library_amd.api import EINVAL, Simplification
    data, r0, d, iso, s = mesh(reflibs, "sheet")
    V, T, A, dA = uploaded(reflibs, "sheet")
    nan, inf = float("nan"), float("inf")
    cases = [dict(V=None), dict(T=None), dict(oV=None), dict(oT=None), dict(attr0=None), dict(oAttr0=None), dict(nV=1 << 32), dict(nT=1 << 32), dict(n_attr=3),
             dict(mode=2), dict(mode=-1), dict(cell=(0.0, 1.0, 1.0)), dict(cell=(1.0, -1.0, 1.0)), dict(cell=(1.0, 1.0, inf)), dict(cell=(nan, 1.0, 1.0)),
             dict(origin=(inf, 0.0, 0.0)), dict(origin=(0.0, -inf, 0.0)), dict(origin=(0.0, 0.0, nan))]
    for change in cases:
        call = Call(ctx, V, T, (1.0, 1.0, 1.0), r0, attrs=dA, change=change)
        assert call.rc == EINVAL, (change, call.rc, call.message)
        call.spare_intact(written=False)  # every output still at its fill
    L = ctx.lib.mc33hip_simplify_surface
    assert L(ctx.ctx, None) == EINVAL and L(None, C.byref(Simplification())) == EINVAL
    # every overlapping pair of ranges: each array gets a place of its own in one buffer, then one output at a time is moved onto
    # the last byte of an input or of another output
    nV, nT, capV, capT = 1000, 2000, 900, 1800
    size = {"V": nV * 12, "T": nT * 12, "attr0": nV * 4, "attr1": nV * 4, "oV": capV * 12, "oT": capT * 12, "oN": capV * 12, "oMap": nV * 4, "oAttr0": capV * 4, "oAttr1": capV * 4}
    buf = torch.zeros((sum(size.values()) + 64 * len(size),), dtype=torch.uint8, device="cuda")
    at, off = {}, 0
    for n, b in size.items():
        at[n] = buf.data_ptr() + off
        off += b + 64

    def struct(moved=None, onto=None, end=True):
        a = Simplification()
        p = dict(at)
        if moved:
            p[moved] = at[onto] + size[onto] - 1 if end else at[onto] - size[moved] + 1
        a.V, a.T, a.nV, a.nT, a.n_attr = p["V"], p["T"], nV, nT, 2
        a.attr[0], a.attr[1], a.oAttr[0], a.oAttr[1] = p["attr0"], p["attr1"], p["oAttr0"], p["oAttr1"]
        a.origin, a.cell = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(1.0, 1.0, 1.0)
        a.oV, a.oT, a.oN, a.oMap, a.capV, a.capT = p["oV"], p["oT"], p["oN"], p["oMap"], capV, capT
        return a
    outs, ins = ["oV", "oT", "oN", "oMap", "oAttr0", "oAttr1"], ["V", "T", "attr0", "attr1"]
    pairs = [(o, i) for o in outs for i in ins] + [(o, p) for o in outs for p in outs if o != p]
    assert len(pairs) == 24 + 30
    for o, other in pairs:
        for end in (True, False):
            assert L(ctx.ctx, C.byref(struct(o, other, end))) == EINVAL, (o, other, end)
    assert not buf.any().item()  # nothing was written
    assert L(ctx.ctx, C.byref(struct())) == 0  # the same arrays side by side: zeros, every triangle collapsed
    assert np.array_equal(bits(V.cpu().numpy()), bits(s.V)) and np.array_equal(T.cpu().numpy().view(np.uint32), s.T)
    assert Call(ctx, V, T, (1.0, 1.0, 1.0), r0).rc == 0  # the context is still good


# ---- the other builds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["u8", "f64"])
def test_other_sample_types(reflibs, case):
    """MC33_real is double in libMC33_f64: rows of 24 bytes, and FIRST moves all of them"""
    dtype, n = case, 40
    r0, d = mo.AWKWARD_R0, mo.AWKWARD_D
    if dtype == "f64":
        data, iso = fx.cos_field(n, dtype=np.float64)[0], 0.0
    else:
        data, iso = fx.cos_field_int(n, np.uint8, 40.0, 128.0), 128.5
    s = reflibs[dtype].isosurface(data, iso, r0, d)
    assert s.V.dtype == (np.float64 if dtype == "f64" else np.float32) and s.V.strides[0] == (24 if dtype == "f64" else 12) and s.nV > 1000
    g = device_grid(data, r0, d)
    V, T = to_device(s.V), to_device(s.T)
    A = (words(s.nV, 31),)
    c = tuple(3.0 * x for x in d)
    for mode in (sp.MEAN, sp.FIRST):
        want = sp.simplify(s.V, s.T, c, r0, mode, True)
        assert want.V.dtype == s.V.dtype and 100 < want.nV_out < s.nV // 4
        call = Call(g, V, T, c, r0, mode, True, attrs=[to_device(A[0])])
        assert call.rc == 0, call.message
        call.check(want, A)
        check_topology(g, call)
    V3, N3, T3, info = g.extract_simplified(iso, 3.0, mode="first")
    assert (info["nV_out"], info["nT_out"]) == (want.nV_out, want.nT_out)
    assert np.array_equal(bits(V3.cpu().numpy()), bits(want.V)) and np.array_equal(T3.cpu().numpy().view(np.uint32), want.T)
    assert np.array_equal(bits(N3.cpu().numpy()), bits(normals_of(want)))
    g.close()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def test_python_methods(reflibs):
    data, r0, d, iso, s = mesh(reflibs, "quant")
    P = fx.noise_f32(0, 77, shape=data.shape) * np.float32(1000.0)
    g = device_grid(data, r0, d, P)
    V, T = to_device(s.V), to_device(s.T)
    A = (words(s.nV, 11), po.sample_property(s.V, r0, d, P))
    for cell, mode, drop in (("2x2x2", "mean", True), ("3x2x5", "first", False)):
        want = simplified(reflibs, "quant", cell, mode, drop)
        c = tuple(CELLS[cell][k] * d[k] for k in range(3))
        V2, N2, T2, attrs2, vmap, info = g.simplify(V, T, c, mode=mode, drop_duplicates=drop, attrs=[to_device(x) for x in A])
        assert tuple(info[n] for n in COUNTS) == want.counts() and info["ratio"] == want.nT_out / s.nT
        assert np.array_equal(bits(V2.cpu().numpy()), bits(want.V)) and np.array_equal(T2.cpu().numpy().view(np.uint32), want.T)
        assert np.array_equal(bits(N2.cpu().numpy()), bits(normals_of(want))) and np.array_equal(vmap.cpu().numpy().view(np.uint32), want.vmap)
        for x, w in zip(attrs2, A):
            assert np.array_equal(bits(x.cpu().numpy()), bits(w[want.keep]))
        # the product's own extraction: its V, T are the reference's bit for bit
        V3, N3, T3, info3, P3 = g.extract_simplified(iso, CELLS[cell], with_property=True, mode=mode, drop_duplicates=drop)
        assert np.array_equal(bits(V3.cpu().numpy()), bits(want.V)) and np.array_equal(T3.cpu().numpy().view(np.uint32), want.T)
        assert np.array_equal(bits(N3.cpu().numpy()), bits(normals_of(want))) and np.array_equal(bits(P3.cpu().numpy()), bits(A[1][want.keep]))
    none = g.simplify(V, T, c, origin=(1.0, 2.0, 3.0), normals=False)  # another origin: another result, and no normals
    w = sp.simplify(s.V, s.T, c, (1.0, 2.0, 3.0))
    assert none[1] is None and np.array_equal(bits(none[0].cpu().numpy()), bits(w.V)) and w.clamped_vertices > 0
    g.close()


# ---- the C API -----------------------------------------------------------------------------------------------------------------------

def simplified_surface(lib, M, iso, sm):
    S = lib.lib.MC33_calculate_simplified_isosurface(M, lib.real(iso), C.byref(sm) if sm is not None else None)
    if not S:
        return None
    try:
        m, r = M.contents, S.contents
        assert (m.nV, m.nT, m.memoryfault, m.iso) == (0, r.nT, 0, np.float32(iso))  # as calculate_isosurface leaves them
        if r.nV:  # the object's public prefix mirrors the returned surface
            assert (m.T, m.V, m.N, m.color, m.capt, m.capv) == (r.T, r.V, r.N, r.color, r.capt, r.capv)
        return lib.copy_surface(S)
    finally:
        lib.lib.free_surface_memory(S)


@pytest.mark.parametrize("nneg", [False, True], ids=["plain", "nneg"])
def test_c_api(reflibs, nneg):
    """the oracle applied to the reference's surface - the _nneg reference's for the _nneg flavour: two indices exchanged, and
    the normals follow the winding"""
    name = "quant"
    field, iso, _ = mo.FIXTURES[name]
    data, r0, d = field()
    s = MC33Lib(ref_path("f32", nneg=True), "f32").isosurface(data, iso, r0, d) if nneg else mesh(reflibs, name)[4]
    lib = capi(nneg=nneg)
    L = lib.lib
    G, keep = lib.make_grid(data, r0, d)
    prop = fx.noise_f32(0, 79, shape=data.shape) * np.float32(10.0)
    Pg, keep2 = lib.make_grid(prop, r0, d)
    M = L.create_MC33(G)
    assert M
    try:
        for cell, mode, drop in (("2x2x2", sp.MEAN, True), ("3x2x5", sp.FIRST, False)):
            c = tuple(CELLS[cell][k] * d[k] for k in range(3))
            want = sp.simplify(s.V, s.T, c, r0, mode, drop)
            got = simplified_surface(lib, M, iso, csimp(CELLS[cell], mode, drop))
            assert got is not None and (got.nV, got.nT) == (want.nV_out, want.nT_out) and np.array_equal(got.T, want.T)
            assert np.array_equal(bits(got.V), bits(want.V)) and np.array_equal(bits(got.N), bits(normals_of(want)))
            assert np.all(got.color == po.DEFAULT_COLOR) and got.color.size == want.nV_out
        # colours: those of the extracted vertices, the first of every cell
        pal, lo, hi = palette(7), -2.5, 3.25
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        painted = simplified_surface(lib, M, iso, csimp(CELLS[cell], mode, drop))
        want_color = po.color_vertices(s.V, r0, d, prop, pal, lo, hi)[want.keep]
        assert np.array_equal(painted.color, want_color) and np.unique(painted.color).size > 2
        assert np.array_equal(bits(painted.V), bits(want.V)) and np.array_equal(painted.T, want.T)
        assert L.MC33_set_property_grid(M, None) == 0
        # one cell for everything: an empty surface, no failure
        void = simplified_surface(lib, M, iso, csimp((100.0, 100.0, 100.0), sp.MEAN, True))
        assert void is not None and (void.nV, void.nT) == (0, 0)
        # a null struct and refused parameters give NULL and leave the object alone; its surface is the reference's still
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        mine = lib.copy_surface(S)
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        nan, inf = float("nan"), float("inf")
        assert simplified_surface(lib, M, iso + 1.0, None) is None
        for sm in (csimp((0.0, 2.0, 2.0), 0, 1), csimp((2.0, -2.0, 2.0), 0, 1), csimp((2.0, 2.0, inf), 0, 1), csimp((nan, 2.0, 2.0), 0, 1), csimp((2.0, 2.0, 2.0), 2, 1)):
            assert simplified_surface(lib, M, iso + 1.0, sm) is None
            assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        L.free_surface_memory(S)
        assert np.array_equal(bits(mine.V), bits(s.V)) and np.array_equal(mine.T, s.T) and np.array_equal(bits(mine.N), bits(s.N))
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2


def test_c_api_refuses_an_inclined_grid():
    data = fx.cos_field(20)[0]
    lib = capi()
    L = lib.lib
    A = [[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    Ai = np.linalg.inv(np.array(A)).tolist()
    G, keep = lib.make_grid(data, inclined=(A, Ai))
    M = L.create_MC33(G)
    assert M
    try:
        assert simplified_surface(lib, M, 0.0, csimp((2.0, 2.0, 2.0), 0, 1)) is None and M.contents.memoryfault == 0
        S = L.calculate_isosurface(M, lib.real(0.0))  # the object is still good
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refuses_an_object_on_several_slabs(launcher):
    """MC33_HIP_DEVICES=0,0 in a fresh process, before the library is loaded: two slabs on one device (tests/capi_slab_refusals_worker.py)."""
    out = refusal(launcher, "simplify")
    assert out["rc"] == 0 and "refused: 1 0" in out["stdout"], out
