"""GPU tests of the clipping by planes (include/mc33_hip.h: mc33hip_clip_surface; include/marching_cubes_33.h:
MC33_calculate_clipped_isosurface; DeviceGrid.clip / extract_clipped).

V, N and T come from the reference twin (oracle/_ref) or are made up (tests/clip_cases.py); the expected arrays come from
tests/clip_oracle.py, the definition in numpy.  Everything is compared bit for bit - oV, oN, oT, both attributes, oMap and the ten
counts; nothing here has a tolerance.  Every output of every call is canaried (tests/mesh_harness.py: CanariedCall)."""
import ctypes as C

import numpy as np
import pytest

from capi_slab_refusals import refusal
import clip_cases as cc
import clip_oracle as co
import fixtures as fx
import measure_oracle as mo
import mesh_pieces as mp
import property_oracle as po
from clip_cases import MODES, PLANES, TABLE, attributes, cbox, cclip, clipped, plane_of
from mc33_capi import MC33Lib, ref_path
from mesh_checks import reference_mesh as mesh
from mesh_harness import SPARE, ClipCall as Call, bits, capi, c_palette, ctx, device_grid, once_per_key, palette, to_device, words  # noqa: F401 (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

COUNTS = co.Clipped.COUNTS


def check_topology(g, call, manifold=False):
    """mc33hip_surface_topology on the output: no invalid triangle (it would raise), every vertex named"""
    nV2, nT2 = call.counts[0], call.counts[1]
    if nT2:
        t = g.topology(call.oT[:nT2].contiguous(), nV2)
        assert t.referenced_vertices == nV2
        if manifold:
            assert t.manifold and t.oriented and t.nonmanifold_edges == 0 and t.degenerate_triangles == 0
        return t


@once_per_key
def uploaded(reflibs, name):
    """a fixture's surface and two attribute arrays on the device, uploaded once"""
    s = mesh(reflibs, name)[4]
    return (to_device(s.V), to_device(s.N), to_device(s.T), [to_device(x) for x in attributes(s.nV)])


# ---- the five fixtures x the four planes, an interpolated and a copied attribute --------------------------------------------------

@pytest.mark.parametrize("which", PLANES)
@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_fixtures_f32(reflibs, ctx, name, which):
    s = mesh(reflibs, name)[4]
    want = clipped(reflibs, name, which)
    assert want.counts()[:8] == TABLE[(name, which)]
    V, N, T, dA = uploaded(reflibs, name)
    plane = plane_of(s.V, which)
    first = Call(ctx, V, N, T, plane, dA, MODES)
    assert first.rc == 0, first.message
    first.check(want)
    check_topology(ctx, first, manifold=name in ("sphere", "blobs", "sheet"))
    again = Call(ctx, V, N, T, plane, dA, MODES)
    assert again.rc == 0 and again.all_bytes() == first.all_bytes(), "two calls on the same inputs differ"
    if which == "oblique":  # the floats copied and interpolated, no normals, no map
        A = attributes(s.nV)
        other = Call(ctx, V, None, T, plane, [dA[0], dA[0]], MODES[::-1], with_map=False)
        assert other.rc == 0, other.message
        other.check(co.clip(s.V, None, s.T, plane, (A[0], A[0]), MODES[::-1]))


# ---- made-up meshes: where the kernels can still go wrong ---------------------------------------------------------------------------

def run_made_up(ctx, V, N, T, plane=cc.PLANE_Z, A=None):
    A = (cc.floats(V.shape[0], 21), words(V.shape[0], 22)) if A is None else A
    want = co.clip(V, N, T, plane, A, MODES)
    call = Call(ctx, to_device(V), to_device(N), to_device(T), plane, [to_device(x) for x in A], MODES)
    assert call.rc == (0 if want.invalid_triangles == 0 else -5), call.message
    call.check(want)
    check_topology(ctx, call)
    return want


@pytest.mark.parametrize("nV", mp.TILE_EDGE_SIZES)
def test_scan_tiles(ctx, nV):
    """vertex counts around 1 and 256 tiles of the scans; the plane cuts about half of the shuffled strips"""
    V, N, T = cc.tile_edge(nV, nV)
    assert V.shape[0] == nV
    want = run_made_up(ctx, V, N, T)
    assert want.cut_triangles > nV // 4 and want.on_plane_vertices > nV // 100 and want.kept_vertices > nV // 3


def test_runs_of_cut_triangles(ctx):
    """runs of 1 .. 1025 consecutive cut triangles between whole and dropped ones: neighbouring lanes hold the same edge"""
    V, N, T, kinds = cc.runs(4)
    want = run_made_up(ctx, V, N, T)
    assert want.cut_triangles == sum(cc.RUNS) and want.whole_triangles == 3 * len(cc.RUNS) and want.dropped_triangles == 2 * len(cc.RUNS)


def test_one_edge_shared_by_5000_triangles(ctx):
    """the cut edge {0, 1} in 5000 triangles anywhere in T, in both directions; its owner is row 3000 or later"""
    V, N, T, first = cc.shared_edge(5)
    want = run_made_up(ctx, V, N, T)
    row = np.nonzero((want.edges == [0, 1]).all(axis=1))[0]
    assert row.size == 1 and want.owners[row[0], 0] == first >= 3000


def test_copies_before_originals(ctx):
    want = run_made_up(ctx, *cc.duplicated(6))
    assert want.cut_triangles > 2000


def test_every_triangle_cut_and_none(ctx):
    V, N, T, kinds = cc.runs(8, lengths=(3000, 1, 700))
    every = run_made_up(ctx, V, N, T[kinds == 0])
    assert every.cut_triangles == 3701 and every.whole_triangles == 0 and every.dropped_triangles == 0
    none = run_made_up(ctx, V, N, T, plane=(0.0, 0.0, 1.0, 10.0))
    assert none.cut_triangles == 0 and none.whole_triangles == T.shape[0] and none.nV_out == V.shape[0]
    gone = run_made_up(ctx, V, N, T, plane=(0.0, 0.0, -1.0, -10.0))
    assert gone.counts()[:7] == (0,) * 7 and gone.dropped_triangles == T.shape[0]


def test_all_patterns_over_several_blocks(ctx):
    """the tiny mesh 400 times: every pattern in every rotation in every lane position; 400 invalid triangles among them"""
    V, N, T, A = cc.tiny_repeated(400)
    words = np.arange(V.shape[0], dtype=np.uint32) * 3 + 1
    want = run_made_up(ctx, V, N, T, A=(A, words))
    assert want.counts() == tuple(400 * x for x in (17, 29, 7, 10, 3, 7, 16, 8, 1, 2))


def test_nonfinite_vertices(ctx):
    V, N, T = cc.nonfinite(7)
    want = run_made_up(ctx, V, N, T)
    s = co.signed(V, cc.PLANE_Z)
    copies = ~np.isfinite(s[want.edges]).all(axis=1)  # new vertices that are byte copies of their end inside
    assert want.nonfinite_vertices > 200 and np.count_nonzero(copies) > 50 and np.isinf(want.V[:want.kept_vertices, 2]).any()
    assert not np.isnan(want.V[:, 2]).any()  # (a NaN is out: it never reaches the output)


# ---- error paths ----------------------------------------------------------------------------------------------------------------------

def test_invalid_triangles_are_counted_not_read(reflibs, ctx):
    """mesh_pieces.spoil(..., "invalid"): 300 triangles name row nV.  V and N are the first nV rows of tensors with spare rows
    behind them, so that not even a wrong kernel could touch memory this test does not own."""
    import torch
    from mc33_c_library_amd.api import ERUNTIME
    s = mesh(reflibs, "blobs")[4]
    roomV = torch.zeros((s.nV + SPARE, 3), dtype=torch.float32, device="cuda")
    roomN = torch.zeros((s.nV + SPARE, 3), dtype=torch.float32, device="cuda")
    roomV[:s.nV] = to_device(s.V)
    roomN[:s.nV] = to_device(s.N)
    badT = mp.spoil(s.T, s.nV, 3, "invalid")
    plane = plane_of(s.V, "oblique")
    A = attributes(s.nV)
    want = co.clip(s.V, s.N, badT, plane, A, MODES)
    assert want.invalid_triangles == mp.SPOILED_EACH
    bad = Call(ctx, roomV[:s.nV], roomN[:s.nV], to_device(badT), plane, [to_device(x) for x in A], MODES)
    assert bad.rc == ERUNTIME and "300 triangles " in bad.message, (bad.rc, bad.message)
    bad.check(want)  # the outputs are the oracle's without those triangles
    check_topology(ctx, bad)
    V, N, T, dA = uploaded(reflibs, "blobs")
    good = Call(ctx, V, N, T, plane, dA, MODES)  # the next call on the context succeeds
    assert good.rc == 0, good.message
    good.check(clipped(reflibs, "blobs", "oblique"))


def test_capacity_and_the_size_query(reflibs, ctx):
    from mc33_c_library_amd.api import ECAPACITY
    s = mesh(reflibs, "sheet")[4]
    want = clipped(reflibs, "sheet", "oblique")
    V, N, T, dA = uploaded(reflibs, "sheet")
    plane = plane_of(s.V, "oblique")
    for capV, capT in ((want.nV_out - 1, want.nT_out), (want.nV_out, want.nT_out - 1), (0, want.nT_out), (want.nV_out, 0)):
        short = Call(ctx, V, N, T, plane, dA, MODES, capV=capV, capT=capT)
        assert short.rc == ECAPACITY and short.counts == want.counts(), (short.rc, short.message)
        assert str(want.nV_out) in short.message and str(want.nT_out) in short.message
        short.spare_intact(written=False)  # nothing is written, the map included
    query = Call(ctx, V, N, T, plane, capV=0, capT=0, with_map=False, with_normals=False, change=dict(oV=None, oT=None))
    assert query.rc == ECAPACITY and query.counts == want.counts()
    exact = Call(ctx, V, N, T, plane, dA, MODES, capV=want.nV_out, capT=want.nT_out)
    assert exact.rc == 0, exact.message
    exact.check(want)


def test_invalid_arguments(reflibs, ctx):
    import torch
    from mc33_c_library_amd.api import EINVAL, Clipping
    s = mesh(reflibs, "sheet")[4]
    V, N, T, dA = uploaded(reflibs, "sheet")
    nan, inf = float("nan"), float("inf")
    cases = [dict(V=None), dict(T=None), dict(oV=None), dict(oT=None), dict(attr0=None), dict(oAttr0=None), dict(nV=1 << 32), dict(nT=1 << 32), dict(n_attr=3),
             dict(attr_mode0=2), dict(attr_mode1=-1), dict(N=None),  # (oN without N)
             dict(plane=(0.0, 0.0, 0.0, 1.0)), dict(plane=(nan, 0.0, 1.0, 0.0)), dict(plane=(1.0, inf, 0.0, 0.0)), dict(plane=(1.0, 0.0, -inf, 0.0)),
             dict(plane=(1.0, 0.0, 0.0, nan)), dict(plane=(1.0, 0.0, 0.0, inf))]
    for change in cases:
        call = Call(ctx, V, N, T, (1.0, 0.0, 0.0, 0.0), dA, MODES, change=change)
        assert call.rc == EINVAL, (change, call.rc, call.message)
        call.spare_intact(written=False)  # every output still at its fill
    L = ctx.lib.mc33hip_clip_surface
    assert L(ctx.ctx, None) == EINVAL and L(None, C.byref(Clipping())) == EINVAL
    # every overlapping pair of ranges: each array gets a place of its own in one buffer, then one output at a time is moved onto
    # the last byte of an input or of another output, or so that its own last byte meets the other's first
    nV, nT, capV, capT = 1000, 2000, 900, 2000
    size = {"V": nV * 12, "N": nV * 12, "T": nT * 12, "attr0": nV * 4, "attr1": nV * 4, "oV": capV * 12, "oT": capT * 12, "oN": capV * 12, "oMap": nV * 4,
            "oAttr0": capV * 4, "oAttr1": capV * 4}
    buf = torch.zeros((sum(size.values()) + 64 * len(size),), dtype=torch.uint8, device="cuda")
    at, off = {}, 0
    for n, b in size.items():
        at[n] = buf.data_ptr() + off
        off += b + 64

    def struct(moved=None, onto=None, end=True):
        a = Clipping()
        p = dict(at)
        if moved:
            p[moved] = at[onto] + size[onto] - 1 if end else at[onto] - size[moved] + 1
        a.V, a.N, a.T, a.nV, a.nT, a.n_attr = p["V"], p["N"], p["T"], nV, nT, 2
        a.attr[0], a.attr[1], a.oAttr[0], a.oAttr[1] = p["attr0"], p["attr1"], p["oAttr0"], p["oAttr1"]
        a.plane = (C.c_double * 4)(0.0, 0.0, 1.0, 1.0)
        a.oV, a.oT, a.oN, a.oMap, a.capV, a.capT = p["oV"], p["oT"], p["oN"], p["oMap"], capV, capT
        return a
    outs, ins = ["oV", "oT", "oN", "oMap", "oAttr0", "oAttr1"], ["V", "N", "T", "attr0", "attr1"]
    pairs = [(o, i) for o in outs for i in ins] + [(o, p) for o in outs for p in outs if o != p]
    assert len(pairs) == 30 + 30
    for o, other in pairs:
        for end in (True, False):
            assert L(ctx.ctx, C.byref(struct(o, other, end))) == EINVAL, (o, other, end)
    assert not buf.any().item()  # nothing was written
    a = struct()
    assert L(ctx.ctx, C.byref(a)) == 0  # the same arrays side by side: zeros - every triangle is (0, 0, 0), in and whole
    assert (a.nV_out, a.nT_out, a.whole_triangles) == (1, nT, nT)
    assert np.array_equal(bits(V.cpu().numpy()), bits(s.V)) and np.array_equal(T.cpu().numpy().view(np.uint32), s.T)
    assert Call(ctx, V, N, T, (1.0, 0.0, 0.0, 0.0)).rc == 0  # the context is still good


# ---- the other builds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["u8", "f64"])
def test_other_sample_types(reflibs, case):
    """MC33_real is double in libMC33_f64: rows of 24 bytes, and the new rows are not rounded to float"""
    dtype, n = case, 40
    r0, d = mo.AWKWARD_R0, mo.AWKWARD_D
    if dtype == "f64":
        data, iso = fx.cos_field(n, dtype=np.float64)[0], 0.0
    else:
        data, iso = fx.cos_field_int(n, np.uint8, 40.0, 128.0), 128.5
    s = reflibs[dtype].isosurface(data, iso, r0, d)
    assert s.V.dtype == (np.float64 if dtype == "f64" else np.float32) and s.V.strides[0] == (24 if dtype == "f64" else 12) and s.nV > 1000
    g = device_grid(data, r0, d)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    A = attributes(s.nV)
    for which in ("oblique", "on-grid"):
        plane = plane_of(s.V, which)
        want = co.clip(s.V, s.N, s.T, plane, A, MODES)
        assert want.V.dtype == s.V.dtype and 100 < want.nV_out < s.nV
        call = Call(g, V, N, T, plane, [to_device(x) for x in A], MODES)
        assert call.rc == 0, call.message
        call.check(want)
        check_topology(g, call)
    want = co.clip(s.V, s.N, s.T, plane_of(s.V, "oblique"))
    V3, N3, T3, infos = g.extract_clipped(iso, [plane_of(s.V, "oblique")])
    assert tuple(infos[0][n] for n in COUNTS) == want.counts()
    assert np.array_equal(bits(V3.cpu().numpy()), bits(want.V)) and np.array_equal(T3.cpu().numpy().view(np.uint32), want.T)
    assert np.array_equal(bits(N3.cpu().numpy()), bits(want.N))
    g.close()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------

def chain(s, planes):
    """the oracle, plane after plane"""
    V, N, T = s.V, s.N, s.T
    outs = []
    for plane in planes:
        o = co.clip(V, N, T, plane)
        V, N, T = o.V, o.N, o.T
        outs.append(o)
    return V, N, T, outs


def test_python_methods(reflibs):
    from mc33_c_library_amd import clip_box
    data, r0, d, iso, s = mesh(reflibs, "quant")
    P = fx.noise_f32(0, 77, shape=data.shape) * np.float32(1000.0)
    g = device_grid(data, r0, d, P)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    A = attributes(s.nV)
    plane = plane_of(s.V, "oblique")
    want = clipped(reflibs, "quant", "oblique")
    V2, N2, T2, attrs2, vmap, info = g.clip(V, N, T, plane, attrs=[to_device(x) for x in A], attr_modes=("lerp_f32", "copy"))
    assert tuple(info[n] for n in COUNTS) == want.counts()
    assert np.array_equal(bits(V2.cpu().numpy()), bits(want.V)) and np.array_equal(T2.cpu().numpy().view(np.uint32), want.T)
    assert np.array_equal(bits(N2.cpu().numpy()), bits(want.N)) and np.array_equal(vmap.cpu().numpy().view(np.uint32), want.vmap)
    for x, w in zip(attrs2, want.attrs):
        assert np.array_equal(bits(x.cpu().numpy()), w)
    bare = g.clip(V, None, T, plane)  # no normals, no attributes
    assert bare[1] is None and bare[3] == [] and np.array_equal(bits(bare[0].cpu().numpy()), bits(want.V))
    # the product's own extraction (its V, N, T are the reference's bit for bit) cropped to a box, the property at the final vertices
    lo = s.V.min(axis=0).astype(np.float64)
    hi = s.V.max(axis=0).astype(np.float64)
    planes = clip_box(lo + 0.25 * (hi - lo), hi - 0.3 * (hi - lo))
    Vw, Nw, Tw, outs = chain(s, planes)
    assert 100 < Tw.shape[0] < s.nT // 4 and sum(o.cut_vertices for o in outs) > 100
    V3, N3, T3, infos, P3 = g.extract_clipped(iso, planes, with_property=True)
    assert [tuple(i[n] for n in COUNTS) for i in infos] == [o.counts() for o in outs]
    assert np.array_equal(bits(V3.cpu().numpy()), bits(Vw)) and np.array_equal(T3.cpu().numpy().view(np.uint32), Tw)
    assert np.array_equal(bits(N3.cpu().numpy()), bits(Nw))
    assert np.array_equal(bits(P3.cpu().numpy()), bits(po.sample_property(Vw, r0, d, P)))
    void = g.extract_clipped(iso, [(1.0, 0.0, 0.0, -1e6)])  # nothing is left: empty tensors
    assert void[0].shape[0] == 0 and void[2].shape[0] == 0
    g.close()


# ---- the C API -----------------------------------------------------------------------------------------------------------------------

def clipped_surface(lib, M, iso, cl):
    S = lib.lib.MC33_calculate_clipped_isosurface(M, lib.real(iso), C.byref(cl) if cl is not None else None)
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
    """the oracle applied, plane after plane, to the reference's surface - the _nneg reference's for the _nneg flavour"""
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
        lo, hi = s.V.min(axis=0).astype(np.float64), s.V.max(axis=0).astype(np.float64)
        box, planes = cbox(lib, lo + 0.25 * (hi - lo), hi - 0.3 * (hi - lo))
        Vw, Nw, Tw, outs = chain(s, planes)
        assert 100 < Tw.shape[0] < s.nT // 4
        for attempt in range(2):  # the staging sets as they come, and as the first call left them
            got = clipped_surface(lib, M, iso, box)
            assert got is not None and (got.nV, got.nT) == (Vw.shape[0], Tw.shape[0]) and np.array_equal(got.T, Tw)
            assert np.array_equal(bits(got.V), bits(Vw)) and np.array_equal(bits(got.N), bits(Nw))
            assert np.all(got.color == po.DEFAULT_COLOR) and got.color.size == Vw.shape[0]
        # one oblique plane
        one = plane_of(s.V, "oblique")
        V1, N1, T1, _ = chain(s, [one])
        got = clipped_surface(lib, M, iso, cclip([one]))
        assert np.array_equal(bits(got.V), bits(V1)) and np.array_equal(bits(got.N), bits(N1)) and np.array_equal(got.T, T1)
        # colours: those of the FINAL vertices, the new ones included
        pal, plo, phi = palette(7), -2.5, 3.25
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), plo, phi) == 0
        painted = clipped_surface(lib, M, iso, box)
        assert np.array_equal(painted.color, po.color_vertices(Vw, r0, d, prop, pal, plo, phi)) and np.unique(painted.color).size > 2
        assert np.array_equal(bits(painted.V), bits(Vw)) and np.array_equal(painted.T, Tw)
        # n = 0 is calculate_isosurface, colours included
        plain = clipped_surface(lib, M, iso, cclip([]))
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        mine = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert np.array_equal(bits(plain.V), bits(mine.V)) and np.array_equal(bits(plain.N), bits(mine.N)) and np.array_equal(plain.T, mine.T)
        assert np.array_equal(plain.color, mine.color) and np.array_equal(bits(mine.V), bits(s.V))
        assert L.MC33_set_property_grid(M, None) == 0
        # a plane that removes everything: an empty surface, no failure
        void = clipped_surface(lib, M, iso, cclip([(1.0, 0.0, 0.0, -1e6)]))
        assert void is not None and (void.nV, void.nT) == (0, 0)
        # a null struct, too many planes and refused planes give NULL and leave the object alone; its surface is the reference's still
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        mine = lib.copy_surface(S)
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        nan, inf = float("nan"), float("inf")
        assert clipped_surface(lib, M, iso + 1.0, None) is None
        for cl in (cclip([one] * 7), cclip([(0.0, 0.0, 0.0, 1.0)]), cclip([one, (nan, 0.0, 1.0, 0.0)]), cclip([(1.0, 0.0, 0.0, inf)]), cclip([(1.0, -inf, 0.0, 0.0)])):
            assert clipped_surface(lib, M, iso + 1.0, cl) is None
            assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        L.free_surface_memory(S)
        assert np.array_equal(bits(mine.V), bits(s.V)) and np.array_equal(mine.T, s.T) and np.array_equal(bits(mine.N), bits(s.N))
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2


def test_c_api_on_an_inclined_grid(reflibs):
    """the planes are in the coordinates of the returned vertices: an inclined grid is clipped like any other"""
    data = fx.cos_field(24)[0]
    A = [[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    Ai = np.linalg.inv(np.array(A)).tolist()
    s = reflibs["f32"].isosurface(data, 0.0, inclined=(A, Ai))
    lib = capi()
    L = lib.lib
    G, keep = lib.make_grid(data, inclined=(A, Ai))
    M = L.create_MC33(G)
    assert M
    try:
        one = plane_of(s.V, "oblique")
        V1, N1, T1, outs = chain(s, [one])
        assert outs[0].cut_vertices > 20
        got = clipped_surface(lib, M, 0.0, cclip([one]))
        assert got is not None and np.array_equal(bits(got.V), bits(V1)) and np.array_equal(bits(got.N), bits(N1)) and np.array_equal(got.T, T1)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refuses_an_object_on_several_slabs(launcher):
    """MC33_HIP_DEVICES=0,0 in a fresh process, before the library is loaded: two slabs on one device (tests/capi_slab_refusals_worker.py)."""
    out = refusal(launcher, "clip")
    assert out["rc"] == 0 and "refused: 1 0" in out["stdout"], out
