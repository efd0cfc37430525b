"""GPU tests of the smoothing (include/mc33_hip.h: mc33hip_smooth_surface, mc33hip_vertex_normals; include/marching_cubes_33.h:
MC33_calculate_smoothed_isosurface; DeviceGrid.smooth / vertex_normals / extract_smoothed).

V and T come from the reference twin (oracle/_ref) or are synthetic; the expected arrays come from tests/smooth_oracle.py, the
definition in numpy.  oV and oN are compared bit for bit, the four counts exactly; nothing here has a tolerance.  Every output
of every call is canaried (tests/mesh_harness.py: CanariedCall)."""
import ctypes as C

import numpy as np
import pytest

from capi_slab_refusals import refusal
import fixtures as fx
import measure_oracle as mo
import property_oracle as po
import smooth_oracle as so
from mc33_c_library_amd.api import SurfaceSmoothing
from mc33_capi import MC33Lib, ref_path
from mesh_harness import FILL, SPARE, CanariedCall, bits, capi, c_palette, ctx, device_grid, info_of, palette, to_device  # noqa: F401 (ctx: the module's fixture)
from smooth_cases import TABLE, mesh

pytestmark = pytest.mark.gpu


class Call(CanariedCall):
    """one mc33hip_smooth_surface call; in_place: V is copied into the canaried oV first and oV == V"""

    def __init__(self, g, V, T, iterations=10, lam=0.5, mu=-0.53, pin=True, normals=True, in_place=False, change=None):
        import torch
        from mc33_c_library_amd.api import Smoothing
        super().__init__(g)
        self.nV, self.nT = V.shape[0], T.shape[0]
        self.oV, self.oN = self.room(self.nV, 3, V.dtype), (self.room(self.nV, 3, torch.float32) if normals else None)
        if in_place:
            self.oV[:self.nV] = V
            V = self.oV[:self.nV]
        a = Smoothing()
        a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), self.nV, self.nT
        a.iterations, a.lam, a.mu, a.pin_boundary = iterations, lam, mu, int(bool(pin))
        a.oV, a.oN = self.oV.data_ptr(), (self.oN.data_ptr() if normals else None)
        a.max_degree = a.isolated_vertices = a.boundary_vertices = a.invalid_triangles = 77
        self.keep = (V, T)
        self.call(g.lib.mc33hip_smooth_surface, a, change)
        self.info = (int(a.max_degree), int(a.isolated_vertices), int(a.boundary_vertices), int(a.invalid_triangles))

    def outputs(self):
        return [(self.oV, self.nV), (self.oN, self.nV)]

    def check(self, P, N=None, info=None):
        """bit for bit against the oracle"""
        self.equal_bits("oV", self.oV[:self.nV], P)
        if N is not None:
            self.equal_bits("oN", self.oN[:self.nV], N)
        if info is not None:
            assert self.info == tuple(info), (self.info, info)
        self.spare_intact()


_normals = {}


def smoothed(reflibs, name, pin):
    """the oracle's P and N of a fixture row, 10 iterations: computed once and left unchanged"""
    if (name, pin) not in _normals:
        s, P = mesh(reflibs, name)[4], mesh(reflibs, name)[6]
        n = so.vertex_normals(P[pin], s.T)
        n.setflags(write=False)
        _normals[(name, pin)] = n
    return mesh(reflibs, name)[6][pin], _normals[(name, pin)]


# ---- the five fixtures, float ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pin", [True, False], ids=["pinned", "free"])
@pytest.mark.parametrize("name", list(TABLE))
def test_fixtures_f32(reflibs, name, pin):
    data, r0, d, iso, s, A, _ = mesh(reflibs, name)
    P, N = smoothed(reflibs, name, pin)
    assert info_of(A)[:3] == TABLE[name][:3]
    g = device_grid(data, r0, d)
    V, T = to_device(s.V), to_device(s.T)
    first = Call(g, V, T, pin=pin)
    assert first.rc == 0, first.message
    first.check(P, N, info_of(A))
    again = Call(g, V, T, pin=pin)
    assert again.rc == 0 and again.all_bytes() == first.all_bytes(), "two calls on the same inputs differ"
    inp = Call(g, V, T, pin=pin, in_place=True)
    assert inp.rc == 0, inp.message
    inp.check(P, N, info_of(A))
    assert np.array_equal(bits(V.cpu().numpy()), bits(s.V)) and np.array_equal(T.cpu().numpy().view(np.uint32), s.T)  # the inputs are as they were
    # the Python layer, and the product's own extraction: its V, N, T are the reference's bit for bit
    V2, N2, info = g.smooth(V, T, pin_boundary=pin)
    assert np.array_equal(bits(V2.cpu().numpy()), bits(P)) and np.array_equal(bits(N2.cpu().numpy()), bits(N))
    assert tuple(info[k] for k in ("max_degree", "isolated_vertices", "boundary_vertices", "invalid_triangles")) == info_of(A)
    V3, N3, T3, cnt = g.extract_smoothed(iso, pin_boundary=pin)
    assert (cnt.nV, cnt.nT) == (s.nV, s.nT) and np.array_equal(T3.cpu().numpy().view(np.uint32), s.T)
    assert np.array_equal(bits(V3.cpu().numpy()), bits(P)) and np.array_equal(bits(N3.cpu().numpy()), bits(N))


@pytest.mark.parametrize("name", list(TABLE))
def test_skipped_passes_and_normals_alone(reflibs, name):
    data, r0, d, iso, s, A, _ = mesh(reflibs, name)
    g = device_grid(data, r0, d)
    V, T = to_device(s.V), to_device(s.T)
    N0 = so.vertex_normals(s.V, s.T)
    for in_place in (False, True):  # iterations == 0: V's bytes, the normals of V
        none = Call(g, V, T, iterations=0, in_place=in_place)
        assert none.rc == 0, none.message
        none.check(s.V, N0, info_of(A))
    alone = g.vertex_normals(V, T)
    assert np.array_equal(bits(alone.cpu().numpy()), bits(N0))
    # mu == 0 skips its pass: three passes of lambda, an odd number - in place they begin in the scratch rows
    P3 = so.smooth(s.V, s.T, 3, 0.5, 0.0, True, A=A)[0]
    for in_place in (False, True):
        odd = Call(g, V, T, iterations=3, mu=0.0, normals=False, in_place=in_place)  # (and oN == NULL)
        assert odd.rc == 0, odd.message
        odd.check(P3, None, info_of(A))
    P1 = so.smooth(s.V, s.T, 1, 0.5, -0.53, False, A=A)[0]
    one = Call(g, V, T, iterations=1, pin=False, in_place=True)
    assert one.rc == 0, one.message
    one.check(P1, so.vertex_normals(P1, s.T), info_of(A))
    if name == "sheet":  # property values are those at the unsmoothed vertices
        prop = fx.noise_f32(0, 77, shape=data.shape) * np.float32(1000.0)
        gp = device_grid(data, r0, d, prop)
        V4, N4, T4, cnt, P4 = gp.extract_smoothed(iso, with_property=True, iterations=1, pin_boundary=False)
        assert np.array_equal(bits(P4.cpu().numpy()), bits(po.sample_property(s.V, r0, d, prop)))
        assert np.array_equal(bits(V4.cpu().numpy()), bits(P1))


# ---- scan and row boundaries: synthetic meshes, no grid ------------------------------------------------------------------------------

# around a wave, a block, a tile of 4 per lane, and one round of a 256-tile top-level scan
SIZES = [0, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 262143, 262144, 262145]


@pytest.mark.parametrize("nV", SIZES)
def test_scan_and_row_boundaries(ctx, nV):
    fan = 1000 if nV == 4097 else 0  # degree 1000, 1000 incident triangles: a row longer than a wave, a block, any fixed buffer
    V, T = so.random_mesh(nV, 2000 + nV, fan)
    P, A = so.smooth(V, T, 2, 0.5, -0.53, True)
    N = so.vertex_normals(P, T)
    if fan:
        assert A.deg[0] >= 1000
    if nV > 1000:
        assert A.max_degree >= 12 and np.count_nonzero(A.boundary) > 0 and np.count_nonzero(~A.boundary & (A.deg > 0)) > 0
    dV, dT = to_device(V), to_device(T)
    call = Call(ctx, dV, dT, iterations=2)
    assert call.rc == 0, call.message
    call.check(P, N, info_of(A))
    free = Call(ctx, dV, dT, iterations=2, pin=False, in_place=True)
    assert free.rc == 0, free.message
    Pf = so.smooth(V, T, 2, 0.5, -0.53, False, A=A)[0]
    free.check(Pf, so.vertex_normals(Pf, T), info_of(A))


def test_no_triangles(ctx):
    import torch
    V = so.random_mesh(300, 5)[0]
    V[7, 0] = -0.0
    call = Call(ctx, to_device(V), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    assert call.rc == 0, call.message
    call.check(V, np.zeros((300, 3), np.float32), (0, 300, 0, 0))


# ---- the other builds ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["u8", "u8-corners", "f64"])
def test_other_sample_types(reflibs, case):
    dtype, n = case.split("-")[0], 40
    r0, d = mo.AWKWARD_R0, mo.AWKWARD_D
    if dtype == "f64":
        data, iso = fx.cos_field(n, dtype=np.float64)[0], 0.0
    else:
        data, iso = fx.cos_field_int(n, np.uint8, 40.0, 128.0), (128.5 if case == "u8" else 128.0)  # 128.0: corners equal the isovalue
    s = reflibs[dtype].isosurface(data, iso, r0, d)
    assert s.V.dtype == (np.float64 if dtype == "f64" else np.float32) and s.V.strides[0] == (24 if dtype == "f64" else 12)
    P, A = so.smooth(s.V, s.T, 10, 0.5, -0.53, True)
    if case == "u8":
        assert (s.nV, A.boundary_vertices) == (5856, 432)
    if case == "u8-corners":
        assert (s.nV, A.max_degree) == (5136, 10)
    N = so.vertex_normals(P, s.T)
    g = device_grid(data, r0, d)
    V, T = to_device(s.V), to_device(s.T)
    for in_place in (False, True):
        call = Call(g, V, T, in_place=in_place)
        assert call.rc == 0, call.message
        call.check(P, N, info_of(A))
    V3, N3, T3, cnt = g.extract_smoothed(iso)
    assert np.array_equal(T3.cpu().numpy().view(np.uint32), s.T)
    assert np.array_equal(bits(V3.cpu().numpy()), bits(P)) and np.array_equal(bits(N3.cpu().numpy()), bits(N))


# ---- invalid input -------------------------------------------------------------------------------------------------------------------

def test_a_triangle_outside_v_is_counted_not_read(reflibs):
    """One index set to nV: tested before anything is gathered through it.  V is the first nV rows of a tensor with 16 spare
    rows behind them, so that not even a wrong kernel could touch memory this test does not own."""
    import torch
    from mc33_c_library_amd.api import ERUNTIME
    data, r0, d, iso, s, A, _ = mesh(reflibs, "blobs")
    g = device_grid(data, r0, d)
    room = torch.zeros((s.nV + 16, 3), dtype=torch.float32, device="cuda")
    room[:s.nV] = to_device(s.V)
    V = room[:s.nV]
    badT = s.T.copy()
    badT[777, 1] = s.nV
    P, Ab = so.smooth(s.V, badT, 2, 0.5, -0.53, True)
    assert Ab.invalid_triangles == 1 and Ab.boundary_vertices == 3
    bad = Call(g, V, to_device(badT), iterations=2)
    assert bad.rc == ERUNTIME and "1 triangle " in bad.message, (bad.rc, bad.message)
    bad.check(P, so.vertex_normals(P, badT), info_of(Ab))  # the outputs are the oracle's without that triangle
    good = Call(g, V, to_device(s.T), iterations=2)  # the next call on the context succeeds
    assert good.rc == 0, good.message
    P2 = so.smooth(s.V, s.T, 2, 0.5, -0.53, True, A=A)[0]
    good.check(P2, so.vertex_normals(P2, s.T), info_of(A))


def test_invalid_arguments(reflibs):
    import torch
    from mc33_c_library_amd.api import EINVAL, Smoothing
    data, r0, d, iso, s, A, _ = mesh(reflibs, "sheet")
    g = device_grid(data, r0, d)
    V, T = to_device(s.V), to_device(s.T)
    nan = float("nan")
    cases = [dict(V=None), dict(T=None), dict(oV=None), dict(nV=1 << 32), dict(nT=1 << 32),
             dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5), dict(lam=nan), dict(mu=0.1), dict(mu=-1.5), dict(mu=nan), dict(iterations=1001),
             dict(oV=V.data_ptr() + 12), dict(oV=V.data_ptr() + 12 * (s.nV - 1)), dict(oV=T.data_ptr()), dict(oV=T.data_ptr() + 12 * (s.nT - 1)),
             dict(oN=V.data_ptr()), dict(oN=T.data_ptr() + 24)]
    for change in cases:
        call = Call(g, V, T, change=change)
        assert call.rc == EINVAL, (change, call.rc, call.message)
        call.spare_intact(written=False)  # every output still at its fill
    both = Call(g, V, T)  # oN meeting oV
    both.a.oN = both.oV.data_ptr() + 12 * (s.nV - 1)
    assert g.lib.mc33hip_smooth_surface(g.ctx, C.byref(both.a)) == EINVAL
    assert g.lib.mc33hip_smooth_surface(g.ctx, None) == EINVAL and g.lib.mc33hip_smooth_surface(None, C.byref(Smoothing())) == EINVAL
    assert np.array_equal(bits(V.cpu().numpy()), bits(s.V)) and np.array_equal(T.cpu().numpy().view(np.uint32), s.T)
    # the normals alone: null pointers, sizes, oN meeting an input
    oN = torch.empty((s.nV + SPARE, 3), dtype=torch.float32, device="cuda")
    oN.view(torch.uint8).fill_(FILL)
    vn = g.lib.mc33hip_vertex_normals
    args = (V.data_ptr(), s.nV, T.data_ptr(), s.nT, oN.data_ptr())
    for k, v in ((0, None), (2, None), (4, None), (1, 1 << 32), (3, 1 << 32), (4, V.data_ptr() + 12 * (s.nV - 1)), (4, T.data_ptr())):
        changed = list(args)
        changed[k] = v
        assert vn(g.ctx, *changed) == EINVAL, (k, v)
    assert np.all(oN.cpu().numpy().view(np.uint8) == FILL)
    assert vn(g.ctx, *args) == 0 and np.array_equal(bits(oN[:s.nV].cpu().numpy()), bits(so.vertex_normals(s.V, s.T)))
    assert np.all(oN[s.nV:].cpu().numpy().view(np.uint8) == FILL)
    assert Call(g, V, T).rc == 0  # the context is still good


# ---- the C API -----------------------------------------------------------------------------------------------------------------------

def smoothed_surface(lib, M, iso, sm):
    S = lib.lib.MC33_calculate_smoothed_isosurface(M, lib.real(iso), C.byref(sm) if sm is not None else None)
    if not S:
        return None
    try:
        if S.contents.nV:  # the object's public prefix mirrors the returned surface, as calculate_isosurface leaves it
            m, r = M.contents, S.contents
            assert (m.T, m.V, m.N, m.color, m.nT, m.capt, m.capv) == (r.T, r.V, r.N, r.color, r.nT, r.capt, r.capv)
        return lib.copy_surface(S)
    finally:
        lib.lib.free_surface_memory(S)


@pytest.mark.parametrize("name", ["quant", "sheet"])
def test_c_api(reflibs, name):
    data, r0, d, iso, s, A, _ = mesh(reflibs, name)
    lib = capi()
    L = lib.lib
    G, keep = lib.make_grid(data, r0, d)
    prop = fx.noise_f32(0, 79, shape=data.shape) * np.float32(10.0)
    Pg, keep2 = lib.make_grid(prop, r0, d)
    M = L.create_MC33(G)
    assert M
    try:
        for pin in (1, 0):
            P, N = smoothed(reflibs, name, bool(pin))
            got = smoothed_surface(lib, M, iso, SurfaceSmoothing(10, 0.5, -0.53, pin))
            assert got is not None and (got.nV, got.nT) == (s.nV, s.nT) and np.array_equal(got.T, s.T)
            assert np.array_equal(bits(got.V), bits(P)) and np.array_equal(bits(got.N), bits(N))
            assert np.all(got.color == po.DEFAULT_COLOR) and got.color.size == s.nV
            assert M.contents.iso == np.float32(iso) and M.contents.memoryfault == 0 and M.contents.nT == s.nT
        # colours: those of the unsmoothed surface
        pal, lo, hi = palette(7), -2.5, 3.25
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        painted = smoothed_surface(lib, M, iso, SurfaceSmoothing(10, 0.5, -0.53, 0))
        want_color = po.color_vertices(s.V, r0, d, prop, pal, lo, hi)
        assert np.array_equal(painted.color, want_color) and np.unique(painted.color).size > 2
        assert np.array_equal(bits(painted.V), bits(P)) and np.array_equal(bits(painted.N), bits(N))
        assert L.MC33_set_property_grid(M, None) == 0
        # a null struct and refused parameters give NULL; the object is still good, and its surface is the reference's
        assert smoothed_surface(lib, M, iso, None) is None
        for sm in (SurfaceSmoothing(10, 0.0, -0.53, 1), SurfaceSmoothing(10, 0.5, 0.53, 1), SurfaceSmoothing(1001, 0.5, -0.53, 1), SurfaceSmoothing(10, float("nan"), -0.53, 1)):
            assert smoothed_surface(lib, M, iso, sm) is None and M.contents.memoryfault == 0
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        mine = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert np.array_equal(bits(mine.V), bits(s.V)) and np.array_equal(mine.T, s.T) and np.array_equal(bits(mine.N), bits(s.N))
        # iterations 0: the extracted vertices with recomputed normals
        plain = smoothed_surface(lib, M, iso, SurfaceSmoothing(0, 0.5, -0.53, 1))
        assert np.array_equal(bits(plain.V), bits(s.V)) and np.array_equal(bits(plain.N), bits(so.vertex_normals(s.V, s.T)))
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2


def test_c_api_nneg_flavour():
    """the nneg reference's own surface: two indices exchanged and N negated, so the recomputed normals agree in sign with its N"""
    field, iso, _ = mo.FIXTURES["sheet"]
    data, r0, d = field()
    s = MC33Lib(ref_path("f32", nneg=True), "f32").isosurface(data, iso, r0, d)
    P, A = so.smooth(s.V, s.T, 10, 0.5, -0.53, True)
    N = so.vertex_normals(P, s.T)
    lib = capi(nneg=True)
    L = lib.lib
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    assert M
    try:
        got = smoothed_surface(lib, M, iso, SurfaceSmoothing(10, 0.5, -0.53, 1))
        assert np.array_equal(got.T, s.T) and np.array_equal(bits(got.V), bits(P)) and np.array_equal(bits(got.N), bits(N))
        plain = smoothed_surface(lib, M, iso, SurfaceSmoothing(0, 0.5, -0.53, 1))
        dots = (plain.N.astype(np.float64) * s.N).sum(1)
        print("nneg: smallest dot product of the recomputed normals with the emitted N %.4f" % dots.min())
        assert dots.min() > 0.0
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refuses_an_object_on_several_slabs(launcher):
    """MC33_HIP_DEVICES=0,0 in a fresh process, before the library is loaded: two slabs on one device (tests/capi_slab_refusals_worker.py)."""
    out = refusal(launcher, "smooth")
    assert out["rc"] == 0 and "refused: 1 0" in out["stdout"], out
