"""GPU tests of the caps at the grid faces (include/mc33_hip.h: mc33hip_cap_surface; include/marching_cubes_33.h:
MC33_calculate_capped_isosurface; DeviceGrid.cap / extract_capped).

Every case of tests/cap_cases.py is extracted on the device and capped there; the expected arrays come from tests/cap_oracle.py
run on the very mesh that was downloaded.  Everything is compared bit for bit - V, N, T, both attributes and all counts; nothing
here has a tolerance but the volume, whose bound is measure_oracle's.  The call works in place, so V, N, T and the attributes sit
in canaried tensors (tests/mesh_harness.py: CanariedCall) whose first rows hold the surface."""
import ctypes as C

import numpy as np
import pytest

import cap_cases as cc
import cap_oracle as co
import measure_oracle as mo
from cap_cases import ALL
from mc33_c_library_amd.api import SurfaceCap, SurfaceCapInfo
from mesh_harness import CanariedCall, bits, capi, device_grid, to_device

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ERUNTIME = -1, -4, -5
_grids, _meshes = {}, {}


def grid(name):
    """the case and a context on its grid, made once per case and module"""
    if name not in _grids:
        c = cc.case(name)
        _grids[name] = (c, device_grid(c.data, r0=c.r0, d=c.d))
    return _grids[name]


def extracted(name):
    """(V, N, T) of the case as the device extracts it, on the host; the `hole` case without its NaN triangles"""
    if name not in _meshes:
        c, g = grid(name)
        if c.zr:  # a surface of its own over the planes of the box: a context on those planes (a z range of the whole grid's context
            data, r0 = cc.extraction(c)  # is a slab's piece, whose triangles name vertices of the slice below)
            gz = device_grid(data, r0=r0, d=c.d)
            V, N, T, cnt = gz.extract(c.iso)
            gz.close()
        else:
            V, N, T, cnt = g.extract(c.iso)
        V, N, T = V.cpu().numpy(), N.cpu().numpy(), T.cpu().numpy().view(np.uint32)
        if name == "hole":
            T = cc.without_nonfinite(V, T)
        for a in (V, N, T):
            a.setflags(write=False)
        _meshes[name] = (V, N, T)
    return _meshes[name]


def expected(name, invert=False, attrs=(), modes=()):
    c, _ = grid(name)
    V, N, T = extracted(name)
    return co.cap(V, N, T, c.data, c.iso, c.r0, c.d, c.lo, c.hi, invert=invert, attrs=attrs, attr_modes=modes)


class Call(CanariedCall):
    """one mc33hip_cap_surface call on tensors of capV / capT rows (and SPARE canaried ones) whose first rows hold the surface"""

    def __init__(self, g, c, V, N, T, capV, capT, invert=False, attrs=(), modes=(), change=None):
        import torch
        from mc33_c_library_amd.api import Capping
        super().__init__(g)
        self.nV, self.nT, self.inputs, self.counts = V.shape[0], T.shape[0], (V, N, T, attrs), (0, 0)
        # (a call with too little room still reads the whole surface: the tensors hold it whatever capacity the call is told)
        rowsV, rowsT = self.nV, self.nT
        self.bV, self.bN = self.room(max(capV, rowsV), 3, torch.float64 if V.dtype == np.float64 else torch.float32), self.room(max(capV, rowsV), 3, torch.float32)
        self.bT = self.room(max(capT, rowsT), 3, torch.int32)
        self.bA = [self.room(max(capV, rowsV), 0, torch.int32) for _ in attrs]
        if rowsV:
            self.bV[:rowsV].copy_(to_device(V[:rowsV]))
            self.bN[:rowsV].copy_(to_device(N[:rowsV]))
            for b, x in zip(self.bA, attrs):
                b[:rowsV].copy_(to_device(x.view(np.uint32)[:rowsV]))
        if rowsT:
            self.bT[:rowsT].copy_(to_device(T[:rowsT]))
        self.before = self.all_bytes()
        a = Capping()
        a.V, a.N, a.T, a.nV, a.nT, a.capV, a.capT = self.bV.data_ptr(), self.bN.data_ptr(), self.bT.data_ptr(), self.nV, self.nT, capV, capT
        a.iso, a.invert = float(c.iso), int(invert)
        a.lo, a.hi = (C.c_uint * 3)(*c.lo), (C.c_uint * 3)(*c.hi)
        for k, b in enumerate(self.bA):
            a.attr[k], a.attr_mode[k] = b.data_ptr(), int(modes[k])
        a.n_attr = len(attrs)
        self.call(g.lib.mc33hip_cap_surface, a, change)
        self.counts = tuple(int(getattr(a, n)) for n in co.COUNTS)

    def outputs(self):
        return [(self.bV, self.counts[0]), (self.bN, self.counts[0]), (self.bT, self.counts[1])] + [(b, self.counts[0]) for b in self.bA]

    def check(self, want):
        """bit for bit against the oracle; the canaries behind nV_out / nT_out still hold FILL"""
        assert self.counts == want.counts(), (dict(zip(co.COUNTS, self.counts)), dict(zip(co.COUNTS, want.counts())))
        self.equal_bits("V", self.bV[:want.nV_out], want.V)
        self.equal_bits("N", self.bN[:want.nV_out], want.N)
        self.equal_bits("T", self.bT[:want.nT_out], want.T)
        for k, b in enumerate(self.bA):
            self.equal_bits("attribute %d" % k, b[:want.nV_out], want.attrs[k])
        self.spare_intact()

    def untouched(self):
        assert self.all_bytes() == self.before, "a refused call wrote to its arrays"


def attributes(nV):
    return (np.random.default_rng(5).standard_normal(nV).astype(np.float32), np.random.default_rng(6).integers(1, 1 << 32, nV, dtype=np.uint64).astype(np.uint32))


MODES = (co.F32, co.WORD)


@pytest.mark.parametrize("name", ALL + cc.LARGE)
def test_cases_bit_for_bit(name):
    c, g = grid(name)
    V, N, T = extracted(name)
    A = attributes(V.shape[0])
    want = expected(name, attrs=A, modes=MODES)
    print("    %s: %r" % (name, dict(zip(co.COUNTS, want.counts()))))
    assert (want.closed == 1) == (name not in cc.OPEN)
    first = Call(g, c, V, N, T, want.nV_out, want.nT_out, attrs=A, modes=MODES)  # exact capacity
    assert first.rc == 0, first.message
    first.check(want)
    # the rows of the surface are what they were
    assert first.host(first.bV[:V.shape[0]]).tobytes() == V.tobytes() and first.host(first.bT[:T.shape[0]]).view(np.uint32).tobytes() == T.tobytes()
    again = Call(g, c, V, N, T, want.nV_out + 5, want.nT_out + 3, attrs=A, modes=MODES)  # room to spare: the rows behind the counted ones stay FILL
    assert again.rc == 0, again.message
    again.check(want)
    if name in cc.LARGE:
        assert want.cap_triangles > 4 * 1024 and want.cap_vertices > 2 * 1024 and T.shape[0] > 2 * 256


@pytest.mark.parametrize("name", ["dome", "quant", "saddle", "sub", "dome_f64"])
def test_invert(name):
    c, g = grid(name)
    V, N, T = extracted(name)
    want = expected(name, invert=True)
    plain = expected(name)
    assert want.solid_above == 0 and plain.solid_above == 1
    call = Call(g, c, V, N, T, want.nV_out, want.nT_out, invert=True)
    assert call.rc == 0, call.message
    call.check(want)
    assert np.array_equal(call.host(call.bT[:T.shape[0]]).view(np.uint32), T[:, [0, 2, 1]])


def test_capacity_and_the_size_query():
    c, g = grid("dome")
    V, N, T = extracted("dome")
    want = expected("dome", invert=True)
    for capV, capT in ((want.nV_out - 1, want.nT_out), (want.nV_out, want.nT_out - 1), (0, 0)):
        call = Call(g, c, V, N, T, capV, capT, invert=True)
        assert call.rc == ECAPACITY and call.counts == want.counts(), (capV, capT, call.rc, call.message)
        call.untouched()
    call = Call(g, c, V, N, T, want.nV_out, want.nT_out, invert=True)
    assert call.rc == 0
    call.check(want)


def test_refusals():
    c, g = grid("dome")
    V, N, T = extracted("dome")
    want = expected("dome")
    nan = float("nan")
    for change in ({"lo": (3, 0, 0), "hi": (3, 10, 8)}, {"lo": (0, 5, 0), "hi": (12, 4, 8)}, {"hi": (13, 10, 8)}, {"hi": (12, 10, 9)}, {"iso": nan}, {"n_attr": 3},
                   {"V": None}, {"T": None}, {"N": None}):
        call = Call(g, c, V, N, T, want.nV_out, want.nT_out, change=change)
        assert call.rc == EINVAL, (change, call.rc, call.message)
        call.untouched()
    # an inclined context
    gi = device_grid(c.data, r0=c.r0, d=c.d)
    gi.set_inclined([[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, -0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    call = Call(gi, c, V, N, T, want.nV_out, want.nT_out)
    assert call.rc == EINVAL and "orthogonal" in call.message
    call.untouched()
    gi.close()
    # a z-slab context: planes 2 .. 6 of the grid
    from mc33_c_library_amd import DeviceGrid
    gs = DeviceGrid(to_device(c.data)[2:7].contiguous(), nz_total=c.data.shape[0] - 1, plane0=2)
    call = Call(gs, c, V, N, T, want.nV_out, want.nT_out)
    assert call.rc == EINVAL and "slab" in call.message
    call.untouched()
    gs.close()


def test_invalid_triangles_are_counted_not_read():
    c, g = grid("corner")
    V, N, T = extracted("corner")
    T2 = np.concatenate([T[:7], np.array([[0, 1, V.shape[0]], [0xFFFFFFFF, 2, 3]], np.uint32), T[7:]])
    want = co.cap(V, N, T2, c.data, c.iso, c.r0, c.d, c.lo, c.hi)
    assert want.invalid_triangles == 2 and want.closed == 1
    call = Call(g, c, V, N, T2, want.nV_out, want.nT_out)
    assert call.rc == ERUNTIME and "2 triangles" in call.message
    call.check(want)


def test_the_result_goes_through_the_other_passes():
    c, g = grid("dome")
    V, N, T, info = g.extract_capped(c.iso)
    want = expected("dome")
    assert tuple(info[n] for n in co.COUNTS) == want.counts()
    assert np.array_equal(bits(V.cpu().numpy()), bits(want.V)) and np.array_equal(T.cpu().numpy().view(np.uint32), want.T)
    assert np.array_equal(bits(N.cpu().numpy()), bits(want.N))
    t = g.topology(T, V.shape[0])
    assert t.closed and t.manifold and t.oriented and t.boundary_edges == 0 and t.referenced_vertices == V.shape[0]
    m = g.measure(V, T)
    ref = mo.measure(want.V, want.T, c.r0, c.d, c.data.shape)
    assert abs(m.volume - ref.volume) <= ref.volume_bound and abs(m.area - ref.area) <= ref.area_bound and m.volume > 0.0
    sm = g.smooth(V, T, iterations=2)
    assert sm[0].shape == V.shape and bool(sm[0].isfinite().all())
    sp = g.simplify(V, T, (2.0, 2.0, 2.0))
    assert 0 < sp[0].shape[0] < V.shape[0]
    cl = g.clip(V, N, T, (1.0, 0.0, 0.0, -6.0))
    assert 0 < cl[2].shape[0]
    assert g.section(V, T, (1.0, 0.0, 0.0, -6.25)).P.shape[0] > 0
    # a z range: the box is the range's
    from mc33_c_library_amd.api import Range
    cs, gs = grid("sub")
    Vs, Ns, Ts, infos = gs.extract_capped(cs.iso, Range(cs.zr[0], cs.zr[1], 0, 0))  # (the method extracts over the planes of the range)
    ws = expected("sub")
    assert tuple(infos[n] for n in co.COUNTS) == ws.counts() and np.array_equal(bits(Vs.cpu().numpy()), bits(ws.V)) and np.array_equal(Ts.cpu().numpy().view(np.uint32), ws.T)
    # attributes through the Python method: NaN in a float tensor, 0 in a word tensor
    A = attributes(extracted("dome")[0].shape[0])
    Vd, Nd, Td = (to_device(x) for x in extracted("dome"))
    out = g.cap(Vd, Nd, Td, c.iso, attrs=(to_device(A[0]), to_device(A[1])))
    wa = expected("dome", attrs=A, modes=MODES)
    assert np.array_equal(out[3][0].cpu().numpy().view(np.uint32), wa.attrs[0]) and np.array_equal(out[3][1].cpu().numpy().view(np.uint32), wa.attrs[1])
    assert np.array_equal(Td.cpu().numpy().view(np.uint32), extracted("dome")[2])  # the input is left alone


def test_call_order():
    """cap, another extraction on the same context, cap again: the same bits"""
    c, g = grid("noise")
    V, N, T = extracted("noise")
    want = expected("noise")
    first = Call(g, c, V, N, T, want.nV_out, want.nT_out)
    g.extract(0.5)
    g.topology(to_device(T), V.shape[0])
    second = Call(g, c, V, N, T, want.nV_out, want.nT_out)
    assert first.rc == 0 and second.rc == 0 and first.all_bytes() == second.all_bytes()
    second.check(want)


# ---- the C API -----------------------------------------------------------------------------------------------------------------------

def capped_surface(lib, M, iso, options, info):
    S = lib.lib.MC33_calculate_capped_isosurface(M, lib.real(iso), C.byref(options) if options is not None else None, C.byref(info) if info is not None else None)
    if not S:
        return None
    try:
        m, r = M.contents, S.contents
        assert (m.nV, m.nT, m.memoryfault, m.iso) == (0, r.nT, 0, np.float32(iso))  # as calculate_isosurface leaves them
        return lib.copy_surface(S)
    finally:
        lib.lib.free_surface_memory(S)


@pytest.mark.parametrize("name", ["dome", "quant"])
def test_c_api(name):
    c, g = grid(name)
    lib = capi(c.dtype)
    L = lib.lib
    G, keep = lib.make_grid(c.data, c.r0, c.d)
    M = L.create_MC33(G)
    assert M
    try:
        V, N, T, pinfo = g.extract_capped(c.iso)
        for attempt in range(2):  # the staging set as it comes, and as the first call left it
            info = SurfaceCapInfo()
            got = capped_surface(lib, M, c.iso, None if attempt else SurfaceCap((C.c_uint * 3)(*c.lo), (C.c_uint * 3)(*c.hi), 0), info)
            assert got is not None and (got.nV, got.nT) == (V.shape[0], T.shape[0]) and got.color.size == got.nV
            assert np.array_equal(bits(got.V), bits(V.cpu().numpy())) and np.array_equal(bits(got.N), bits(N.cpu().numpy()))
            assert np.array_equal(got.T, T.cpu().numpy().view(np.uint32))
            assert (info.nV, info.nT) == (got.nV, got.nT)
            assert tuple(getattr(info, n) for n in co.COUNTS[2:8]) == tuple(pinfo[n] for n in co.COUNTS[2:8]) and (info.solid_above, info.closed) == (pinfo["solid_above"], pinfo["closed"])
        assert capped_surface(lib, M, c.iso, None, None).nV == V.shape[0]
        Vi, Ni, Ti, iinfo = g.extract_capped(c.iso, invert=True)
        info = SurfaceCapInfo()
        inv = capped_surface(lib, M, c.iso, SurfaceCap((C.c_uint * 3)(0, 0, 0), (C.c_uint * 3)(0, 0, 0), 1), info)
        assert np.array_equal(bits(inv.V), bits(Vi.cpu().numpy())) and np.array_equal(inv.T, Ti.cpu().numpy().view(np.uint32)) and np.array_equal(bits(inv.N), bits(Ni.cpu().numpy()))
        assert info.solid_above == 0 and info.closed == iinfo["closed"]
        # a refused box gives NULL and leaves the object alone
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault)
        bad = SurfaceCap((C.c_uint * 3)(0, 0, 0), (C.c_uint * 3)(c.hi[0] + 1, c.hi[1], c.hi[2]), 0)
        assert capped_surface(lib, M, c.iso + 1.0, bad, None) is None and (M.contents.iso, M.contents.nT, M.contents.memoryfault) == before
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_nneg_flavour_caps_below():
    """the _nneg library stores the opposite winding: its solid side is below, and the capped surface is closed all the same"""
    import topology_oracle as to
    c = cc.case("dome")
    lib = capi("f32", nneg=True)
    L = lib.lib
    G, keep = lib.make_grid(c.data, c.r0, c.d)
    M = L.create_MC33(G)
    assert M
    try:
        S = L.calculate_isosurface(M, lib.real(c.iso))
        assert S
        s = lib.copy_surface(S)
        L.free_surface_memory(S)
        want = co.cap(s.V, s.N, s.T, c.data, c.iso, c.r0, c.d, c.lo, c.hi, normal_neg=True)
        info = SurfaceCapInfo()
        got = capped_surface(lib, M, c.iso, None, info)
        assert (info.solid_above, info.closed, got.nV, got.nT) == (0, 1, want.nV_out, want.nT_out)
        assert np.array_equal(bits(got.V), bits(want.V)) and np.array_equal(got.T, want.T) and np.array_equal(bits(got.N), bits(want.N))
        e = to.EdgeTable(got.T, got.nV)
        assert not e.boundary.any() and not e.nonmanifold.any() and not e.misoriented.any()
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
