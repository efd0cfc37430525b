"""GPU tests of the curvature pass (include/mc33_hip.h: mc33hip_curvature_vertices / mc33hip_color_values;
include/marching_cubes_33.h: MC33_set_color_source / MC33_isosurface_curvature).

V is made up (tests/curvature_cases.py) unless a test says otherwise; the expected values come from tests/curvature_oracle.py, the
definition in numpy float64.  Every output sits in a canaried tensor and is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import curvature_cases as cc
import curvature_oracle as co
import fixtures as fx
import layouts
import property_oracle as po
from mc33_c_library_amd.api import IsosurfaceCurvature
from mesh_harness import CanariedCall, bits, c_palette, capi, device_grid, palette, to_device

pytestmark = pytest.mark.gpu

MEMBERS = ("oMean", "oGauss", "oK1", "oK2")
R0, D = cc.AWKWARD_R0, cc.AWKWARD_D


def one_nan(a):
    """a float array with every NaN replaced by the one quiet NaN 0x7FC00000.  IEEE 754 leaves the sign and payload of the NaN that
    an invalid operation makes (0 / 0, inf - inf) to the implementation - the host's is negative, the device's positive - and which
    operand's payload survives an operation on two NaNs: that a value is NaN is part of the definition, which NaN is not."""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a


class CurvatureCall(CanariedCall):
    """mc33hip_curvature_vertices over V with the outputs named in `which`, each in a canaried tensor; every other bit of every
    output is compared, NaNs as one_nan leaves them"""

    def host(self, t):
        return one_nan(t.cpu().numpy())

    def __init__(self, g, V, sign=1, which=co.NAMES, change=None):
        import torch
        from mc33_c_library_amd.api import Curvature
        super().__init__(g)
        self.nV = V.shape[0]
        self.dV = to_device(V) if self.nV else None
        self.out = {k: self.room(self.nV, 0, torch.float32) for k in which}
        a = Curvature()
        a.dV, a.nV, a.sign = (self.dV.data_ptr() if self.nV else None), self.nV, sign
        for k, m in zip(co.NAMES, MEMBERS):
            setattr(a, m, self.out[k].data_ptr() if k in self.out else None)
        self.call(g.lib.mc33hip_curvature_vertices, a, change)

    def outputs(self):
        return [(t, self.nV) for t in self.out.values()]

    def summary(self):
        return co.Summary(tuple(self.a.lo), tuple(self.a.hi), int(self.a.finite), int(self.a.undefined))

    def check(self, want):
        """the arrays against the oracle's, the summary against the oracle's summary of all four, the canaries"""
        assert self.rc == 0, self.message
        for q, k in enumerate(co.NAMES):
            if k in self.out:
                raw = self.out[k][:self.nV].cpu().numpy()
                print("%s: %d NaNs, %d of them other bits than the oracle's" % (k, np.isnan(raw).sum(), np.count_nonzero(bits(raw) != bits(want[q]))))
                self.equal_bits(k, self.out[k][:self.nV], one_nan(want[q]))
        assert self.summary() == co.summary(want), (self.summary(), co.summary(want))
        self.spare_intact()


def grid_and_vertices(dtype, grid, seed=0):
    shape = cc.SHAPES[grid]
    return cc.field(dtype, shape, seed), cc.made_up_vertices(shape, R0, D, cc.real_of(dtype), seed)


@pytest.mark.parametrize("dtype,grid", [(t, g) for t in ("f32", "f64") for g in cc.SHAPES] + [(t, "9x8x7") for t in ("u8", "u16", "u32")])
def test_made_up_vertices_are_bit_identical(dtype, grid):
    """every node, edge points, cell centres, points outside every face, NaN rows: 1, 2, 4 and 8 nodes mixed in every wave"""
    F, V = grid_and_vertices(dtype, grid)
    g = device_grid(F, R0, D)
    want = co.curvature(V, R0, D, F)
    assert co.summary(want).undefined >= 4 and co.summary(want).finite > V.shape[0] // 2
    CurvatureCall(g, V).check(want)
    CurvatureCall(g, V, sign=-1).check(co.curvature(V, R0, D, F, sign=-1))
    g.close()


@pytest.mark.parametrize("dtype", ["f32", "f64", "u8", "u16", "u32"])
def test_adopted_buffer_with_padding_and_an_unaligned_base(dtype):
    """pitch and slice larger than the grid, the base off every alignment; what lies between the rows is NaN (all bits set for
    integers), so a read outside a row's npx points shows in the output"""
    from mc33_c_library_amd import DeviceGrid
    F, V = grid_and_vertices(dtype, "9x8x7", seed=2)
    flat, lay = cc.padded(F, "all")
    view = layouts.device_view(layouts.to_device(flat), F.shape, lay)
    g = DeviceGrid(view, r0=R0, d=D)
    CurvatureCall(g, V).check(co.curvature(V, R0, D, F))
    g.close()


def test_wave_divergence():
    """64 vertices - one wave - that alternate between x-, y- and z-edges and cell interiors, in a geometry that inverts exactly:
    lanes with two nodes beside lanes with eight"""
    shape = cc.SHAPES["9x8x7"]
    F = cc.field("f32", shape, seed=3)
    V = cc.divergent_vertices(shape, cc.EXACT_R0, cc.EXACT_D, np.float32)
    _, _, f = po.grid_coordinates(V, cc.EXACT_R0, cc.EXACT_D, shape)
    assert (f != 0).sum(axis=1).tolist() == [1, 1, 1, 3] * 16 and [int(np.argmax(r)) for r in (f != 0)[:3]] == [0, 1, 2]
    g = device_grid(F, cc.EXACT_R0, cc.EXACT_D)
    CurvatureCall(g, V).check(co.curvature(V, cc.EXACT_R0, cc.EXACT_D, F))
    g.close()


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_made_up_vertices_in_a_geometry_that_inverts_exactly(dtype):
    """the same made-up vertices where a node has no live axis, an edge point one, a cell centre three"""
    F, _ = grid_and_vertices(dtype, "9x8x7", seed=4)
    V = cc.made_up_vertices(F.shape, cc.EXACT_R0, cc.EXACT_D, cc.real_of(dtype), seed=4)
    _, _, f = po.grid_coordinates(V, cc.EXACT_R0, cc.EXACT_D, F.shape)
    live = np.bincount((f != 0).sum(axis=1), minlength=4)
    assert live[0] >= 9 * 8 * 7 and live[1] > 1000 and live[3] > 500, live
    g = device_grid(F, cc.EXACT_R0, cc.EXACT_D)
    CurvatureCall(g, V).check(co.curvature(V, cc.EXACT_R0, cc.EXACT_D, F))
    g.close()


def test_extracted_surface_summary_and_null_outputs():
    """the cos_field(48) surface as extract() returns it, with both signs; k1 >= k2 and their mean; subsets of NULL outputs"""
    data, r0, d = fx.cos_field(48)
    g = device_grid(data, r0, d)
    V = g.extract(0.0)[0].cpu().numpy()
    assert V.shape[0] == 8424
    for sign in (1, -1):
        want = co.curvature(V, r0, d, data, sign)
        call = CurvatureCall(g, V, sign)
        call.check(want)
        mean, gauss, k1, k2 = (call.host(call.out[k][:call.nV]) for k in co.NAMES)
        both = np.isfinite(k1) & np.isfinite(k2)
        assert both.sum() > 8000 and (k1[both] >= k2[both]).all()
        # 0.5 * (k1 + k2) against mean.  k1 and k2 are mean + r and mean - r rounded to float, each off by half an ulp of ITS
        # OWN size at most, and mean by half an ulp of its own: the half sum is within one ulp of the largest of the three.  (On
        # this surface mean is near 0 and k1 near -k2, so an ulp of mean itself is not a bound that rounding can keep.)
        half = 0.5 * (k1[both].astype(np.float64) + k2[both].astype(np.float64))
        size = np.maximum(np.maximum(np.abs(k1[both]), np.abs(k2[both])), np.abs(mean[both]))
        off = np.abs(half - mean[both].astype(np.float64))
        print("sign %+d: |0.5 (k1 + k2) - mean| above one ulp of mean at %d of %d vertices, above one ulp of the largest at %d" % (
            sign, np.count_nonzero(off > np.spacing(np.abs(mean[both]))), both.sum(), np.count_nonzero(off > np.spacing(size))))
        assert (off <= np.spacing(size)).all()
        whole = {k: call.host(call.out[k]).tobytes() for k in co.NAMES}
        for which in (("mean",), ("gauss", "k2"), ("k1",), ()):
            part = CurvatureCall(g, V, sign, which)
            assert part.rc == 0 and part.summary() == call.summary()
            for k in which:
                assert part.host(part.out[k]).tobytes() == whole[k], k
        again = CurvatureCall(g, V, sign)
        assert again.all_bytes() == call.all_bytes() and again.summary() == call.summary()
    # the Python method: the same tensors and summary
    res = g.curvature(to_device(V), which=("mean", "k2"))
    want = co.curvature(V, r0, d, data)
    assert np.array_equal(bits(one_nan(res.mean.cpu().numpy())), bits(one_nan(want[0]))) and np.array_equal(bits(one_nan(res.k2.cpu().numpy())), bits(one_nan(want[3])))
    assert res.gauss is None
    s = co.summary(want)
    assert tuple(res.lo[k] for k in co.NAMES) == s.lo and tuple(res.hi[k] for k in co.NAMES) == s.hi and (res.finite, res.undefined) == (s.finite, s.undefined)
    # no vertices: success, nothing touched
    empty = CurvatureCall(g, V[:0])
    assert empty.rc == 0 and empty.summary() == co.Summary((np.inf,) * 4, (-np.inf,) * 4, 0, 0)
    empty.spare_intact(written=False)
    g.close()


def test_refusals_leave_the_outputs_untouched():
    from mc33_c_library_amd import DeviceGrid
    from mc33_c_library_amd.api import EINVAL
    F, V = grid_and_vertices("f32", "5x4x3")

    def refused(g, word, **kw):
        call = CurvatureCall(g, V, **kw)
        assert call.rc == EINVAL and word in call.message, (call.rc, call.message)
        call.spare_intact(written=False)

    g = DeviceGrid(to_device(F), nz_total=F.shape[0] + 3, plane0=1, r0=R0, d=D)   # planes 1 .. 3 of a grid of 6 cell slices
    refused(g, "z-slab")
    g.close()
    g = device_grid(F, R0, D)
    refused(g, "sign", sign=0)
    refused(g, "sign", sign=2)
    refused(g, "null", change={"dV": None})
    A, Ai = fx.cell_matrices(80.0, 75.0, 100.0)
    g.set_inclined(A, Ai, True)
    refused(g, "orthogonal")
    g.set_inclined(None)
    CurvatureCall(g, V).check(co.curvature(V, R0, D, F))
    g.close()
    for shape in ((2, 4, 5), (3, 2, 5), (3, 4, 2)):   # one cell on z, on y, on x
        g = device_grid(cc.field("f32", shape), R0, D)
        refused(g, "2 cells")
        g.close()


@pytest.mark.parametrize("n", [2, 7, 256])
def test_color_values_of_the_sampled_property_equal_color_vertices(n):
    """the property tests' fixture: both clamps hit, NaNs planted in the property"""
    import torch
    from mc33_c_library_amd.api import MC33Error, EINVAL
    data, iso = fx.noise_f32(0, 9, shape=(26, 31, 40)), 0.05
    P = fx.noise_f32(0, 78, shape=data.shape) * np.float32(10.0)
    P.reshape(-1)[::97] = np.nan
    g = device_grid(data, R0, D, P)
    V = g.extract(iso)[0]
    assert V.shape[0] > 40000
    pal, lo, hi = palette(n), -2.5, 3.25
    val = g.sample_property(V)
    want = g.color_vertices(V, pal, lo, hi).cpu().numpy()
    assert len(set(want.tolist())) == n + 1
    got = g.color_values(val, pal, lo, hi).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got, po.color_values(val.cpu().numpy(), pal, lo, hi))
    assert np.array_equal(g.color_values(val, pal, lo, hi, nan_color=0x01020304).cpu().numpy(), po.color_values(val.cpu().numpy(), pal, lo, hi, default=0x01020304))
    for bad_pal, blo, bhi in ((pal[:1], lo, hi), (palette(257), lo, hi), (pal, hi, lo), (pal, lo, lo), (pal, float("nan"), hi), (pal, lo, float("nan"))):
        with pytest.raises(MC33Error) as e:
            g.color_values(val, bad_pal, blo, bhi)
        assert e.value.code == EINVAL
    # no property grid, an inclined context: served all the same; the canaries behind the counted words stay
    g.detach_property()
    A, Ai = fx.cell_matrices(80.0, 75.0, 100.0)
    g.set_inclined(A, Ai, True)
    assert np.array_equal(g.color_values(val, pal, lo, hi).cpu().numpy(), want)
    call = CanariedCall(g)
    out = call.room(val.shape[0], 0, torch.int32)
    assert g.lib.mc33hip_color_values(g.ctx, C.c_void_p(val.data_ptr()), val.shape[0], c_palette(pal), n, lo, hi, int(po.DEFAULT_COLOR), C.c_void_p(out.data_ptr())) == 0
    assert g.lib.mc33hip_synchronize(g.ctx) == 0
    assert np.array_equal(out[:val.shape[0]].cpu().numpy(), want) and np.all(out[val.shape[0]:].cpu().numpy().view(np.uint8) == 0x55)
    g.close()


# ---- the C API -----------------------------------------------------------------------------------------------------------

def one_surface(lib, M, iso):
    S = lib.lib.calculate_isosurface(M, lib.real(iso))
    assert S, "calculate_isosurface returned NULL"
    try:
        return lib.copy_surface(S)
    finally:
        lib.lib.free_surface_memory(S)


def c_field(dtype):
    if dtype == "f32":
        return fx.cos_field(40)[0], 0.25
    return fx.cos_field_int(40, np.uint16, 10000.0, 32768.0), 34000.5


def as_tuple(out):
    return (out.nV, out.nT, tuple(out.lo), tuple(out.hi), out.finite, out.undefined, out.total_mean, out.total_gauss)


@pytest.mark.parametrize("dtype,nneg", [("f32", False), ("u16", False), ("f32", True)])
def test_c_api_colours_and_struct(dtype, nneg):
    lib = capi(dtype, nneg)
    L = lib.lib
    data, iso = c_field(dtype)
    sign = -1 if nneg else 1
    pal = palette(9)
    G, keep = lib.make_grid(data, R0, D)
    M = L.create_MC33(G)
    assert M
    try:
        plain = one_surface(lib, M, iso)
        assert plain.nV > 1000 and np.all(plain.color == po.DEFAULT_COLOR)
        val = co.curvature(plain.V, R0, D, data, sign)
        summ = co.summary(val)
        lo, hi = float(np.nanpercentile(val[0], 20)), float(np.nanpercentile(val[0], 80))
        assert L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        assert np.all(one_surface(lib, M, iso).color == po.DEFAULT_COLOR)   # a map alone paints nothing
        assert L.MC33_set_color_source(M, 5) == -1 and L.MC33_set_color_source(M, -1) == -1
        for source in (1, 2, 3, 4):
            assert L.MC33_set_color_source(M, source) == 0
            painted = one_surface(lib, M, iso)
            assert np.array_equal(bits(painted.V), bits(plain.V)) and np.array_equal(painted.T, plain.T) and np.array_equal(bits(painted.N), bits(plain.N))
            want = po.color_values(val[source - 1], pal, lo, hi)
            assert np.array_equal(painted.color, want), "source %d: %d of %d colours differ" % (source, np.count_nonzero(painted.color != want), want.size)
            assert source != 1 or len(set(want.tolist())) == len(pal)
        assert L.MC33_set_color_source(M, 0) == 0
        assert np.all(one_surface(lib, M, iso).color == po.DEFAULT_COLOR)   # back at the property: what it was before
        # the struct
        out = IsosurfaceCurvature()
        assert L.MC33_isosurface_curvature(M, lib.real(iso), C.byref(out)) == 0 and L.MC33_isosurface_curvature(M, lib.real(iso), None) == -1
        assert (out.nV, out.nT) == (plain.nV, plain.nT)
        assert (tuple(out.lo), tuple(out.hi), out.finite, out.undefined) == (summ.lo, summ.hi, summ.finite, summ.undefined)
        assert summ.undefined == 0
        bounds = []
        for got, q in ((out.total_mean, 0), (out.total_gauss, 1)):
            want, bound = co.total(plain.V, plain.T, R0, D, data.shape, val[q])
            bounds.append(bound)
            print("%s nneg=%d total %s = %.12g, oracle %.12g +- %.3g" % (dtype, nneg, co.NAMES[q], got, want, bound))
            assert abs(got - want) <= bound
        if not nneg:   # ... and equals the composition of the device calls, to the bit
            g = device_grid(data, R0, D)
            V, N, T, cnt = g.extract(iso)
            res = g.curvature(V)
            comp = (cnt.nV, cnt.nT, tuple(res.lo[k] for k in co.NAMES), tuple(res.hi[k] for k in co.NAMES), res.finite, res.undefined,
                    g.measure(V, T, res.mean).property_integral, g.measure(V, T, res.gauss).property_integral)
            assert as_tuple(out) == comp
            g.close()
        else:   # the plain flavour on the same grid: the negated mean, the same gauss
            other = capi(dtype, False)
            M2 = other.lib.create_MC33(G)
            assert M2
            try:
                out2 = IsosurfaceCurvature()
                assert other.lib.MC33_isosurface_curvature(M2, other.real(iso), C.byref(out2)) == 0
            finally:
                other.lib.free_MC33(M2)
            assert tuple(out.lo) == (-out2.hi[0], out2.lo[1], -out2.hi[3], -out2.hi[2]) and tuple(out.hi) == (-out2.lo[0], out2.hi[1], -out2.lo[3], -out2.lo[2])
            assert abs(out.total_mean + out2.total_mean) <= 2 * bounds[0] and abs(out.total_gauss - out2.total_gauss) <= 2 * bounds[1]
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_totals_are_nan_when_a_vertex_is_undefined():
    """an infinite sample at the high end of a cut edge: the surface keeps its cells, the gradient there is infinite, the
    curvature inf / inf"""
    lib = capi("f32")
    L = lib.lib
    data, iso = c_field("f32")
    data = data.copy()
    G, keep = lib.make_grid(data, R0, D)
    M = L.create_MC33(G)
    assert M
    try:
        V = one_surface(lib, M, iso).V
        _, i, f = po.grid_coordinates(V[1000:1001], R0, D, data.shape)
        x, y, z = (int(v) for v in i[0])
        ends = [(z, y, x), (z + int(f[0, 2] != 0), y + int(f[0, 1] != 0), x + int(f[0, 0] != 0))]
        high = [e for e in ends if data[e] > iso]
        assert len(high) == 1
        keep[high[0]] = np.inf
        data[high[0]] = np.inf
        L.MC33_grid_changed(M)
        s = one_surface(lib, M, iso)
        summ = co.summary(co.curvature(s.V, R0, D, data))
        assert summ.undefined > 0 and summ.finite > 1000
        out = IsosurfaceCurvature()
        assert L.MC33_isosurface_curvature(M, lib.real(iso), C.byref(out)) == 0
        assert (out.nV, out.finite, out.undefined) == (s.nV, summ.finite, summ.undefined) and (tuple(out.lo), tuple(out.hi)) == (summ.lo, summ.hi)
        assert np.isnan(out.total_mean) and np.isnan(out.total_gauss)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refusals(monkeypatch):
    lib = capi("f32")
    L = lib.lib
    data, iso = c_field("f32")
    out = IsosurfaceCurvature(7, 8)
    # an inclined grid
    G, keep = lib.make_grid(data, None, (0.1, 0.1, 0.1), inclined=fx.cell_matrices(80.0, 75.0, 100.0))
    M = L.create_MC33(G)
    assert M
    try:
        assert L.MC33_set_color_source(M, 1) == -1 and L.MC33_set_color_source(M, 0) == 0
        assert L.MC33_isosurface_curvature(M, lib.real(iso), C.byref(out)) == -1 and (out.nV, out.nT) == (7, 8)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
    # one cell on an axis
    G, keep = lib.make_grid(data[:2])
    M = L.create_MC33(G)
    assert M
    try:
        assert L.MC33_set_color_source(M, 2) == -1 and L.MC33_isosurface_curvature(M, lib.real(iso), C.byref(out)) == -1
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
    # an object on several slabs refuses the source and still extracts
    monkeypatch.delenv("MC33_HIP_DEVICES", raising=False)
    G, keep = lib.make_grid(data, R0, D)
    M = L.create_MC33(G)
    one = one_surface(lib, M, iso)
    L.free_MC33(M)
    monkeypatch.setenv("MC33_HIP_DEVICES", "0,0,0")
    M = L.create_MC33(G)
    assert M
    try:
        pal = palette(5)
        assert L.MC33_set_color_map(M, c_palette(pal), len(pal), -1.0, 1.0) == 0
        assert L.MC33_set_color_source(M, 1) == -1 and L.MC33_isosurface_curvature(M, lib.real(iso), C.byref(out)) == -1
        s = one_surface(lib, M, iso)
        assert np.array_equal(bits(s.V), bits(one.V)) and np.array_equal(s.T, one.T) and np.all(s.color == po.DEFAULT_COLOR)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
