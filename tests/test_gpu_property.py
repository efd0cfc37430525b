"""GPU tests of the property grid: a second scalar field sampled at the vertices on the device (include/mc33_hip.h:
mc33hip_sample_property / mc33hip_color_vertices; include/marching_cubes_33.h: MC33_set_property_grid / MC33_set_color_map).

V always comes from the reference twin (oracle/_ref), which tests/test_gpu_parity.py proves bit-equal to the product's V; the
expected values come from tests/property_oracle.py, the definition in numpy float64.  Everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import property_oracle as po
from mc33_capi import FN
from mesh_harness import bits, c_palette, capi, device_grid, palette, to_device

pytestmark = pytest.mark.gpu

AWKWARD_R0, AWKWARD_D = (-1.3, 0.7, 2.9), (0.1, 0.07, 0.13)
UNIT_R0, UNIT_D = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


CASES = {
    "cos64": lambda: (fx.cos_field(64)[0], 0.0),
    "noise": lambda: (fx.noise_f32(0, 9, shape=(26, 31, 40)), 0.05),
}


@pytest.mark.parametrize("geometry", ["own", "unit", "awkward"])
@pytest.mark.parametrize("case", ["cos64", "noise"])
def test_sample_property_f32_is_bit_identical(reflibs, case, geometry):
    data, iso = CASES[case]()
    r0, d = {"own": (fx.cos_field(64)[1], fx.cos_field(64)[2]), "unit": (UNIT_R0, UNIT_D), "awkward": (AWKWARD_R0, AWKWARD_D)}[geometry]
    V = reflibs["f32"].isosurface(data, iso, r0, d).V
    P = fx.noise_f32(0, 77, shape=data.shape) * np.float32(1000.0)
    g = device_grid(data, r0, d, P)
    got = g.sample_property(to_device(V)).cpu().numpy()
    want = po.sample_property(V, r0, d, P)
    nbad = int(np.count_nonzero(bits(got) != bits(want)))
    print("%s %s: %d vertices, %d differ" % (case, geometry, V.shape[0], nbad))
    assert V.shape[0] > 1000 and nbad == 0
    # ... and the same through extract(with_property=True), on the product's own V
    V2, _, _, cnt, p2 = g.extract(iso, with_property=True)
    assert np.array_equal(bits(V2.cpu().numpy()), bits(V)) and np.array_equal(bits(p2.cpu().numpy()), bits(want))
    g.detach_property()
    from mc33_c_library_amd.api import MC33Error
    with pytest.raises(MC33Error):
        g.sample_property(to_device(V))


@pytest.mark.parametrize("n", [2, 7, 256])
def test_color_vertices_f32(reflibs, n):
    """lo / hi inside the value range, so both clamps are hit; NaNs planted in the property"""
    data, iso = CASES["noise"]()
    V = reflibs["f32"].isosurface(data, iso, AWKWARD_R0, AWKWARD_D).V
    P = fx.noise_f32(0, 78, shape=data.shape) * np.float32(10.0)
    P.reshape(-1)[::97] = np.nan
    val = po.sample_property(V, AWKWARD_R0, AWKWARD_D, P)
    lo, hi = -2.5, 3.25
    assert np.nanmin(val) < lo and np.nanmax(val) > hi and np.isnan(val).any() and not np.isnan(val).all()
    pal = palette(n)
    g = device_grid(data, AWKWARD_R0, AWKWARD_D, P)
    got = g.color_vertices(to_device(V), pal, lo, hi).cpu().numpy()
    want = po.color_values(val, pal, lo, hi)
    assert len(set(want.tolist())) == n + 1  # every palette entry and the NaN colour
    assert np.array_equal(got, want), "%d of %d colours differ" % (np.count_nonzero(got != want), got.size)
    # another NaN colour; and the refusals
    got = g.color_vertices(to_device(V), pal, lo, hi, nan_color=0x01020304).cpu().numpy()
    assert np.array_equal(got, po.color_values(val, pal, lo, hi, default=0x01020304))
    from mc33_c_library_amd.api import MC33Error, EINVAL
    for bad_pal, blo, bhi in ((pal[:1], lo, hi), (palette(257), lo, hi), (pal, hi, lo), (pal, lo, lo), (pal, float("nan"), hi), (pal, lo, float("nan"))):
        with pytest.raises(MC33Error) as e:
            g.color_vertices(to_device(V), bad_pal, blo, bhi)
        assert e.value.code == EINVAL
    A, Ai = fx.cell_matrices(80.0, 75.0, 100.0)
    g.set_inclined(A, Ai, True)
    with pytest.raises(MC33Error) as e:
        g.sample_property(to_device(V))
    assert e.value.code == EINVAL
    g.set_inclined(None)
    assert np.array_equal(bits(g.sample_property(to_device(V)).cpu().numpy()), bits(val))


@pytest.mark.parametrize("dtype", ["u8", "u16", "u32", "f64"])
def test_other_sample_types(reflibs, dtype):
    n = 40
    if dtype == "f64":
        data, iso = fx.cos_field(n, dtype=np.float64)[0], 0.0
        P = fx.noise_f32(0, 5, shape=data.shape).astype(np.float64) * 1e6 + 1e-3
    elif dtype == "u8":
        data, iso, P = fx.cos_field_int(n, np.uint8, 40.0, 128.0), 128.5, fx.noise_u8(0, 5, shape=(n, n, n))
    elif dtype == "u16":
        data, iso, P = fx.cos_field_int(n, np.uint16, 10000.0, 32768.0), 32768.5, fx.noise_u16(0, 5, shape=(n, n, n))
    else:
        data, iso, P = fx.cos_field_int(n, np.uint32, 5.0e8, 2147483648.0), 2147483648.5, fx.noise_u32(0, 5, shape=(n, n, n))
    V = reflibs[dtype].isosurface(data, iso, AWKWARD_R0, AWKWARD_D).V
    assert V.dtype == (np.float64 if dtype == "f64" else np.float32) and V.shape[0] > 1000
    g = device_grid(data, AWKWARD_R0, AWKWARD_D, P)
    got = g.sample_property(to_device(V)).cpu().numpy()
    want = po.sample_property(V, AWKWARD_R0, AWKWARD_D, P)
    assert np.array_equal(bits(got), bits(want)), "%d of %d values differ" % (np.count_nonzero(bits(got) != bits(want)), got.size)
    lo, hi = float(np.percentile(want, 20)), float(np.percentile(want, 80))
    pal = palette(11)
    assert np.array_equal(g.color_vertices(to_device(V), pal, lo, hi).cpu().numpy(), po.color_values(want, pal, lo, hi))


# ---- the C API -----------------------------------------------------------------------------------------------------------

def one_surface(lib, M, iso):
    S = lib.lib.calculate_isosurface(M, lib.real(iso))
    assert S, "calculate_isosurface returned NULL"
    try:
        return lib.copy_surface(S)
    finally:
        lib.lib.free_surface_memory(S)


def same_geometry(a, b):
    return (a.nV == b.nV and a.nT == b.nT and np.array_equal(bits(a.V), bits(b.V)) and np.array_equal(bits(a.N), bits(b.N)) and
            np.array_equal(a.T, b.T))


@pytest.mark.parametrize("nneg", [False, True])
def test_c_api_colours(reflibs, nneg):
    lib = capi("f32", nneg)
    L = lib.lib
    data, iso = CASES["noise"]()
    refV = reflibs["f32"].isosurface(data, iso, AWKWARD_R0, AWKWARD_D).V
    P = fx.noise_f32(0, 79, shape=data.shape) * np.float32(10.0)
    P.reshape(-1)[::101] = np.nan
    pal, lo, hi = palette(7), -2.5, 3.25
    want = po.color_vertices(refV, AWKWARD_R0, AWKWARD_D, P, pal, lo, hi)
    G, keep = lib.make_grid(data, AWKWARD_R0, AWKWARD_D)
    Pg, keep2 = lib.make_grid(P, AWKWARD_R0, AWKWARD_D)
    small, keep3 = lib.make_grid(P[:, :, :-1])
    M = L.create_MC33(G)
    assert M
    try:
        plain = one_surface(lib, M, iso)
        assert np.array_equal(bits(plain.V), bits(refV)) and np.all(plain.color == po.DEFAULT_COLOR)
        assert L.MC33_set_property_grid(M, small) == -1  # wrong N: refused, nothing changes
        assert L.MC33_set_property_grid(M, Pg) == 0
        assert np.all(one_surface(lib, M, iso).color == po.DEFAULT_COLOR)  # no map yet
        assert L.MC33_set_color_map(M, c_palette(pal), 1, lo, hi) == -1 and L.MC33_set_color_map(M, c_palette(pal), len(pal), hi, lo) == -1
        assert L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        painted = one_surface(lib, M, iso)
        assert same_geometry(painted, plain)
        assert np.array_equal(painted.color, want), "%d of %d colours differ" % (np.count_nonzero(painted.color != want), want.size)
        assert L.MC33_set_property_grid(M, small) == -1
        assert np.array_equal(one_surface(lib, M, iso).color, want)
        # DefaultColorMC is read when the surface is made
        dflt = C.c_int.in_dll(L, "DefaultColorMC")
        dflt.value = 0x0badf00d
        try:
            assert np.array_equal(one_surface(lib, M, iso).color, po.color_vertices(refV, AWKWARD_R0, AWKWARD_D, P, pal, lo, hi, default=0x0badf00d))
        finally:
            dflt.value = int(po.DEFAULT_COLOR)
        # several isovalues in one call
        isos = [0.05, -0.3, 0.4]
        out = (C.POINTER(lib.SURFACE) * 3)()
        assert L.calculate_isosurfaces(M, (lib.real * 3)(*isos), 3, out) == 3
        for k, v in enumerate(isos):
            s = lib.copy_surface(out[k])
            L.free_surface_memory(out[k])
            rv = reflibs["f32"].isosurface(data, v, AWKWARD_R0, AWKWARD_D).V
            assert np.array_equal(bits(s.V), bits(rv))
            assert np.array_equal(s.color, po.color_vertices(rv, AWKWARD_R0, AWKWARD_D, P, pal, lo, hi)), "isovalue %g" % v
        # the caller rewrote P: attaching again uploads again
        keep2[:] = keep2 * np.float32(0.5)
        assert L.MC33_set_property_grid(M, Pg) == 0
        assert np.array_equal(one_surface(lib, M, iso).color, po.color_vertices(refV, AWKWARD_R0, AWKWARD_D, keep2, pal, lo, hi))
        # detach: all DefaultColorMC again; the map alone does nothing; attach again without the map: nothing either
        assert L.MC33_set_property_grid(M, None) == 0
        again = one_surface(lib, M, iso)
        assert same_geometry(again, plain) and np.all(again.color == po.DEFAULT_COLOR)
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, None, 0, 0.0, 0.0) == 0
        assert np.all(one_surface(lib, M, iso).color == po.DEFAULT_COLOR)
    finally:
        L.free_MC33(M)
        for x in (G, Pg, small):
            L.free_memory_grd(x)
        del keep, keep2, keep3


def test_c_api_refuses_an_inclined_grid():
    lib = capi("f32")
    L = lib.lib
    data = fx.cos_field(24)[0]
    inc = fx.cell_matrices(80.0, 75.0, 100.0)
    G, keep = lib.make_grid(data, None, (0.1, 0.1, 0.1), inclined=inc)
    Pg, keep2 = lib.make_grid(data)
    Pi, keep3 = lib.make_grid(data, inclined=inc)
    H, keep4 = lib.make_grid(data)
    M, M2 = L.create_MC33(G), L.create_MC33(H)
    assert M and M2
    try:
        assert L.MC33_set_property_grid(M, Pg) == -1   # the extractor's grid is inclined
        assert L.MC33_set_property_grid(M2, Pi) == -1  # the property grid is
        assert L.MC33_set_property_grid(M2, Pg) == 0
    finally:
        L.free_MC33(M)
        L.free_MC33(M2)
        for x in (G, Pg, Pi, H):
            L.free_memory_grd(x)
        del keep, keep2, keep3, keep4


@pytest.mark.parametrize("devices", ["0,0,0", "0,0,0,0,0,0,0"])
def test_slabs_colour_like_one_slab(reflibs, devices, monkeypatch):
    """z-slabs behind the C API: every slab holds its own window of the property grid - one plane beyond each end of its cell
    slices - and colours its own vertices.  Noise: every z plane is cut."""
    lib = capi("f32")
    L = lib.lib
    data, iso = fx.noise_f32(0, 21, shape=(30, 20, 24)), 0.05
    P = fx.noise_f32(0, 22, shape=data.shape) * np.float32(10.0)
    pal, lo, hi = palette(33), -6.0, 5.0
    refV = reflibs["f32"].isosurface(data, iso, AWKWARD_R0, AWKWARD_D).V
    want = po.color_vertices(refV, AWKWARD_R0, AWKWARD_D, P, pal, lo, hi)
    zlo, zhi = po.planes_needed(refV, AWKWARD_R0, AWKWARD_D, data.shape)
    assert (zlo, zhi) == (0, data.shape[0] - 1)
    got = {}
    for env in (None, devices):
        if env is None:
            monkeypatch.delenv("MC33_HIP_DEVICES", raising=False)
        else:
            monkeypatch.setenv("MC33_HIP_DEVICES", env)
        G, keep = lib.make_grid(data, AWKWARD_R0, AWKWARD_D)
        Pg, keep2 = lib.make_grid(P, AWKWARD_R0, AWKWARD_D)
        M = L.create_MC33(G)
        assert M
        try:
            assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
            got[env] = one_surface(lib, M, iso)
        finally:
            L.free_MC33(M)
            L.free_memory_grd(G)
            L.free_memory_grd(Pg)
            del keep, keep2
    assert same_geometry(got[devices], got[None]) and np.array_equal(bits(got[None].V), bits(refV))
    assert np.array_equal(got[None].color, want)
    assert np.array_equal(got[devices].color, got[None].color), "%d colours differ" % np.count_nonzero(got[devices].color != got[None].color)


def test_window_violation_is_reported_not_clamped(reflibs):
    """A property window without its upper halo plane: the kernel tests the plane index before it loads, counts the vertices it
    cannot serve, and the next synchronising call says so; the context extracts correctly afterwards."""
    from mc33_c_library_amd.api import MC33Error, ERUNTIME
    data, iso = CASES["noise"]()
    ref = reflibs["f32"].isosurface(data, iso, AWKWARD_R0, AWKWARD_D)
    P = fx.noise_f32(0, 80, shape=data.shape)
    _, i, f = po.grid_coordinates(ref.V, AWKWARD_R0, AWKWARD_D, data.shape)
    top = data.shape[0] - 1
    missing = int(np.count_nonzero(i[:, 2] + (f[:, 2] != 0.0) >= top))
    assert missing > 0
    g = device_grid(data, AWKWARD_R0, AWKWARD_D)
    g.attach_property(to_device(P[:top]), plane0=0)  # planes [0, top): the last one is missing
    with pytest.raises(MC33Error) as e:
        g.sample_property(to_device(ref.V))
    assert e.value.code == ERUNTIME and str(missing) in str(e.value), str(e.value)
    V, N, T, cnt = g.extract(iso)
    assert cnt.nV == ref.nV and np.array_equal(bits(V.cpu().numpy()), bits(ref.V)) and np.array_equal(T.cpu().numpy().view(np.uint32), ref.T)
    # a window that begins above plane 0 is reported the same way; the whole grid attached: served
    g.attach_property(to_device(P[1:]), plane0=1)
    with pytest.raises(MC33Error) as e:
        g.sample_property(to_device(ref.V))
    assert e.value.code == ERUNTIME
    g.attach_property(to_device(P))
    assert np.array_equal(bits(g.sample_property(to_device(ref.V)).cpu().numpy()), bits(po.sample_property(ref.V, AWKWARD_R0, AWKWARD_D, P)))
    # a slab's window, in global plane numbers: the vertices it can serve agree with the whole grid
    sel = (i[:, 2] >= 10) & (i[:, 2] + (f[:, 2] != 0.0) <= 15)
    g.attach_property(to_device(P[10:16]), plane0=10)
    sub = np.ascontiguousarray(ref.V[sel])
    assert sub.shape[0] > 100
    assert np.array_equal(bits(g.sample_property(to_device(sub)).cpu().numpy()), bits(po.sample_property(sub, AWKWARD_R0, AWKWARD_D, P)))


def test_more_than_2_pow_24_vertices(reflibs):
    """A 1024^3 grid with five times the bench field's frequency: more than 2^24 vertices, so vertex indices and byte offsets
    beyond what a float or a 32-bit product holds.  The linear property is exact in float.  Every colour is compared with the
    oracle, run once on the host (stronger than the hash of the array), and a fixed sample of 2^16 of them is reported."""
    import torch
    n = 1024
    data, r0, d = fx.cos_field(n, lo=-20.0, hi=20.0)
    V = reflibs["f32"].isosurface(data, 0.0, r0, d).V
    nV = V.shape[0]
    print("vertices: %d" % nV)
    assert nV > (1 << 24)
    ax = np.arange(n, dtype=np.float32)
    plane = (np.float32(3.0) * ax)[None, :] + (np.float32(-2.0) * ax)[:, None] + np.float32(7.0)  # (integers below 2^24: exact)
    P = np.empty((n, n, n), np.float32)
    for k in range(n):
        np.add(plane, np.float32(5.0 * k), out=P[k])
    pal, lo, hi = palette(256), 500.0, 5500.0
    want = po.color_vertices(V, r0, d, P, pal, lo, hi)
    g = device_grid(data, r0, d)
    del data
    g.attach_property(torch.from_numpy(P).cuda())
    got = g.color_vertices(torch.from_numpy(V).cuda(), pal, lo, hi).cpu().numpy()
    idx = (np.arange(1 << 16, dtype=np.int64) * 2654435761) % nV
    nbad_sample = int(np.count_nonzero(got[idx] != want[idx]))
    nbad = int(np.count_nonzero(got != want))
    print("sample of 2^16: %d differ; all %d: %d differ; last vertex %08x / %08x" % (nbad_sample, nV, nbad, int(got[-1]) & 0xFFFFFFFF, int(want[-1]) & 0xFFFFFFFF))
    assert len(set(want[idx].tolist())) > 100
    assert nbad_sample == 0 and nbad == 0


def test_c_api_upload_paths(reflibs):
    """The two upload paths a contiguous float grid does not take: uchar rows that are not a whole number of dwords (packed
    through the staging buffers), and a property grid whose rows are separate allocations (generate_grid_from_fn: alloc_F)."""
    n = 37
    pal, lo, hi = palette(16), 40.0, 200.0
    # uchar, 37-byte rows
    lib = capi("u8")
    L = lib.lib
    data, P = fx.cos_field_int(n, np.uint8, 40.0, 128.0), fx.noise_u8(0, 6, shape=(n, n, n))
    refV = reflibs["u8"].isosurface(data, 128.5, AWKWARD_R0, AWKWARD_D).V
    G, keep = lib.make_grid(data, AWKWARD_R0, AWKWARD_D)
    Pg, keep2 = lib.make_grid(P)
    M = L.create_MC33(G)
    assert M
    try:
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        s = one_surface(lib, M, 128.5)
        assert np.array_equal(bits(s.V), bits(refV)) and np.array_equal(s.color, po.color_vertices(refV, AWKWARD_R0, AWKWARD_D, P, pal, lo, hi))
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2
    # float, every row of the property grid a malloc block of its own
    lib = capi("f32")
    L = lib.lib
    fn = FN(lambda x, y, z: 3.0 * x - 2.0 * y + 5.0 * z + 7.0)
    data = fx.cos_field(n)[0]
    refV = reflibs["f32"].isosurface(data, 0.0, AWKWARD_R0, AWKWARD_D).V
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    P = (3.0 * i - 2.0 * j + 5.0 * k + 7.0).astype(np.float32)
    G, keep = lib.make_grid(data, AWKWARD_R0, AWKWARD_D)
    Pg = L.generate_grid_from_fn(0.0, 0.0, 0.0, n - 1.0, n - 1.0, n - 1.0, 1.0, 1.0, 1.0, fn)
    assert Pg and tuple(Pg.contents.N) == (n - 1, n - 1, n - 1)
    M = L.create_MC33(G)
    assert M
    try:
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        s = one_surface(lib, M, 0.0)
        assert np.array_equal(bits(s.V), bits(refV)) and np.array_equal(s.color, po.color_vertices(refV, AWKWARD_R0, AWKWARD_D, P, pal, lo, hi))
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep
