"""Resampling the grid on the device before extraction, on the GPU: k_rs_resample through DeviceGrid.resampled, the
raw ABI and the C API, every output compared with tests/resample_oracle.py bit for bit - no tolerance anywhere.  The shapes are the
smallest at which the tiling can go wrong (tests/resample_cases.py), not the workload's."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import layouts as lo
import resample_cases as rc
import resample_oracle as ro
from mc33_c_library_amd.api import GridResampling, SurfaceSimplification
from mc33_capi import CMeasure, MC33Lib, product_path, ref_path

pytestmark = pytest.mark.gpu

TYPES = ["f32", "u16", "u8", "u32", "f64"]
CANARY = 0xA5


def unsigned(a):
    """a tensor's or array's samples as numpy of the grid's own type (uint16 / uint32 travel as int16 / int32 bit patterns)"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def source_grid(F, layout="dense", **kw):
    """F adopted at a layout inside a poisoned flat buffer"""
    from mc33_c_library_amd import DeviceGrid
    lay = lo.layout(layout, F.shape, F.dtype.itemsize)
    flat = lo.to_device(lo.place(F, lay, [0.0]))
    g = DeviceGrid(lo.device_view(flat, F.shape, lay), npx=F.shape[2], **kw)
    g.flat = flat
    return g


def canaried(shape, dtype, layout):
    """(flat device tensor full of the canary, the output grid as a strided window of it, the layout)"""
    import torch
    it = np.dtype(dtype).itemsize
    lay = lo.layout(layout, shape, it)
    flat = lo.to_device(np.full(lo.flat_size(shape, lay), np.array([CANARY] * it, np.uint8).view(dtype)[0], dtype))
    return flat, torch.as_strided(flat, tuple(shape), (lay[1], lay[0], 1), lay[2]), lay


def split(flat, shape, lay):
    """(the grid, every other sample) of a flat output buffer"""
    out = unsigned(flat)
    got = np.array(lo.host_view(out, shape, lay))
    mask = np.ones(out.size, bool)
    np.lib.stride_tricks.as_strided(mask[lay[2]:], shape, (lay[1], lay[0], 1))[...] = False
    return got, out[mask]


def resample_at(g, want_shape, dtype, taps, stride, dst_layout):
    flat, view, lay = canaried(want_shape, rc.NP_DTYPES[dtype], dst_layout)
    g.resample_into(view, want_shape[2], taps, stride)
    return split(flat, want_shape, lay)


def check(got, rest, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = int(np.count_nonzero(got.view(np.uint8) != want.view(np.uint8)))
    assert bad == 0, "%s: %d of %d bytes differ from the oracle" % (what, bad, want.nbytes)
    assert np.all(rest.view(np.uint8) == CANARY), "%s: a sample that is no output grid point was written" % what


# ---- the case table ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.CASES))
def test_case_table(name):
    F, taps, stride, want = rc.case(name, "f32")
    g = source_grid(F, "padx_odd")
    assert g.resampled_size(taps, stride) == want.shape[::-1]
    got, rest = resample_at(g, want.shape, "f32", taps, stride, "padx_odd")
    check(got, rest, want, name)
    # ... and through DeviceGrid.resampled: a tensor with rows on 16-byte boundaries, a grid of the new geometry
    r = g.resampled(taps, stride)
    assert r.tensor.data_ptr() % 16 == 0 and r.tensor.stride(1) * 4 % 16 == 0 and r.tensor.stride(1) >= want.shape[2]
    assert (r.desc.npx, r.desc.npy, r.desc.npz_resident, r.desc.nz_total) == (want.shape[2], want.shape[1], want.shape[0], want.shape[0] - 1)
    assert ro.same_bits(unsigned(r.tensor[:, :, :want.shape[2]]), want), name


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", list(rc.ALL_TYPE_CASES))
def test_every_sample_type(name, dtype):
    F, taps, stride, want = rc.case(name, dtype)
    g = source_grid(F, "offs")
    got, rest = resample_at(g, want.shape, dtype, taps, stride, "all")
    check(got, rest, want, "%s %s" % (name, dtype))
    r = g.resampled(taps, stride)
    assert ro.same_bits(unsigned(r.tensor[:, :, :want.shape[2]]), want)
    assert tuple(r.desc.d) == ro.geometry(g.desc.r0, g.desc.d, stride)[1] and tuple(r.desc.r0) == tuple(g.desc.r0)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u8", "f64"])
def test_result_is_the_same_at_every_pair_of_layouts(dtype):
    F, taps, stride, want = rc.case("types_stride_3_1_2", dtype)
    for src in ("dense", "padx_odd", "offs", "all"):
        g = source_grid(F, src)
        for dst in ("padx16", "padx_odd", "all"):
            got, rest = resample_at(g, want.shape, dtype, taps, stride, dst)
            check(got, rest, want, "%s: %s -> %s" % (dtype, src, dst))
        g.close()


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_uploaded_grid_gives_the_bytes_of_the_adopted_one(dtype):
    """the library's own pitched copy (mc33hip_upload_contiguous) as the source, through the raw ABI"""
    from mc33_c_library_amd.api import GridDesc, Resampling, load_library
    F, taps, stride, want = rc.case("types_one_past_a_tile", dtype)
    lib = load_library(dtype)
    npz, npy, npx = F.shape
    desc = GridDesc(npx, npy, npz, 0, npz - 1, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1), F.dtype.itemsize, 0)
    ctx = C.c_void_p()
    assert lib.mc33hip_create(C.byref(ctx), C.byref(desc)) == 0
    try:
        host = np.ascontiguousarray(F)
        assert lib.mc33hip_upload_contiguous(ctx, C.c_void_p(host.ctypes.data)) == 0
        flat, view, lay = canaried(want.shape, F.dtype, "padx16")
        r = Resampling()
        keep = [(C.c_double * len(t))(*t) for t in taps]
        for a in range(3):
            r.taps[a], r.ntaps[a], r.stride[a] = C.cast(keep[a], C.POINTER(C.c_double)), len(taps[a]), stride[a]
        n = (C.c_uint * 3)()
        assert lib.mc33hip_resampled_size(ctx, C.byref(r), C.byref(n)) == 0 and tuple(n) == want.shape[::-1]
        assert lib.mc33hip_resample_grid(ctx, C.byref(r), C.c_void_p(view.data_ptr()), lay[0], lay[1]) == 0
        got, rest = split(flat, want.shape, lay)
        check(got, rest, want, "uploaded " + dtype)
    finally:
        lib.mc33hip_destroy(ctx)


def test_two_calls_and_other_taps_on_one_context():
    F, taps, stride, want = rc.case("stride_3_1_2", "f32")
    g = source_grid(F)
    a = resample_at(g, want.shape, "f32", taps, stride, "dense")[0]
    F2, taps2, stride2, want2 = rc.case("radii_8_0_3", "f32")   # the same 67 x 35 x 19 field (one seed per shape is not needed: other taps, other tiles)
    g2 = source_grid(F2)
    first = resample_at(g2, want2.shape, "f32", taps2, stride2, "dense")[0]
    other = ro.resample(F2, taps, stride)
    assert ro.same_bits(resample_at(g2, other.shape, "f32", taps, stride, "dense")[0], other)   # other taps: the scratch is reused
    again = resample_at(g2, want2.shape, "f32", taps2, stride2, "dense")[0]
    assert ro.same_bits(first, want2) and ro.same_bits(again, first) and ro.same_bits(a, want)
    b = resample_at(g, want.shape, "f32", taps, stride, "dense")[0]
    assert ro.same_bits(a, b)


# ---- argument checks --------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    import torch
    from mc33_c_library_amd import DeviceGrid, MC33Error, Range
    from mc33_c_library_amd.api import EINVAL, Resampling
    F = rc.finite_field("f32", (12, 9, 7), seed=9)
    g = source_grid(F)
    want = ro.resample(F)
    flat, view, lay = canaried(want.shape, np.float32, "padx16")
    nan, inf = float("nan"), float("inf")
    bad = [dict(taps=([0.5, 0.5], None, None)), dict(taps=(None, [1.0] * 19, None)), dict(taps=(None, None, [0.25, nan, 0.25])),
           dict(taps=([inf], None, None)), dict(stride=(0, 1, 1)), dict(stride=(1, 1, 7)), dict(stride=(12, 1, 1)), dict(taps=(None, [], None))]
    for kw in bad:
        with pytest.raises(MC33Error) as e:
            g.resample_into(view, want.shape[2], **kw)
        assert e.value.code == EINVAL, kw
        with pytest.raises(MC33Error):
            g.resampled_size(**kw)
    lib, r = g.lib, Resampling()
    r.stride[0] = r.stride[1] = r.stride[2] = 1
    ptr, pitch, slc = C.c_void_p(view.data_ptr()), lay[0], lay[1]
    assert lib.mc33hip_resample_grid(None, C.byref(r), ptr, pitch, slc) == EINVAL
    assert lib.mc33hip_resample_grid(g.ctx, None, ptr, pitch, slc) == EINVAL
    assert lib.mc33hip_resample_grid(g.ctx, C.byref(r), None, pitch, slc) == EINVAL
    assert lib.mc33hip_resample_grid(g.ctx, C.byref(r), ptr, want.shape[2] - 1, slc) == EINVAL            # pitch < np_out[0]
    assert lib.mc33hip_resample_grid(g.ctx, C.byref(r), ptr, pitch, pitch * want.shape[1] - 1) == EINVAL  # slice < pitch * np_out[1]
    assert lib.mc33hip_resampled_size(g.ctx, C.byref(r), None) == EINVAL
    # not in place: dst inside the source's byte range, and a range that only meets its last sample
    src = g.tensor
    assert lib.mc33hip_resample_grid(g.ctx, C.byref(r), C.c_void_p(src.data_ptr()), src.stride(1), src.stride(0)) == EINVAL
    last = src.data_ptr() + (F.size - 1) * 4
    assert lib.mc33hip_resample_grid(g.ctx, C.byref(r), C.c_void_p(last), src.stride(1), src.stride(0)) == EINVAL
    # a z-slab context
    slab = DeviceGrid(src[2:6], nz_total=F.shape[0] - 1, plane0=2)
    assert lib.mc33hip_resample_grid(slab.ctx, C.byref(r), ptr, pitch, slc) == EINVAL
    slab.close()
    assert np.all(unsigned(flat).view(np.uint8) == CANARY)   # dst still holds its canary
    assert ro.same_bits(unsigned(g.flat)[:F.size].reshape(F.shape), F)   # ... and the source its samples
    # the context still resamples and extracts
    g.resample_into(view, want.shape[2])
    assert ro.same_bits(split(flat, want.shape, lay)[0], want)
    V, N, T, cnt = g.extract(0.25)
    assert cnt.nV > 0 and cnt.nT > 0
    torch.cuda.synchronize()


# ---- end to end: the surface of the resampled grid ----------------------------------------------------------------------------------------

def _cos(dtype):
    if dtype == "f32":
        data, r0, d = fx.cos_field(64)
        return data, r0, d, 0.1
    return fx.cos_field_u16(64, 64, 64), (0.0, 0.0, 0.0), (0.5, 0.25, 1.0), 30000.5


def same_surface(got, ref, what):
    V, N, T, cnt = got
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT) and ref.nV > 0, what
    assert np.array_equal(T.cpu().numpy().view(np.uint32), ref.T), what
    assert ro.same_bits(V.cpu().numpy(), ref.V) and ro.same_bits(N.cpu().numpy(), ref.N), what


@pytest.mark.parametrize("stride", [(1, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_extraction_of_the_resampled_grid(reflibs, dtype, stride):
    from mc33_c_library_amd import DeviceGrid
    data, r0, d, iso = _cos(dtype)
    want = ro.resample(data, (rc.G1, rc.G1, rc.G1), stride)
    r0o, do = ro.geometry(r0, d, stride)
    ref = reflibs[dtype].isosurface(want, iso, r0o, do)
    g = DeviceGrid(lo.to_device(data.reshape(-1)).reshape(data.shape), r0=r0, d=d)
    r = g.resampled(sigma=1.0, stride=stride)
    g.close()   # (the new grid does not need the old one)
    same_surface(r.extract(iso), ref, "%s stride %r" % (dtype, stride))


def test_extraction_of_a_resampled_inclined_grid(reflibs):
    from mc33_c_library_amd import DeviceGrid
    data, r0, d, iso = _cos("f32")
    A, Ai = fx.general_matrices()
    stride = (2, 1, 3)
    want = ro.resample(data, (rc.G1, None, rc.G1), stride)
    r0o, do = ro.geometry(r0, d, stride)
    ref = reflibs["f32"].isosurface(want, iso, r0o, do, inclined=(A, Ai))
    g = DeviceGrid(lo.to_device(data.reshape(-1)).reshape(data.shape), r0=r0, d=d)
    g.set_inclined(A, Ai)
    r = g.resampled(sigma=(1.0, 0.0, 1.0), stride=stride)
    same_surface(r.extract(iso), ref, "inclined")


# ---- the C API ------------------------------------------------------------------------------------------------------------------------------

def resampling(sigma, stride, radius=(0, 0, 0)):
    return GridResampling((C.c_double * 3)(*sigma), (C.c_uint * 3)(*radius), (C.c_uint * 3)(*stride))


def grid_samples(lib, Z):
    """the samples of a _GRD made by alloc_F, as numpy [z][y][x]"""
    z = Z.contents
    npx, npy, npz = z.N[0] + 1, z.N[1] + 1, z.N[2] + 1
    planes = C.cast(z.F, C.POINTER(C.POINTER(C.c_void_p)))
    out = np.empty((npz, npy, npx), lib.np_dtype)
    for k in range(npz):
        for j in range(npy):
            C.memmove(out[k, j].ctypes.data, planes[k][j], npx * out.itemsize)
    return out


def surface_of(lib, L, M, iso):
    S = L.calculate_isosurface(M, lib.real(iso))
    assert S
    try:
        return lib.copy_surface(S)
    finally:
        L.free_surface_memory(S)


def same_host_surface(got, ref, what):
    assert (got.nV, got.nT) == (ref.nV, ref.nT) and ref.nV > 0, what
    assert np.array_equal(got.T, ref.T) and ro.same_bits(got.V, ref.V) and ro.same_bits(got.N, ref.N), what


@pytest.mark.parametrize("dtype", ["f32", "u16", "f64"])
def test_c_api(products, reflibs, dtype):
    lib = products[dtype]
    L = lib.lib
    if dtype == "f64":
        data, r0, d, iso = fx.cos_field(40, dtype=np.float64) + (0.1,)
    else:
        data, r0, d, iso = _cos(dtype)
        data = data[:40, :44, :48]
    sig, stride = (1.0, 0.0, 2.0), (2, 1, 3)
    taps = tuple(ro.gaussian_taps(s) if s else None for s in sig)
    want = ro.resample(data, taps, stride)
    r0o, do = ro.geometry(r0, d, stride)
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    assert M
    R = L.MC33_create_resampled(M, C.byref(resampling(sig, stride)))
    assert R
    assert not L.MC33_resampled_grid(M)   # an ordinary object has no such grid
    # the refused structs: NULL, and the source as it was
    before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
    for bad in (resampling((-1.0, 0, 0), (1, 1, 1)), resampling((float("nan"), 0, 0), (1, 1, 1)), resampling((3.0, 0, 0), (1, 1, 1)),
                resampling((1.0, 0, 0), (1, 1, 1), radius=(9, 0, 0)), resampling((0, 0, 0), (1, 0, 1)), resampling((0, 0, 0), (1, 1, data.shape[0]))):
        assert not L.MC33_create_resampled(M, C.byref(bad))
    assert not L.MC33_create_resampled(M, None)
    assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
    L.free_MC33(M)   # the source goes first
    L.free_memory_grd(G)
    del keep
    try:
        m = R.contents
        assert (m.nx, m.ny, m.nz) == (want.shape[2] - 1, want.shape[1] - 1, want.shape[0] - 1) and not m.F
        assert tuple(m.O) == tuple(lib.np_real(x) for x in r0o) and tuple(m.D) == tuple(lib.np_real(x) for x in do)
        ref = reflibs[dtype].isosurface(want, iso, r0o, do)
        same_host_surface(surface_of(lib, L, R, iso), ref, dtype)
        Z = L.MC33_resampled_grid(R)
        assert Z
        z = Z.contents
        assert tuple(z.N) == (m.nx, m.ny, m.nz) and tuple(z.r0) == r0o and tuple(z.d) == do and z.internal_data == 1
        assert ro.same_bits(grid_samples(lib, Z), want)
        L.free_memory_grd(Z)
        # a resampled object resampled again: the oracle applied twice
        sig2, stride2 = (0.0, 0.5, 0.0), (1, 2, 1)
        R2 = L.MC33_create_resampled(R, C.byref(resampling(sig2, stride2)))
        assert R2
        want2 = ro.resample(want, (None, ro.gaussian_taps(0.5), None), stride2)
        Z2 = L.MC33_resampled_grid(R2)
        assert Z2 and ro.same_bits(grid_samples(lib, Z2), want2) and tuple(Z2.contents.d) == ro.geometry(r0o, do, stride2)[1]
        L.free_memory_grd(Z2)
        same_host_surface(surface_of(lib, L, R2, iso), reflibs[dtype].isosurface(want2, iso, *ro.geometry(r0o, do, stride2)), dtype + " twice")
        L.free_MC33(R2)
        # MC33_grid_changed does nothing on it, and it extracts again
        L.MC33_grid_changed(R)
        same_host_surface(surface_of(lib, L, R, iso), ref, dtype + " again")
    finally:
        L.free_MC33(R)


def test_c_api_measures_and_simplifies_a_resampled_object(products):
    """the other entry points work on it as on an object created from the same samples"""
    lib = products["f32"]
    L = lib.lib
    data, r0, d, iso = _cos("f32")
    stride = (2, 2, 2)
    want = ro.resample(data, (rc.G1, rc.G1, rc.G1), stride)
    r0o, do = ro.geometry(r0, d, stride)
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    R = L.MC33_create_resampled(M, C.byref(resampling((1.0, 1.0, 1.0), stride)))
    G2, keep2 = lib.make_grid(want, r0o, do)
    P = L.create_MC33(G2)   # the plain object of the oracle's grid
    assert M and R and P
    try:
        sp = SurfaceSimplification((C.c_double * 3)(2, 2, 2), 1, 1)   # the first vertex of every cell: rows of the input, bit for bit
        out = []
        for obj in (R, P):
            mm = CMeasure()
            assert L.MC33_measure_isosurface(obj, lib.real(iso), C.byref(mm)) == 0
            S = L.MC33_calculate_simplified_isosurface(obj, lib.real(iso), C.byref(sp))
            assert S
            out.append((mm, lib.copy_surface(S)))
            L.free_surface_memory(S)
        (ma, sa), (mb, sb) = out
        assert (ma.nV, ma.nT) == (mb.nV, mb.nT) and ma.nV > 0
        assert tuple(ma.bbox_min) == tuple(mb.bbox_min) and tuple(ma.bbox_max) == tuple(mb.bbox_max)
        same_host_surface(sa, sb, "simplified")
    finally:
        for obj in (R, P, M):
            L.free_MC33(obj)
        L.free_memory_grd(G)
        L.free_memory_grd(G2)
        del keep, keep2


def test_c_api_normal_neg_flavour():
    lib, ref = MC33Lib(product_path("f32", nneg=True), "f32"), MC33Lib(ref_path("f32", nneg=True), "f32")
    L = lib.lib
    data, r0, d, iso = _cos("f32")
    stride = (2, 2, 2)
    want = ro.resample(data, (rc.G1, rc.G1, rc.G1), stride)
    r0o, do = ro.geometry(r0, d, stride)
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    R = L.MC33_create_resampled(M, C.byref(resampling((1.0, 1.0, 1.0), stride)))
    assert M and R
    try:
        same_host_surface(surface_of(lib, L, R, iso), ref.isosurface(want, iso, r0o, do), "nneg")
    finally:
        L.free_MC33(R)
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
