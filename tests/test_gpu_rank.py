"""Rank-filtering the grid on the device, on the GPU: k_rk_minmax and k_rk_median through the raw ABI,
DeviceGrid.ranked and the C API, every output compared with tests/rank_oracle.py bit for bit - no tolerance anywhere.  The shapes
are the smallest at which the tiling can go wrong (tests/rank_cases.py), not the workload's.  Every padding of a source holds the
sample that would win the rank if it were read; every output sits in a canary."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fixtures as fx
import layouts as lo
import rank_cases as kc
import rank_oracle as ko
import resample_oracle as ro
from mc33_c_library_amd.api import EINVAL, GridDesc, GridResampling, Ranking, load_library

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = ["f32", "u16", "u8", "u32", "f64"]
CANARY = 0xA5


def unsigned(a):
    """a tensor's or array's samples as numpy of the grid's own type (uint16 / uint32 travel as int16 / int32 bit patterns)"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def ranking(rank, radius):
    return Ranking((C.c_uint * 3)(*radius), rank)


def adopted(F, dtype, rank, layout="all", **kw):
    """F adopted at a layout - "all": an odd pitch, a slice with a sample to spare, an odd base offset - inside a flat buffer whose
    every other sample would win the rank, and which ends with the last grid point"""
    from mc33_c_library_amd import DeviceGrid
    lay = lo.layout(layout, F.shape, F.dtype.itemsize)
    flat = lo.to_device(kc.place(F, lay, kc.poison(dtype, rank)))
    g = DeviceGrid(lo.device_view(flat, F.shape, lay), npx=F.shape[2], **kw)
    g.flat = flat
    return g


class Uploaded:
    """F as the library's own pitched copy (mc33hip_upload_contiguous), through the raw ABI"""

    def __init__(self, F, dtype):
        lo.to_device(np.zeros(1, np.float32))   # (torch's HIP runtime first)
        self.lib = load_library(dtype)
        npz, npy, npx = F.shape
        desc = GridDesc(npx, npy, npz, 0, npz - 1, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1), F.dtype.itemsize, 0)
        self.ctx = C.c_void_p()
        assert self.lib.mc33hip_create(C.byref(self.ctx), C.byref(desc)) == 0
        host = np.ascontiguousarray(F)
        assert self.lib.mc33hip_upload_contiguous(self.ctx, C.c_void_p(host.ctypes.data)) == 0

    def close(self):
        self.lib.mc33hip_destroy(self.ctx)


def canaried(shape, dtype, layout):
    """(flat device tensor full of the canary - the layout's padding and the rows behind the grid -, the output grid as a strided
    window of it, the layout)"""
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


def rank_at(src, shape, dtype, rank, radius, dst_layout):
    """mc33hip_rank_grid of a source (an Uploaded or a DeviceGrid) into a canaried buffer"""
    flat, view, lay = canaried(shape, kc.NP_DTYPES[dtype], dst_layout)
    r = ranking(rank, radius)
    rc = src.lib.mc33hip_rank_grid(src.ctx, C.byref(r), C.c_void_p(view.data_ptr()), lay[0], lay[1])
    assert rc == 0, (rc, src.lib.mc33hip_last_error())
    return split(flat, shape, lay)


def check(got, rest, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = int(np.count_nonzero(got.view(np.uint8) != want.view(np.uint8)))
    assert bad == 0, "%s: %d of %d bytes differ from the oracle" % (what, bad, want.nbytes)
    assert np.all(rest.view(np.uint8) == CANARY), "%s: a sample that is no output grid point was written" % what


def both_sources(name, dtype, dst_layouts):
    F, rank, radius, want = kc.case(name, dtype)
    g = adopted(F, dtype, rank)
    try:
        got, rest = rank_at(g, want.shape, dtype, rank, radius, dst_layouts[0])
        check(got, rest, want, "%s %s, adopted at an odd pitch, slice and offset" % (name, dtype))
        assert ko.same_bits(unsigned(g.tensor), F)   # (the source keeps its samples)
    finally:
        g.close()
    u = Uploaded(F, dtype)
    try:
        got, rest = rank_at(u, want.shape, dtype, rank, radius, dst_layouts[1])
        check(got, rest, want, "%s %s, the library's own copy" % (name, dtype))
    finally:
        u.close()


# ---- the case table ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(kc.CASES))
def test_case_table(name):
    both_sources(name, "f32", ("padx_odd", "all"))


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", list(kc.ALL_TYPE_CASES))
def test_every_sample_type(name, dtype):
    both_sources(name, dtype, ("all", "padx16"))


def test_two_calls_return_the_same_bytes():
    F, rank, radius, want = kc.case("no_multiple_of_a_tile_median", "f32")
    g = adopted(F, "f32", rank)
    a = rank_at(g, want.shape, "f32", rank, radius, "dense")[0]
    F2, rank2, radius2, want2 = kc.case("max_8_0_3", "f32")   # (another kernel on the same context in between)
    g2 = adopted(F2, "f32", rank2)
    first = rank_at(g2, want2.shape, "f32", rank2, radius2, "padx16")[0]
    other = rank_at(g2, want2.shape, "f32", kc.MIN, (1, 1, 1), "padx16")[0]
    again = rank_at(g2, want2.shape, "f32", rank2, radius2, "padx16")[0]
    b = rank_at(g, want.shape, "f32", rank, radius, "dense")[0]
    assert ko.same_bits(a, want) and ko.same_bits(a, b) and ko.same_bits(first, want2) and ko.same_bits(again, first)
    assert ko.same_bits(other, ko.rank_filter(F2, kc.MIN, (1, 1, 1)))
    g.close()
    g2.close()


# ---- argument checks --------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing():
    import torch
    from mc33_c_library_amd import DeviceGrid, MC33Error
    F = kc.field("f32", (12, 9, 7), seed=9)
    g = adopted(F, "f32", kc.MAX, "dense")
    flat, view, lay = canaried(F.shape, np.float32, "padx16")
    lib = g.lib
    ptr, pitch, slc = C.c_void_p(view.data_ptr()), lay[0], lay[1]
    ok = ranking(kc.MEDIAN, (1, 1, 1))
    call = lib.mc33hip_rank_grid
    # a null pointer
    assert call(None, C.byref(ok), ptr, pitch, slc) == EINVAL
    assert call(g.ctx, None, ptr, pitch, slc) == EINVAL
    assert call(g.ctx, C.byref(ok), None, pitch, slc) == EINVAL
    # a rank that is none of the three, a radius above its limit
    for rank, radius in ((3, (0, 0, 0)), (-1, (1, 1, 1)), (kc.MEDIAN, (2, 1, 1)), (kc.MEDIAN, (0, 0, 2)), (kc.MIN, (9, 0, 0)), (kc.MAX, (0, 9, 0)),
                         (kc.MAX, (0, 0, 0xFFFFFFFF))):
        bad = ranking(rank, radius)
        assert call(g.ctx, C.byref(bad), ptr, pitch, slc) == EINVAL, (rank, radius)
        with pytest.raises(MC33Error) as e:
            g.rank_into(view, F.shape[2], rank, radius)
        assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        g.rank_into(view, F.shape[2], "mean", 1)
    # a bad pitch or slice
    assert call(g.ctx, C.byref(ok), ptr, F.shape[2] - 1, slc) == EINVAL
    assert call(g.ctx, C.byref(ok), ptr, 0, slc) == EINVAL
    assert call(g.ctx, C.byref(ok), ptr, pitch, pitch * F.shape[1] - 1) == EINVAL
    # not in place: dst inside the source's byte range, and a range that only meets its last sample
    src = g.tensor
    assert call(g.ctx, C.byref(ok), C.c_void_p(src.data_ptr()), src.stride(1), src.stride(0)) == EINVAL
    last = src.data_ptr() + (F.size - 1) * 4
    assert call(g.ctx, C.byref(ok), C.c_void_p(last), src.stride(1), src.stride(0)) == EINVAL
    # a z-slab context
    slab = DeviceGrid(src[2:6], nz_total=F.shape[0] - 1, plane0=2)
    assert call(slab.ctx, C.byref(ok), ptr, pitch, slc) == EINVAL
    slab.close()
    # a context without a grid
    desc = GridDesc(F.shape[2], F.shape[1], F.shape[0], 0, F.shape[0] - 1, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1), 4, 0)
    empty = C.c_void_p()
    assert lib.mc33hip_create(C.byref(empty), C.byref(desc)) == 0
    assert call(empty, C.byref(ok), ptr, pitch, slc) == EINVAL
    lib.mc33hip_destroy(empty)
    torch.cuda.synchronize()
    assert np.all(unsigned(flat).view(np.uint8) == CANARY)   # dst still holds its canary
    assert ko.same_bits(unsigned(g.flat).reshape(F.shape), F)   # ... and the source its samples
    # the context still filters and extracts
    g.rank_into(view, F.shape[2], "median", 1)
    assert ko.same_bits(split(flat, F.shape, lay)[0], ko.rank_filter(F, "median", (1, 1, 1)))
    g.close()


# ---- DeviceGrid.ranked --------------------------------------------------------------------------------------------------------------------

def test_device_grid_ranked_on_a_strided_view_and_the_opening():
    F, rank, radius, want = kc.case("no_multiple_of_a_tile_median", "f32")
    g = adopted(F, "f32", rank, "all", r0=(1.0, 2.0, 3.0), d=(0.5, 0.25, 2.0))
    A, Ai = fx.general_matrices()
    g.set_inclined(A, Ai)
    r = g.ranked()   # the 3 x 3 x 3 median
    assert r.tensor.data_ptr() % 16 == 0 and r.tensor.stride(1) * 4 % 16 == 0 and r.tensor.stride(1) >= F.shape[2]
    assert (r.desc.npx, r.desc.npy, r.desc.npz_resident, r.desc.nz_total) == (F.shape[2], F.shape[1], F.shape[0], F.shape[0] - 1)
    assert tuple(r.desc.r0) == (1.0, 2.0, 3.0) and tuple(r.desc.d) == (0.5, 0.25, 2.0) and r.inclined == g.inclined
    assert ko.same_bits(unsigned(r.tensor[:, :, :F.shape[2]]), want)
    assert ko.same_bits(unsigned(g.ranked(ko.MEDIAN, 1).tensor[:, :, :F.shape[2]]), want)
    opened = g.ranked("min", 1).ranked("max", 1)
    assert ko.same_bits(unsigned(opened.tensor[:, :, :F.shape[2]]), ko.rank_filter(ko.rank_filter(F, "min", (1, 1, 1)), "max", (1, 1, 1)))
    closed = g.ranked("max", (2, 1, 0)).ranked("min", (2, 1, 0))
    assert ko.same_bits(unsigned(closed.tensor[:, :, :F.shape[2]]), ko.rank_filter(ko.rank_filter(F, "max", (2, 1, 0)), "min", (2, 1, 0)))
    g.close()


def test_extraction_of_a_ranked_inclined_grid(reflibs):
    from mc33_c_library_amd import DeviceGrid
    data, r0, d, iso = spiked("f32")
    A, Ai = fx.general_matrices()
    want = ko.rank_filter(data, "median", (1, 1, 1))
    ref = reflibs["f32"].isosurface(want, iso, r0, d, inclined=(A, Ai))
    g = DeviceGrid(lo.to_device(data.reshape(-1)).reshape(data.shape), r0=r0, d=d)
    g.set_inclined(A, Ai)
    r = g.ranked("median", 1)
    g.close()   # (the new grid does not need the old one)
    V, N, T, cnt = r.extract(iso)
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT) and ref.nV > 0
    assert np.array_equal(T.cpu().numpy().view(np.uint32), ref.T) and ko.same_bits(V.cpu().numpy(), ref.V) and ko.same_bits(N.cpu().numpy(), ref.N)


# ---- the C API ------------------------------------------------------------------------------------------------------------------------------

def spiked(dtype, n=48):
    """the cosine field of n^3 points with isolated spikes planted in it: (data, r0, d, an isovalue)"""
    if dtype == "u16":
        data, r0, d, iso, hi, lo_ = fx.cos_field_u16(n, n, n), (0.0, 0.0, 0.0), (0.5, 0.25, 1.0), 30000.5, 65535, 0
    else:
        data, r0, d = fx.cos_field(n, dtype=kc.NP_DTYPES[dtype])
        iso, hi, lo_ = 0.1, 1000.0, -1000.0
    data = data.copy()
    rng = np.random.default_rng(48)
    for k, (z, y, x) in enumerate((z, y, x) for z in range(1, n, 5) for y in range(2, n, 5) for x in range(0, n, 5)):
        if rng.random() < 0.5:
            data[z, y, x] = hi if k & 1 else lo_
    return data, r0, d, iso


def declare(lib):
    L = lib.lib
    L.MC33_create_ranked.restype, L.MC33_create_ranked.argtypes = C.POINTER(lib.MC33), [C.POINTER(lib.MC33), C.POINTER(Ranking)]
    return L


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
    assert np.array_equal(got.T, ref.T) and ko.same_bits(got.V, ref.V) and ko.same_bits(got.N, ref.N), what


def downloaded(lib, L, R):
    Z = L.MC33_resampled_grid(R)
    assert Z
    try:
        return grid_samples(lib, Z), tuple(Z.contents.r0), tuple(Z.contents.d), Z.contents.internal_data
    finally:
        L.free_memory_grd(Z)


@pytest.mark.parametrize("dtype", ["f32", "u16", "f64"])
def test_c_api(products, reflibs, dtype):
    lib = products[dtype]
    L = declare(lib)
    data, r0, d, iso = spiked(dtype)
    want = ko.rank_filter(data, "median", (1, 1, 1))
    plain = reflibs[dtype].isosurface(data, iso, r0, d)
    ref = reflibs[dtype].isosurface(want, iso, r0, d)
    assert plain.nV > ref.nV   # the spikes make surface that the median removes
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    assert M
    R = L.MC33_create_ranked(M, C.byref(ranking(kc.MEDIAN, (1, 1, 1))))
    assert R
    assert not L.MC33_resampled_grid(M)   # an ordinary object has no such grid
    # the refused structs: NULL, and the source as it was and still extracting
    before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
    for bad in (ranking(kc.MEDIAN, (2, 1, 1)), ranking(kc.MIN, (0, 9, 0)), ranking(kc.MAX, (0, 0, 9)), ranking(3, (0, 0, 0)), ranking(-1, (0, 0, 0))):
        assert not L.MC33_create_ranked(M, C.byref(bad))
    assert not L.MC33_create_ranked(M, None) and not L.MC33_create_ranked(None, C.byref(ranking(kc.MEDIAN, (1, 1, 1))))
    assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
    same_host_surface(surface_of(lib, L, M, iso), plain, dtype + " source")
    L.free_MC33(M)   # the source goes first
    L.free_memory_grd(G)
    del keep
    try:
        m = R.contents
        assert (m.nx, m.ny, m.nz) == (data.shape[2] - 1, data.shape[1] - 1, data.shape[0] - 1) and not m.F
        assert tuple(m.O) == tuple(lib.np_real(x) for x in r0) and tuple(m.D) == tuple(lib.np_real(x) for x in d)
        same_host_surface(surface_of(lib, L, R, iso), ref, dtype)
        got, gr0, gd, internal = downloaded(lib, L, R)
        assert ko.same_bits(got, want) and gr0 == tuple(r0) and gd == tuple(d) and internal == 1
        # chained: a ranked object resampled, and ranked again - an opening of the despeckled grid
        R2 = L.MC33_create_resampled(R, C.byref(GridResampling((C.c_double * 3)(1.0, 0.0, 0.0), (C.c_uint * 3)(0, 0, 0), (C.c_uint * 3)(2, 1, 1))))
        assert R2
        want2 = ro.resample(want, (ro.gaussian_taps(1.0), None, None), (2, 1, 1))
        assert ko.same_bits(downloaded(lib, L, R2)[0], want2)
        R2b = L.MC33_create_ranked(R2, C.byref(ranking(kc.MAX, (1, 0, 2))))   # ... and a resampled one ranked
        assert R2b and ko.same_bits(downloaded(lib, L, R2b)[0], ko.rank_filter(want2, kc.MAX, (1, 0, 2)))
        L.free_MC33(R2b)
        L.free_MC33(R2)
        R3 = L.MC33_create_ranked(R, C.byref(ranking(kc.MIN, (1, 1, 1))))
        assert R3
        R4 = L.MC33_create_ranked(R3, C.byref(ranking(kc.MAX, (1, 1, 1))))
        assert R4
        L.free_MC33(R3)
        want4 = ko.rank_filter(ko.rank_filter(want, kc.MIN, (1, 1, 1)), kc.MAX, (1, 1, 1))
        assert ko.same_bits(downloaded(lib, L, R4)[0], want4)
        same_host_surface(surface_of(lib, L, R4, iso), reflibs[dtype].isosurface(want4, iso, r0, d), dtype + " opened")
        L.free_MC33(R4)
        # MC33_grid_changed does nothing on it, and it extracts again
        L.MC33_grid_changed(R)
        same_host_surface(surface_of(lib, L, R, iso), ref, dtype + " again")
    finally:
        L.free_MC33(R)


def test_c_api_normal_neg_flavour():
    from mc33_capi import MC33Lib, product_path, ref_path
    lib, ref = MC33Lib(product_path("f32", nneg=True), "f32"), MC33Lib(ref_path("f32", nneg=True), "f32")
    L = declare(lib)
    data, r0, d, iso = spiked("f32")
    want = ko.rank_filter(data, "max", (1, 1, 0))
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    R = L.MC33_create_ranked(M, C.byref(ranking(kc.MAX, (1, 1, 0))))
    assert M and R
    try:
        same_host_surface(surface_of(lib, L, R, iso), ref.isosurface(want, iso, r0, d), "nneg")
    finally:
        L.free_MC33(R)
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refuses_an_object_on_several_slabs(launcher):
    out = launcher.run([sys.executable, os.path.join(HERE, "capi_ranked_refusal_worker.py")], env={"MC33_HIP_DEVICES": "0,0"}, timeout=300)
    assert out["rc"] == 0 and "ranked refused: 1 0" in out["stdout"], out
