"""The contour spectrum of the grid, on the GPU: k_sp_spectrum through DeviceGrid.spectrum, the raw ABI and the C
API.  Every count is compared with tests/spectrum_oracle.py exactly - integers, no tolerance anywhere - and with the count path
of the extraction, which this feature does not touch.  The shapes are the smallest at which the tiling, the packed loads and the
counters can go wrong (tests/spectrum_cases.py), not the workload's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import layouts as lo
import spectrum_cases as sc
import spectrum_oracle as so
from mc33_c_library_amd.api import GridResampling
from spectrum_cases import c_spectrum, report

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = sc.TYPES


def grid_of(F, layout="dense", isos=(0.0,), planes=None, **kw):
    """F - or its planes [planes[0], planes[1]] as a z-slab context - adopted at a layout inside a flat buffer poisoned at the
    isovalues"""
    from mc33_c_library_amd import DeviceGrid
    if planes is not None:
        kw.update(nz_total=F.shape[0] - 1, plane0=planes[0])
        F = F[planes[0]:planes[1] + 1]
    lay = lo.layout(layout, F.shape, F.dtype.itemsize)
    flat = lo.to_device(lo.place(F, lay, list(isos) or [0.0]))
    g = DeviceGrid(lo.device_view(flat, F.shape, lay), npx=F.shape[2], **kw)
    g.flat, g.lay = flat, lay
    return g


def as_oracle(s):
    return so.Spectrum(s.cut_cells, s.histogram, s.points, s.cells, s.nan_samples, s.sample_min, s.sample_max)


def check(got, want, what=""):
    got = as_oracle(got)
    assert so.same(got, want), "%s\n%s" % (what, report(got, want))


# ---- the case table ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_table(name):
    F, isos, want = sc.case(name, "f32")
    g = grid_of(F, isos=isos)
    try:
        check(g.spectrum(isos), want, name)
    finally:
        g.close()


@pytest.mark.parametrize("dtype", ["u16", "u8", "u32", "f64"])
def test_every_sample_type(dtype):
    for name in sc.cases_of(dtype):
        F, isos, want = sc.case(name, dtype)
        g = grid_of(F, "padx16", isos=isos)
        try:
            check(g.spectrum(isos), want, "%s %s" % (name, dtype))
        finally:
            g.close()


@pytest.mark.parametrize("dtype", TYPES)
def test_every_layout_gives_the_oracles_result(dtype):
    """every legal pitch, slice and alignment, the padding poisoned at the isovalues; 1- and 2-byte samples reach both the packed
    form and the one that loads a sample per lane"""
    from mc33_c_library_amd import Range
    forms = set()
    for name in (sc.LAYOUT_CASE, sc.LAYOUT_CASE_2):
        F, isos, want = sc.case(name, dtype)
        for layout in lo.LAYOUTS:
            g = grid_of(F, layout, isos=isos)
            try:
                p4 = lo.predicates(g.tensor.data_ptr(), g.lay[0], g.lay[1], F.dtype.itemsize)[4]
                forms.add(all(p4))
                check(g.spectrum(isos), want, "%s %s %s" % (name, dtype, layout))
                check(g.spectrum(isos, Range(0, 1, 0, 0)), so.spectrum(F, isos, 0, 1), "%s %s %s first slice" % (name, dtype, layout))
            finally:
                g.close()
    assert forms == ({True, False} if F.dtype.itemsize < 4 else {True})


# ---- ranges ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("parts", [1, 3, 8])
def test_disjoint_ranges_add_up_to_the_whole_grid(dtype, parts):
    from mc33_c_library_amd import Range
    for name in ("tile_minus_1_beyond_cos", "narrow_dword_plus_3_noise", "small_noise"):
        F, isos, want = sc.case(name, dtype)
        ranges = sc.split(F.shape[0] - 1, parts)
        g = grid_of(F, isos=isos)
        try:
            got = []
            for a, b in ranges:
                got.append(as_oracle(g.spectrum(isos, Range(a, b, 7, 9))))   # (ghost_below and id_base are ignored)
                assert so.same(got[-1], so.spectrum(F, isos, a, b)), (name, a, b)
            assert so.same(so.add(got), want), name
        finally:
            g.close()
    if parts == 8:   # one-slice ranges
        assert all(b - a == 1 for a, b in sc.split(sc.SHAPES["small"][2] - 1, parts))


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_slab_contexts(dtype):
    """contexts that hold the planes of one slab only (plane0 > 0): their own slices add up to the whole grid; a range whose planes
    are not resident is refused"""
    from mc33_c_library_amd import MC33Error, Range
    from mc33_c_library_amd.api import EINVAL
    from mc33_c_library_amd.slabs import Slab
    F, isos, want = sc.case("one_point_beyond_noise", dtype)
    nzt = F.shape[0] - 1
    got = []
    for rank in range(3):
        slab = Slab(rank, 3, nzt)
        g = grid_of(F, "padx4", isos=isos, planes=(slab.p_lo, slab.p_hi))
        try:
            assert rank == 0 or g.desc.plane0 > 0
            got.append(as_oracle(g.spectrum(isos, slab.range())))
            assert so.same(got[-1], so.spectrum(F, isos, slab.z_begin, slab.z_end)), rank
            if rank == 1:
                check(g.spectrum(isos), so.spectrum(F, isos, slab.p_lo, slab.p_hi), "the default range: every slice whose planes are resident")
                for bad in (Range(slab.p_lo - 1, slab.z_end, 0, 0), Range(slab.z_begin, slab.p_hi + 1, 0, 0), Range(0, nzt, 0, 0)):
                    with pytest.raises(MC33Error) as e:
                        g.spectrum(isos, bad)
                    assert e.value.code == EINVAL
        finally:
            g.close()
    assert so.same(so.add(got), want)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    from mc33_c_library_amd import MC33Error, Range
    from mc33_c_library_amd.api import EINVAL, Spectrum
    F, isos, want = sc.case("small_noise", "f32")
    g = grid_of(F, isos=isos)
    try:
        nzt = F.shape[0] - 1
        nan = float("nan")
        for bad in ([0.0, nan], [nan], [0.0, 0.0], [1.0, 0.5], [1.0, 1.0 + 2.0 ** -40], [float(k) for k in range(256)], [0.0, float("inf"), float("inf")]):
            with pytest.raises(MC33Error) as e:
                g.spectrum(bad)
            assert e.value.code == EINVAL, bad
        for rng in (Range(0, 0, 0, 0), Range(2, 1, 0, 0), Range(0, nzt + 1, 0, 0), Range(nzt, nzt, 0, 0)):
            with pytest.raises(MC33Error) as e:
                g.spectrum(isos, rng)
            assert e.value.code == EINVAL
        # null pointers where a size is not zero, through the raw entry point; nothing is written
        arr = (C.c_double * 2)(0.0, 1.0)
        cut = (C.c_ulonglong * 2)(5, 5)
        hist = (C.c_ulonglong * 3)(5, 5, 5)
        rng = g.full_range()
        fn = g.lib.mc33hip_grid_spectrum

        def call(ctx, r, isos_p, n, cut_p, hist_p):
            a = Spectrum()
            a.isos, a.n, a.cut_cells, a.histogram = isos_p, n, cut_p, hist_p
            return fn(ctx, r, C.byref(a))

        assert call(g.ctx, C.byref(rng), None, 2, cut, hist) == EINVAL and call(g.ctx, C.byref(rng), arr, 2, None, hist) == EINVAL
        assert call(g.ctx, C.byref(rng), arr, 2, cut, None) == EINVAL and call(g.ctx, C.byref(rng), None, 0, None, None) == EINVAL
        assert call(g.ctx, None, arr, 2, cut, hist) == EINVAL and call(None, C.byref(rng), arr, 2, cut, hist) == EINVAL
        assert fn(g.ctx, C.byref(rng), None) == EINVAL and call(g.ctx, C.byref(rng), arr, 256, cut, hist) == EINVAL
        assert list(cut) == [5, 5] and list(hist) == [5, 5, 5]
        assert call(g.ctx, C.byref(rng), None, 0, None, hist) == 0 and hist[0] == F.size and list(hist)[1:] == [5, 5]   # n == 0 needs the histogram only
        check(g.spectrum(isos), want, "after the refusals")
    finally:
        g.close()
    # a context without a grid
    import torch
    from mc33_c_library_amd.api import GridDesc, load_library
    lib = load_library("f32")
    ctx = C.c_void_p()
    desc = GridDesc(4, 4, 4, 0, 3, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1), 4, torch.cuda.current_device())
    assert lib.mc33hip_create(C.byref(ctx), C.byref(desc)) == 0
    try:
        a = Spectrum()
        h = (C.c_ulonglong * 1)()
        a.histogram = h
        r = Range(0, 3, 0, 0)
        assert lib.mc33hip_grid_spectrum(ctx, C.byref(r), C.byref(a)) == EINVAL
    finally:
        lib.mc33hip_destroy(ctx)


def test_uploaded_grid_and_the_ladder():
    """the library's own pitched copy (mc33hip_upload_contiguous) gives what the adopted buffer gives; spectrum_ladder is the two
    calls it says it is"""
    import torch
    from mc33_c_library_amd import isovalue_ladder
    for dtype in ("f32", "u8"):
        F, isos, want = sc.case("dword_plus_3_noise", dtype)
        g = grid_of(F, isos=isos)
        try:
            assert g.lib.mc33hip_upload_contiguous(g.ctx, C.c_void_p(np.ascontiguousarray(F).ctypes.data)) == 0
            check(g.spectrum(isos), want, "uploaded " + dtype)
        finally:
            g.close()
    F, isos, want = sc.case("one_point_beyond_cos", "f32")
    g = grid_of(F)
    try:
        got = g.spectrum_ladder(11)
        steps = isovalue_ladder(float(F.min()), float(F.max()), 11)
        assert got.isovalues == steps and got.busiest() in steps
        check(got, so.spectrum(F, steps), "ladder")
        assert got.histogram[0] > 0 and got.histogram[-1] > 0 and (got.cut_cells > 0).all()
    finally:
        g.close()
    g = grid_of(sc.case("constant", "f32")[0])
    try:
        with pytest.raises(ValueError):
            g.spectrum_ladder(4)
    finally:
        g.close()
    del torch


# ---- against the count path of the extraction -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,name,n", [("f32", "special_values", 9), ("u8", "plateau_isovalues_equal_samples", 5), ("u8", "one_point_beyond_noise", 12),
                                          ("u16", "tile_minus_1_beyond_cos", 7), ("f64", "special_values", 9), ("u32", "one_point_beyond_cos", 7)])
def test_cut_cells_are_the_active_cells_of_the_count_path(dtype, name, n):
    from mc33_c_library_amd import Range
    F, isos, want = sc.case(name, dtype)
    assert len(isos) == n
    if "special" in name:
        assert np.isnan(F).any()
    if name.startswith("plateau"):
        assert all(float(v).is_integer() for v in isos)
    nzt = F.shape[0] - 1
    g = grid_of(F, "padx16", isos=isos)
    try:
        got = g.spectrum(isos)
        check(got, want, name)
        counted = [int(g.count(v, Range(0, nzt, 0, 0)).active_cells) for v in isos]
        assert [int(x) for x in got.cut_cells] == counted
    finally:
        g.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------------

def _outputs(g, cnt):
    import torch
    V = torch.zeros((cnt.nV + 8, 3), dtype=torch.float32, device=g.device)
    N = torch.zeros((cnt.nV + 8, 3), dtype=torch.float32, device=g.device)
    T = torch.zeros((cnt.nT + 8, 3), dtype=torch.int32, device=g.device)
    return V, N, T


def _bytes(g, *tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def test_count_spectrum_emit_returns_the_bytes_of_count_emit():
    F, isos, want = sc.case("tile_minus_1_beyond_cos", "f32")
    iso = isos[3]
    for layout in ("dense", "padx_odd"):
        g = grid_of(F, layout, isos=isos)
        try:
            cnt = g.count(iso)
            assert cnt.nV > 1000
            V, N, T = _outputs(g, cnt)
            g.emit_into(V, N, T)
            plain = _bytes(g, V, N, T)
            cnt2 = g.count(iso)
            first = g.spectrum(isos)
            second = g.spectrum(isos[::2])   # another ladder in between
            V2, N2, T2 = _outputs(g, cnt2)
            g.emit_into(V2, N2, T2)
            assert (cnt2.nV, cnt2.nT, cnt2.active_cells) == (cnt.nV, cnt.nT, cnt.active_cells)
            assert _bytes(g, V2, N2, T2) == plain
            check(first, want)
            check(second, so.spectrum(F, isos[::2]))
            assert int(first.cut_cells[3]) == cnt.active_cells
        finally:
            g.close()


def test_prepare_many_spectrum_extract_returns_the_bytes_without_the_spectrum():
    F, isos, want = sc.case("tile_minus_1_beyond_cos", "f32")
    g = grid_of(F, isos=isos)

    def run(with_spectrum):
        out = []
        g.prepare_many(isos)
        if with_spectrum:
            check(g.spectrum(isos), want)
        for k, v in enumerate(isos):
            cnt = g.count(v)
            if with_spectrum and k == 3:   # ... and between a count and its extraction
                check(g.spectrum(isos[:2]), so.spectrum(F, isos[:2]))
            V, N, T = _outputs(g, cnt)
            c2, ok = g.extract_into(v, V, N, T)
            assert ok and (c2.nV, c2.nT) == (cnt.nV, cnt.nT)
            out.append(((c2.nV, c2.nT, c2.active_cells), _bytes(g, V, N, T)))
        return out

    try:
        plain = run(False)
        assert sum(1 for c, _ in plain if c[0] > 0) >= 5
        assert run(True) == plain
        assert [c[2] for c, _ in plain] == [int(x) for x in want.cut_cells]
    finally:
        g.close()


def test_two_calls_return_the_same_bytes():
    for dtype, name in (("f32", "n_255_noise"), ("u8", "n_255_noise"), ("f64", "special_values")):
        F, isos, want = sc.case(name, dtype)
        g = grid_of(F, isos=isos)
        try:
            a, b = g.spectrum(isos), g.spectrum(isos)
            assert a.cut_cells.tobytes() == b.cut_cells.tobytes() and a.histogram.tobytes() == b.histogram.tobytes()
            assert (a.points, a.cells, a.nan_samples, a.sample_min, a.sample_max) == (b.points, b.cells, b.nan_samples, b.sample_min, b.sample_max)
            check(a, want)
        finally:
            g.close()


# ---- the C API ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u16", "f64", "u8"])
def test_c_api(products, dtype):
    lib = products[dtype]
    L = lib.lib
    F, isos, want = sc.case("one_point_beyond_noise", dtype)
    data = np.array(F)
    G, keep = lib.make_grid(data)
    M = L.create_MC33(G)
    assert M
    try:
        nV, nT = C.c_uint(), C.c_uint()
        L.size_of_isosurface(M, lib.real(isos[2]), C.byref(nV), C.byref(nT))
        before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
        got = c_spectrum(lib, L, M, isos)
        assert so.same(got, want), report(got, want)
        assert so.same(c_spectrum(lib, L, M, []), so.spectrum(F, []))
        assert c_spectrum(lib, L, M, [1.0, 1.0]) == -1 and c_spectrum(lib, L, M, [float(k) for k in range(256)]) == -1
        assert L.MC33_grid_spectrum(M, None, 2, None, None, None) == -1
        assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        # samples rewritten in place: seen after MC33_grid_changed, not before
        keep[1:3] = keep[1:3][:, ::-1].copy()
        keep[0, 0, 0] = data.max()
        assert so.same(c_spectrum(lib, L, M, isos), want)
        L.MC33_grid_changed(M)
        assert so.same(c_spectrum(lib, L, M, isos), so.spectrum(keep, isos))
        assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        # an object made by MC33_create_resampled: every second point, no taps
        R = L.MC33_create_resampled(M, C.byref(GridResampling((C.c_double * 3)(0, 0, 0), (C.c_uint * 3)(0, 0, 0), (C.c_uint * 3)(2, 2, 2))))
        assert R
        try:
            rb = bytes(C.string_at(C.addressof(R.contents), C.sizeof(lib.MC33)))
            got = c_spectrum(lib, L, R, isos)
            assert so.same(got, so.spectrum(np.ascontiguousarray(keep[::2, ::2, ::2]), isos))
            assert bytes(C.string_at(C.addressof(R.contents), C.sizeof(lib.MC33))) == rb
        finally:
            L.free_MC33(R)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_three_slabs_on_one_device(launcher):
    """MC33_HIP_DEVICES=0,0,0 is read when the extractor is created: a fresh process (tests/spectrum_slab_worker.py)"""
    out = launcher.run([sys.executable, os.path.join(HERE, "spectrum_slab_worker.py")], env={"MC33_HIP_DEVICES": "0,0,0"}, timeout=300)
    assert out["rc"] == 0 and "SPECTRUM_SLABS_OK 4" in out["stdout"], out
