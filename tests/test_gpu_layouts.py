"""GPU tests of adopted device grids at every legal pitch, slice and alignment (include/mc33_hip.h: mc33hip_adopt_device,
mc33hip_property_adopt_device; mc33_c_library_amd.DeviceGrid passes a tensor's strides straight through).

What the kernels do depends on the layout in three places: the packed dword sweep of 1- and 2-byte samples needs base, pitch
and slice to be multiples of 4 bytes, the staged rows of the vertex pass need them to be multiples of 16 bytes, and every
consumer of the grid indexes (z - z0) * slice + y * pitch + x.  Here every grid sits in a flat tensor in one of the layouts
of tests/layouts.py, everything that is not a grid point holding poison; the expected surface is always the unmodified
reference's (oracle/_ref) on the dense numpy array, and every comparison is exact: counts, T as uint32, V and N by bit pattern.
There is no tolerance anywhere in this file.  The forms are reached through the alignment predicates alone - no switch of the
library is set except MC33_HIP_SLOW_SLOTS where a test says so."""
import ctypes as C
import functools

import numpy as np
import pytest

import fixtures as fx
import layouts as lo
from canaries import canaried as _canaried, only_the_rows_were_written as _only_the_rows_were_written, windows as _windows, words

pytestmark = pytest.mark.gpu

NP = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
DTYPES = tuple(NP)
ALL_LAYOUTS = lo.LAYOUTS + ("padx16_npx",)  # (padx16 handed over at its full width with DeviceGrid's npx=)
ROUGH = (20, 66, 258)


@functools.lru_cache(maxsize=None)
def crop(W):
    """(35, 66, W): two row segments (SEG_CELLS = 256), two y tiles (63 rows), more than one z tile; 258: nx & 3 == 1, 261: nx & 3 == 0"""
    c = np.ascontiguousarray(fx.cos_field(W)[0][100:135, 90:156, :])
    assert c.shape == (35, 66, W)
    return c


# name -> (() -> dense array, isovalues of the extraction test, smooth?)
def _grids(dtype):
    g = {}
    for W in (258, 261):
        if dtype == "f32":
            g["smooth%d" % W] = (lambda W=W: crop(W), (1.0,), True)
            g["smoothq%d" % W] = (lambda W=W: np.rint(crop(W) * np.float32(50)).astype(np.float32), (50.0,), True)  # ~11 000 samples equal the isovalue
        elif dtype == "f64":
            g["smooth%d" % W] = (lambda W=W: crop(W).astype(np.float64), (1.0,), True)
        elif dtype == "u8":
            g["smooth%d" % W] = (lambda W=W: np.rint(128.0 + 40.0 * crop(W).astype(np.float64)).astype(np.uint8), (168.0, 168.5), True)
        elif dtype == "u16":
            g["smooth%d" % W] = (lambda W=W: np.rint(32768.0 + 10000.0 * crop(W).astype(np.float64)).astype(np.uint16), (42768.0, 42768.5), True)
        else:
            g["smooth%d" % W] = (lambda W=W: np.rint(2147483648.0 + 5e8 * crop(W).astype(np.float64)).astype(np.uint32), (2647483648.0,), True)
    if dtype == "f32":
        g["rough"] = (lambda: fx.noise_f32(0, 11, shape=ROUGH), (0.05,), False)
        g["roughq"] = (lambda: fx.noise_quant(0, 5, shape=ROUGH), (0.0,), False)
    elif dtype == "f64":
        g["roughq"] = (lambda: fx.noise_quant(0, 5, shape=ROUGH).astype(np.float64), (1.0,), False)
    else:
        g["rough"] = (lambda: {"u8": fx.noise_u8, "u16": fx.noise_u16, "u32": fx.noise_u32}[dtype](0, 2, 7, shape=ROUGH), (3.0, 2.5), False)
    return g


GRIDS = {d: _grids(d) for d in DTYPES}
# four isovalues for one pass over the smooth grid: two that no sample can equal first (integer types: ZM 2 as a pair), an integer
# one (ZM 1), and -0.0 (ZM 0 for the whole pass)
MANY = {"f32": (1.0, 0.5, 1.5, 2.0), "f64": (1.0, 0.5, 1.5, 2.0), "u8": (168.5, 150.5, 168.0, -0.0),
        "u16": (42768.5, 45000.5, 42768.0, -0.0), "u32": (2647483648.5, 2447483648.5, 2647483648.0, -0.0)}


@functools.lru_cache(maxsize=None)
def dense(dtype, grid):
    a = GRIDS[dtype][grid][0]()
    assert a.dtype == NP[dtype]
    a.setflags(write=False)
    return a


def poison_isos(dtype, grid):
    return tuple(GRIDS[dtype][grid][1]) + (MANY[dtype] if grid == "smooth258" else ())


_refs, _tensors = {}, {}


def reference(reflibs, dtype, grid, iso):
    """The expected surface: the unmodified reference on the dense array, once per (dtype, grid, isovalue)"""
    key = (dtype, grid, repr(float(iso)))
    if key not in _refs:
        _refs[key] = reflibs[dtype].isosurface(dense(dtype, grid), iso)
    return _refs[key]


def placed(dtype, grid, layout):
    """(flat device tensor, the grid as a strided window of it, npx, (pitch, slice, off)): built once per (dtype, grid, layout)"""
    key = (dtype, grid, layout)
    if key not in _tensors:
        data = dense(dtype, grid)
        full = layout == "padx16_npx"
        lay = lo.layout("padx16" if full else layout, data.shape, data.dtype.itemsize)
        flat = lo.to_device(lo.place(data, lay, poison_isos(dtype, grid)))
        _tensors[key] = (flat, lo.device_view(flat, data.shape, lay, full_width=full), data.shape[2], lay)
    return _tensors[key]


def device_grid(dtype, grid, layout, **kw):
    from mc33_c_library_amd import DeviceGrid
    flat, view, npx, lay = placed(dtype, grid, layout)
    g = DeviceGrid(view, npx=npx, **kw)
    g.flat = flat
    return g


def same(got, ref, what):
    V, N, T, cnt = got
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT), what
    v, n, t = V.cpu().numpy(), N.cpu().numpy(), T.cpu().numpy().view(np.uint32)
    assert v.dtype == ref.V.dtype and v.shape == ref.V.shape and n.shape == ref.N.shape, what
    assert np.array_equal(t, ref.T), what
    bad_v, bad_n = int(np.count_nonzero(words(v) != words(ref.V))), int(np.count_nonzero(words(n) != words(ref.N)))
    assert bad_v == 0 and bad_n == 0, "%s: %d position words, %d normal words differ" % (what, bad_v, bad_n)


# ---- 0: the inputs reach every form -------------------------------------------------------------------------------------------

def test_the_matrix_reaches_every_form_through_the_predicates():
    """Recomputes the two host predicates from data_ptr() and the strides of every tensor the tests below hand over - base,
    pitch * size and slice * size all multiples of 4 (packed sweep, 1- and 2-byte samples), all multiples of 16 (staged rows) -
    and prints the form each one selects.  A check of the inputs: nothing inside the library is read."""
    isolated = {"offs": 0, "pitch_only": 1, "slice_odd": 2}  # layout -> the one term (base, pitch, slice) that fails
    for dtype in DTYPES:
        size = np.dtype(NP[dtype]).itemsize
        narrow = size < 4
        seen = set()
        for grid in GRIDS[dtype]:
            for layout in ALL_LAYOUTS:
                flat, view, npx, lay = placed(dtype, grid, layout)
                assert flat.data_ptr() % 256 == 0
                assert view.data_ptr() == flat.data_ptr() + lay[2] * size and (view.stride(1), view.stride(0)) == lay[:2]
                p = lo.predicates(view.data_ptr(), view.stride(1), view.stride(0), size)
                ok4, ok16 = all(p[4]), all(p[16])
                seen.add((ok4, ok16))
                print("%-3s %-9s %-11s pitch %4d slice %6d off %2d: sweep %-8s vertex rows %s" % (
                    dtype, grid, layout, lay[0], lay[1], lay[2], ("packed" if ok4 else "unpacked") if narrow else "-", "staged" if ok16 else "direct"))
                assert not (ok16 and not ok4)
                if layout in isolated:
                    want = tuple(k != isolated[layout] for k in range(3))
                    assert p[16] == want, (dtype, grid, layout, p)
                    if narrow:
                        assert p[4] == want, (dtype, grid, layout, p)
                if layout == "padx_odd":
                    assert not p[16][1] and (not narrow or not p[4][1]), (dtype, grid, layout, p)
                if layout in ("padx16", "padx16_npx", "pady"):
                    assert ok4 and ok16
                if layout == "padx4":
                    assert ok4 and not ok16
                if layout == "pady":
                    assert lay[1] != lay[0] * view.shape[1]
        assert (True, True) in seen and (True, False) in seen, (dtype, seen)
        if narrow:
            assert (False, False) in seen, (dtype, seen)


# ---- 1: extraction --------------------------------------------------------------------------------------------------------------

def _extract_all(reflibs, dtype, layout):
    for grid, (_, isos, smooth) in GRIDS[dtype].items():
        g = device_grid(dtype, grid, layout)
        for iso in isos:
            ref = reference(reflibs, dtype, grid, iso)
            assert ref.nV > (5000 if smooth else 100000), (dtype, grid, iso, ref.nV)
            for rep in range(2):  # (the second call picks its emit kernels from the first call's counts)
                same(g.extract(iso), ref, (dtype, grid, layout, iso, rep))
        g.close()


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_extraction(reflibs, dtype, layout):
    _extract_all(reflibs, dtype, layout)


@pytest.mark.parametrize("slots", ["0", "1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_extraction_with_either_slow_emit_kernel(reflibs, monkeypatch, dtype, slots):
    monkeypatch.setenv("MC33_HIP_SLOW_SLOTS", slots)  # (read when the context is made)
    _extract_all(reflibs, dtype, "all")


# ---- 2: several isovalues per pass -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["pady", "padx_odd", "all"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_several_isovalues_per_pass(reflibs, dtype, layout):
    isos = MANY[dtype]
    refs = [reference(reflibs, dtype, "smooth258", iso) for iso in isos]
    assert sum(r.nV > 5000 for r in refs) >= 2
    g = device_grid(dtype, "smooth258", layout)
    g.prepare_many(isos)
    for k in reversed(range(4)):
        same(g.extract(isos[k]), refs[k], (dtype, layout, "prepare_many", isos[k]))
    for pair in ((0, 1), (1, 2)):  # (integer types: a pair nothing can equal, a pair with an integer isovalue)
        g.sweep_many([isos[k] for k in pair])
        for k in pair:
            same(g.extract(isos[k]), refs[k], (dtype, layout, "sweep_many", pair, isos[k]))
    g.close()


# ---- 3: z-slabs on a strided buffer ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["pady", "all"])
@pytest.mark.parametrize("dtype,grid,iso", [("f32", "roughq", 0.0), ("u16", "rough", 3.0)])
def test_z_slabs_as_windows_of_one_strided_buffer(reflibs, dtype, grid, iso, layout):
    """test_gpu_device_api.slabbed with every slab an as_strided window (off += p_lo * slice) of ONE flat tensor"""
    import torch
    from mc33_c_library_amd import DeviceGrid, Range
    ref = reference(reflibs, dtype, grid, iso)
    flat, view, npx, (pitch, slc, off) = placed(dtype, grid, layout)
    npz, npy = view.shape[0], view.shape[1]
    nz_total = npz - 1
    bounds = [0, 7, 8, nz_total]
    grids, counts = [], []
    for zb, ze in zip(bounds[:-1], bounds[1:]):
        ghost = 1 if zb else 0
        p_lo, p_hi = max(zb - ghost - 1, 0), min(ze + 1, nz_total)
        window = torch.as_strided(flat, (p_hi - p_lo + 1, npy, npx), (slc, pitch, 1), off + p_lo * slc)
        g = DeviceGrid(window, nz_total=nz_total, plane0=p_lo)
        counts.append(g.count(iso, Range(zb, ze, ghost, 0)))
        grids.append(g)
    assert sum(c.nV for c in counts) == ref.nV and sum(c.nT for c in counts) == ref.nT
    Vs, Ns, Ts, base = [], [], [], 0
    for g, c in zip(grids, counts):
        V = torch.empty((max(c.nV, 1), 3), dtype=torch.float32, device="cuda")
        N = torch.empty_like(V)
        T = torch.empty((max(c.nT, 1), 3), dtype=torch.int32, device="cuda")
        g.emit_into(V, N, T, base)
        torch.cuda.synchronize()
        Vs.append(V[:c.nV].cpu().numpy()); Ns.append(N[:c.nV].cpu().numpy()); Ts.append(T[:c.nT].cpu().numpy().view(np.uint32))
        base += c.nV
        g.close()
    assert np.array_equal(np.concatenate(Ts), ref.T)
    assert np.array_equal(words(np.concatenate(Vs)), words(ref.V)) and np.array_equal(words(np.concatenate(Ns)), words(ref.N))


# ---- 4: the property grid with a layout of its own ------------------------------------------------------------------------------------

def _property_field(dtype, shape):
    if dtype == "f32":
        return fx.noise_f32(0, 77, shape=shape) * np.float32(1000.0)
    if dtype == "f64":
        return fx.noise_f32(0, 5, shape=shape).astype(np.float64) * 1e6 + 1e-3
    return fx.noise_u8(0, 5, shape=shape)


@pytest.mark.parametrize("dtype,grid_layout,prop_layout", [("f32", "padx16", "all"), ("u8", "padx16", "all"), ("f64", "padx16", "all"),
                                                           ("f32", "all", "pady"), ("f32", "dense", "padx16_npx")])
def test_property_grid_with_a_layout_of_its_own(reflibs, dtype, grid_layout, prop_layout):
    import measure_oracle as mo
    import property_oracle as po
    from measure_cases import check_measures
    iso = {"f32": 1.0, "f64": 1.0, "u8": 168.5}[dtype]
    r0, d = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    data = dense(dtype, "smooth258")
    ref = reference(reflibs, dtype, "smooth258", iso)
    assert ref.nV > 5000
    P = _property_field(dtype, data.shape)
    full = prop_layout == "padx16_npx"
    play = lo.layout("padx16" if full else prop_layout, P.shape, P.dtype.itemsize)
    pflat = lo.to_device(lo.place(P, play, (iso,)))  # (poisoned like the grid's)
    pview = lo.device_view(pflat, P.shape, play, full_width=full)
    assert (pview.shape[2] > data.shape[2]) == full
    want = po.sample_property(ref.V, r0, d, P)
    g = device_grid(dtype, "smooth258", grid_layout)
    g.attach_property(pview)
    Vd = lo.to_device(ref.V)
    got = g.sample_property(Vd).cpu().numpy()
    assert np.array_equal(words(got), words(want)), "%d of %d values differ" % (np.count_nonzero(words(got) != words(want)), got.size)
    V2, N2, T2, cnt, p2 = g.extract(iso, with_property=True)
    same((V2, N2, T2, cnt), ref, (dtype, grid_layout, prop_layout))
    assert np.array_equal(words(p2.cpu().numpy()), words(want))
    check_measures("%s %s/%s" % (dtype, grid_layout, prop_layout), g.measure_iso(iso, with_property=True),
                   mo.measure(ref.V, ref.T, r0, d, data.shape, P=want))
    g.close()


# ---- 5: outputs inside larger tensors ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["padx16", "all"])
@pytest.mark.parametrize("dtype,grid,iso", [("f32", "smooth258", 1.0), ("f32", "roughq", 0.0), ("u8", "rough", 3.0), ("f64", "smooth258", 1.0)])
def test_outputs_inside_larger_tensors(reflibs, dtype, grid, iso, layout):
    import torch
    ref = reference(reflibs, dtype, grid, iso)
    g = device_grid(dtype, grid, layout)
    for rep in range(2):  # extract_into, twice (the second with the first call's counts)
        V, N, T = _canaried(ref.nV, ref.nT, dtype == "f64")
        cnt, ok = g.extract_into(iso, *_windows(V, N, T, ref.nV, ref.nT))
        torch.cuda.synchronize()
        assert ok and (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
        _only_the_rows_were_written(V, N, T, ref, (dtype, grid, layout, "extract_into", rep))
    V, N, T = _canaried(ref.nV, ref.nT, dtype == "f64")  # count, then emit_into
    cnt = g.count(iso)
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
    g.emit_into(*_windows(V, N, T, ref.nV, ref.nT))
    torch.cuda.synchronize()
    _only_the_rows_were_written(V, N, T, ref, (dtype, grid, layout, "emit_into"))
    g.close()


@pytest.mark.parametrize("layout", ["padx16", "all"])
def test_two_slabs_write_one_canaried_array_at_device_bases(reflibs, layout):
    """count_async / counts_to_device / bases_from_table / emit_at_device_bases with concatenated=True: two slabs of the rough
    float grid write their rows into ONE window of one canaried array"""
    import torch
    from mc33_c_library_amd import DeviceGrid, Range
    dtype, grid, iso = "f32", "roughq", 0.0
    ref = reference(reflibs, dtype, grid, iso)
    flat, view, npx, (pitch, slc, off) = placed(dtype, grid, layout)
    npz, npy = view.shape[0], view.shape[1]
    nz_total = npz - 1
    bounds = [0, 8, nz_total]
    grids, ranges = [], []
    for zb, ze in zip(bounds[:-1], bounds[1:]):
        ghost = 1 if zb else 0
        p_lo, p_hi = max(zb - ghost - 1, 0), min(ze + 1, nz_total)
        grids.append(DeviceGrid(torch.as_strided(flat, (p_hi - p_lo + 1, npy, npx), (slc, pitch, 1), off + p_lo * slc), nz_total=nz_total, plane0=p_lo))
        ranges.append(Range(zb, ze, ghost, 0))
    for attempt in range(2):  # (the first pass sizes every slab's record buffers through the synchronous path)
        for g, rg in zip(grids, ranges):
            g.count(iso, rg)
    table = torch.zeros(4, dtype=torch.int64, device="cuda")
    V, N, T = _canaried(ref.nV, ref.nT, False)
    win = _windows(V, N, T, ref.nV, ref.nT)
    for r, (g, rg) in enumerate(zip(grids, ranges)):
        g.count_async(iso, rg)
        g.counts_to_device(table[2 * r:2 * r + 2])
    for r, g in enumerate(grids):
        g.bases_from_table(table, 2, r, True)
        g.emit_at_device_bases(*win)
    fin = [g.count_finish() for g in grids]
    assert all(ok for _, ok in fin)
    assert sum(c.nV for c, _ in fin) == ref.nV and sum(c.nT for c, _ in fin) == ref.nT
    _only_the_rows_were_written(V, N, T, ref, (layout, "emit_at_device_bases"))
    for g in grids:
        g.close()


# ---- 6: pitches the kernels cannot address are refused -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["u8", "f32", "f64"])
def test_adopt_refuses_what_32_bit_offsets_cannot_reach(dtype):
    """Argument checks only: no kernel runs, the pointer is never followed."""
    import torch
    from mc33_c_library_amd import DeviceGrid
    from mc33_c_library_amd.api import EINVAL, OK
    size = np.dtype(NP[dtype]).itemsize
    t = torch.zeros((3, 4, 5), dtype={"u8": torch.uint8, "f32": torch.float32, "f64": torch.float64}[dtype], device="cuda")
    g = DeviceGrid(t)
    adopt = lambda pitch, slc: g.lib.mc33hip_adopt_device(g.ctx, C.c_void_p(t.data_ptr()), pitch, slc)
    assert adopt(4, 16) == EINVAL and adopt(5, 19) == EINVAL               # pitch < npx, slice < pitch * npy
    assert adopt(1 << 32, 4 << 32) == EINVAL                               # the pitch does not fit GridView's 32 bits
    last = 0xFFFFFFFF // (64 * size)                                       # 64 rows of a tile in 32-bit byte offsets
    assert adopt(last + 1, (last + 1) * 4) == EINVAL
    assert b"32-bit" in g.lib.mc33hip_last_error()
    assert adopt(last, last * 4) == OK
    assert adopt(t.stride(1), t.stride(0)) == OK
    g.close()
