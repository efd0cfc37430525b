"""The contour spectrum of a grid (include/mc33_hip.h: mc33hip_grid_spectrum) restated in numpy: the oracle of
test_spectrum_cpu.py and test_gpu_spectrum.py.  Everything is an integer and every comparison is exact.

    r          = (MC33_real)F                 MC33_real: float, double for double grids
    rank(r)    = #{ j : iso_j < r }           a NaN: n when its sign bit is set, else 0
    cut_cells[k]  cells with min_rank <= k < max_rank over their eight corners
    histogram[j]  grid points with rank j over planes [z_begin, z_end), and plane z_end when the range ends where the grid does
"""
from collections import namedtuple

import numpy as np

Spectrum = namedtuple("Spectrum", "cut_cells histogram points cells nan_samples sample_min sample_max")
MAX_ISOS = 255


def real_type(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


def convert_isovalues(isos, dtype):
    """the isovalues as MC33_real, or None where mc33hip_grid_spectrum answers MC33HIP_EINVAL"""
    with np.errstate(over="ignore"):
        v = np.asarray(isos, np.float64).reshape(-1).astype(real_type(dtype))
    if v.size > MAX_ISOS or np.isnan(v).any() or (v.size > 1 and not (v[:-1] < v[1:]).all()):
        return None
    return v


def ranks(F, isos):
    """rank of every sample as uint16; isos: what convert_isovalues returned"""
    r = np.asarray(F).astype(isos.dtype)
    rk = np.searchsorted(isos, r, side="left")   # the number of isovalues below r
    nan = np.isnan(r)
    rk[nan] = np.where(np.signbit(r[nan]), isos.size, 0)
    return rk.astype(np.uint16)


def spectrum(F, isos, z_begin=0, z_end=None):
    """F[z][y][x]: the WHOLE grid; cell slices [z_begin, z_end)"""
    F = np.asarray(F)
    nz_total = F.shape[0] - 1
    z_end = nz_total if z_end is None else z_end
    assert 0 <= z_begin < z_end <= nz_total
    v = convert_isovalues(isos, F.dtype)
    assert v is not None
    n = v.size
    rk = ranks(F[z_begin:z_end + 1], v)
    mn = rk[:-1, :-1, :-1].copy()
    mx = mn.copy()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c = rk[dz:rk.shape[0] - 1 + dz, dy:rk.shape[1] - 1 + dy, dx:rk.shape[2] - 1 + dx]
                np.minimum(mn, c, out=mn)
                np.maximum(mx, c, out=mx)
    diff = np.bincount(mn.reshape(-1), minlength=n + 1).astype(np.int64) - np.bincount(mx.reshape(-1), minlength=n + 1).astype(np.int64)
    cut = np.cumsum(diff)[:n].astype(np.uint64)
    planes = z_end - z_begin + (1 if z_end == nz_total else 0)
    hist = np.bincount(rk[:planes].reshape(-1), minlength=n + 1).astype(np.uint64)
    r = F[z_begin:z_begin + planes].astype(v.dtype).reshape(-1)
    ok = r[~np.isnan(r)]
    lo = float(ok.min()) if ok.size else float("inf")
    hi = float(ok.max()) if ok.size else float("-inf")
    return Spectrum(cut, hist, int(r.size), int(mn.size), int(r.size - ok.size), lo, hi)


def brute_cut_cells(F, iso):
    """cells cut at ONE isovalue by the corner test of the extraction: the side of a corner is the sign bit of iso - r, a NaN
    sample's own sign (mc33_cell.h: iso_diff); a cell is cut when its eight corners are not all on one side"""
    F = np.asarray(F)
    rt = real_type(F.dtype)
    r = F.astype(rt)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isnan(r), r, rt(iso) - r)
    side = np.signbit(d)
    n = 0
    nz, ny, nx = (s - 1 for s in F.shape)
    for z in range(nz):
        for y in range(ny):
            for x in range(nx):
                c = side[z:z + 2, y:y + 2, x:x + 2]
                n += int(c.any() and not c.all())
    return n


def ladder(lo, hi, n, dtype):
    """MC33_isovalue_ladder: n steps strictly between lo and hi as MC33_real, or None where it returns -1"""
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi) or n > MAX_ISOS:
        return None
    k = np.arange(n, dtype=np.float64)
    v = (lo + (hi - lo) * ((k + 1.0) / float(n + 1))).astype(real_type(dtype))
    if n > 1 and not (v[:-1] < v[1:]).all():
        return None
    return v


def same(a, b):
    """two Spectrum results: integers equal, extremes equal as numbers (which zero is unspecified)"""
    return (np.array_equal(np.asarray(a.cut_cells, np.uint64), np.asarray(b.cut_cells, np.uint64)) and
            np.array_equal(np.asarray(a.histogram, np.uint64), np.asarray(b.histogram, np.uint64)) and
            (int(a.points), int(a.cells), int(a.nan_samples)) == (int(b.points), int(b.cells), int(b.nan_samples)) and
            float(a.sample_min) == float(b.sample_min) and float(a.sample_max) == float(b.sample_max))


def add(parts):
    """the results of disjoint ranges that tile a grid, combined as the host layer combines its slabs"""
    parts = list(parts)
    return Spectrum(sum(np.asarray(p.cut_cells, np.uint64) for p in parts), sum(np.asarray(p.histogram, np.uint64) for p in parts),
                    sum(int(p.points) for p in parts), sum(int(p.cells) for p in parts), sum(int(p.nan_samples) for p in parts),
                    min(float(p.sample_min) for p in parts), max(float(p.sample_max) for p in parts))
