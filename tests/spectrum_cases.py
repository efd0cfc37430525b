"""The case table of the contour spectrum, shared by the host build of the kernel's text (test_spectrum_cpu.py) and
the device (test_gpu_spectrum.py): the smallest shapes at which the tiling, the packed loads and the counters can go wrong, not the
workload's.  The oracle's result of a case is computed once, shared and left unchanged."""
import ctypes as C

import numpy as np

import fixtures as fx
import spectrum_oracle as so
from mc33_c_library_amd.api import SpectrumInfo

# restated from mc33_c_library_amd/csrc/mc33_spectrum.hip.h (test_spectrum_cpu.py checks that they are the header's)
SP_TILE_X, SP_TILE_Y = 64, 16   # cells
SP_ZCHUNK = 32                  # cell slices
SP_THREADS = 256

NP_DTYPES = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
TYPE_CODE = {"f32": 0, "f64": 1, "u8": 2, "u16": 3, "u32": 4}
TYPES = ["f32", "u16", "u8", "u32", "f64"]

# name -> (npx, npy, npz) in POINTS.  A tile of cells plus one is a tile of points.
SHAPES = {
    "one_cell": (2, 2, 2),
    "small": (3, 4, 5),
    "one_tile": (SP_TILE_X + 1, SP_TILE_Y + 1, SP_ZCHUNK + 1),
    "one_point_beyond": (SP_TILE_X + 2, SP_TILE_Y + 2, SP_ZCHUNK + 2),
    "tile_minus_1_beyond": (2 * SP_TILE_X, 2 * SP_TILE_Y, 2 * SP_ZCHUNK),
    "dword_plus_1": (SP_TILE_X + 5, 5, 3),    # widths that end 1, 2 and 3 samples past a dword of 1-byte samples, in a second tile
    "dword_plus_2": (SP_TILE_X + 6, 5, 3),
    "dword_plus_3": (SP_TILE_X + 7, 3, 4),
    "narrow_dword_plus_1": (5, 18, 3),        # ... and in the first
    "narrow_dword_plus_3": (7, 3, 34),
}
FIELDS = ("cos", "noise", "plateau", "constant", "special")   # special: float types only

# (shape, field, number of isovalues): every shape with a smooth and an adverse field, every field, n of 0, 1 and 255
CASES = {}
for _s in SHAPES:
    CASES["%s_cos" % _s] = (_s, "cos", 7)
    CASES["%s_noise" % _s] = (_s, "noise", 12)
CASES.update({
    "plateau_isovalues_equal_samples": ("one_point_beyond", "plateau", 5),
    "constant": ("small", "constant", 3),
    "constant_two_tiles": ("one_point_beyond", "constant", 2),
    "special_values": ("one_point_beyond", "special", 9),
    "special_values_small": ("small", "special", 5),
    "infinite_isovalues": ("small", "special_inf", 5),
    "n_0": ("one_point_beyond", "noise", 0),
    "n_1": ("one_point_beyond", "cos", 1),
    "n_255_noise": ("one_point_beyond", "noise", 255),
    "n_255_cos": ("one_tile", "cos", 255),
    "n_200_noise": ("small", "noise", 200),   # (not a power of two minus one: the search meets the padding)
})
FLOAT_ONLY = ("special_values", "special_values_small", "infinite_isovalues")
# the cases of the layout tests: two tiles and a row tail on every axis, both counters busy
LAYOUT_CASE = "dword_plus_3_noise"
LAYOUT_CASE_2 = "narrow_dword_plus_1_cos"


def _span(dt):
    """(mid, amplitude per unit) that spread the cos field, -3 .. 3, over an integer type"""
    return {1: (128.0, 40.0), 2: (32768.0, 10000.0), 4: (2147483648.0, 5.0e8)}[dt.itemsize]


def field(kind, dtype, shape_xyz, seed=0):
    """samples [z][y][x]"""
    npx, npy, npz = shape_xyz
    dt = np.dtype(NP_DTYPES[dtype])
    rng = np.random.default_rng(4242 + seed)
    ax = [np.cos(fx.axis_accum(-4.0, 8.0 / max(n - 1, 1), n)) for n in (npx, npy, npz)]
    cos = (ax[0][None, None, :] + ax[1][None, :, None]) + ax[2][:, None, None]
    if kind == "cos":
        if dt.kind == "f":
            return cos.astype(dt)
        mid, amp = _span(dt)
        return np.rint(mid + amp * cos).astype(dt)
    if kind == "noise":
        if dt.kind == "f":
            return rng.uniform(-1.0, 1.0, (npz, npy, npx)).astype(dt)
        return rng.integers(0, np.iinfo(dt).max, size=(npz, npy, npx), endpoint=True).astype(dt)
    if kind == "plateau":   # integer levels 0 .. 6 in every type
        return np.floor(cos + 3.0).clip(0, 6).astype(dt)
    if kind == "constant":
        return np.full((npz, npy, npx), 7, dt)
    if kind in ("special", "special_inf"):
        assert dt.kind == "f"
        F = rng.uniform(-1.0, 1.0, (npz, npy, npx)).astype(dt)
        flat = F.reshape(-1)
        idx = rng.choice(flat.size, size=max(6, flat.size // 5), replace=False)
        neg_nan = np.copysign(dt.type(np.nan), dt.type(-1.0))
        pos_nan = np.copysign(dt.type(np.nan), dt.type(1.0))
        flat[idx] = np.resize(np.array([pos_nan, neg_nan, np.inf, -np.inf, 0.0, -0.0], dt), idx.size)
        return F
    raise KeyError(kind)


def isovalues(kind, dtype, n):
    """n doubles, strictly ascending as MC33_real of the type"""
    dt = np.dtype(NP_DTYPES[dtype])
    if n == 0:
        return []
    if kind == "plateau":
        return [float(k) for k in range(1, n + 1)]           # equal to sample values
    if kind == "constant":
        return [float(k) for k in range(7 - n // 2, 7 - n // 2 + n)]   # 7 among them
    if kind == "special_inf":
        assert n == 5
        return [float("-inf"), -0.5, 0.0, 0.5, float("inf")]
    if kind == "special":   # an odd ladder over -0.9 .. 0.9 has 0.0 in the middle (never -0.0: DESIGN.md 8)
        v = [float(x) for x in so.ladder(-0.9, 0.9, n, dt).astype(np.float64)]
        assert n & 1 and v[n // 2] == 0.0
        return v
    if dt.kind == "f":
        lo, hi = (-3.0, 3.0) if kind == "cos" else (-1.0, 1.0)
    elif kind == "cos":
        mid, amp = _span(dt)
        lo, hi = mid - 3.0 * amp, mid + 3.0 * amp
    else:
        lo, hi = 0.0, float(np.iinfo(dt).max)
    if dt.itemsize == 1 and n == 255:
        return [k + 0.5 for k in range(255)]
    return [float(x) for x in so.ladder(lo, hi, n, dt).astype(np.float64)]


_results = {}


def case(name, dtype="f32"):
    """(F, isovalues as a list of doubles, the oracle's Spectrum of the whole grid) of a case, computed once and left unchanged"""
    key = (name, dtype)
    if key not in _results:
        shape, kind, n = CASES[name]
        F = field(kind, dtype, SHAPES[shape], seed=sum(name.encode()))
        isos = isovalues(kind, dtype, n)
        assert so.convert_isovalues(isos, F.dtype) is not None and len(isos) == n, (name, dtype)
        want = so.spectrum(F, isos)
        F.setflags(write=False)
        _results[key] = (F, isos, want)
    return _results[key]


def cases_of(dtype):
    return [n for n in CASES if NP_DTYPES[dtype]().dtype.kind == "f" or n not in FLOAT_ONLY]


def split(nz, parts):
    """`parts` disjoint ranges that tile cell slices [0, nz): as even as they come, one-slice ranges where parts >= nz / 2"""
    edges = sorted(set(int(round(k * nz / parts)) for k in range(parts + 1)))
    return [(a, b) for a, b in zip(edges[:-1], edges[1:])]


def report(got, want):
    return "cut_cells %s\n     want %s\nhistogram %s\n     want %s\n%s\n%s" % (got.cut_cells.tolist(), want.cut_cells.tolist(), got.histogram.tolist(), want.histogram.tolist(), got[2:], want[2:])


def c_spectrum(lib, L, M, isos):
    """MC33_grid_spectrum of an MC33Lib's object as the oracle's tuple, or its return code when it refuses"""
    n = len(isos)
    arr = (lib.real * max(n, 1))(*isos)
    cut = (C.c_ulonglong * max(n, 1))()
    hist = (C.c_ulonglong * (n + 1))()
    info = SpectrumInfo()
    rc = L.MC33_grid_spectrum(M, arr, n, cut, hist, C.byref(info))
    if rc:
        return rc
    return so.Spectrum(np.array(cut[:n], np.uint64), np.array(hist[:], np.uint64), info.points, info.cells, info.nan_samples, info.sample_min, info.sample_max)
