"""The case table of the grid resampling, shared by the host build of the kernel's text (test_resample_cpu.py) and
the device (test_gpu_resample.py): shapes, taps per axis and strides at which the tiling can go wrong - the smallest such shapes,
not the workload's.  The oracle's result of a case is computed once, shared and left unchanged."""
import numpy as np

import resample_oracle as ro

# restated from mc33_c_library_amd/csrc/mc33_resample.hip.h (test_resample_cpu.py checks that they are the header's)
RS_ZCHUNK = 64
RS_TILE_X, RS_TILE_Y = 32, 16

NP_DTYPES = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
TYPE_CODE = {"f32": 0, "f64": 1, "u8": 2, "u16": 3, "u32": 4}
CLAMPING = [-0.5, 2.5, -0.5]   # on a 0 / MAX checkerboard: 3 MAX (clamped to MAX) and -MAX (clamped to 0)


def random_taps(seed, r):
    """asymmetric, with negative lobes"""
    if r is None:
        return None
    rng = np.random.default_rng(1000 + seed)
    return [float(x) for x in rng.uniform(-0.5, 1.0, 2 * r + 1)]


def _t(seed, radii):
    return tuple(random_taps(seed * 3 + a, r) for a, r in enumerate(radii))


G1 = ro.gaussian_taps(1.0)
# name -> ((npx, npy, npz), taps per axis, stride per axis)
CASES = {
    "shorter_than_the_radius": ((2, 3, 2), _t(1, (8, 8, 8)), (1, 1, 1)),
    "one_past_a_tile": ((RS_TILE_X * 2 + 1, RS_TILE_Y + 1, 9), _t(2, (2, 1, 3)), (1, 1, 1)),
    "no_multiple_of_a_tile": ((67, 35, 19), _t(3, (3, 2, 1)), (1, 1, 1)),
    "z_chunk": ((5, 4, RS_ZCHUNK), _t(4, (1, 0, 2)), (1, 1, 1)),
    "z_chunk_minus_1": ((5, 4, RS_ZCHUNK - 1), _t(4, (1, 0, 2)), (1, 1, 1)),
    "z_chunk_plus_1": ((5, 4, RS_ZCHUNK + 1), _t(4, (1, 0, 2)), (1, 1, 1)),
    "two_z_chunks_plus_1": ((5, 4, 2 * RS_ZCHUNK + 1), _t(4, (1, 0, 2)), (1, 1, 1)),
    "two_z_chunks_of_outputs": ((4, 5, 4 * RS_ZCHUNK + 1), _t(5, (0, 1, 3)), (1, 1, 2)),
    "radii_8_0_3": ((67, 35, 19), _t(6, (8, 0, 3)), (1, 1, 1)),
    "radii_0_8_1": ((33, 20, 7), _t(7, (0, 8, 1)), (1, 1, 1)),
    "stride_2_2_2": ((67, 35, 19), (G1, G1, G1), (2, 2, 2)),
    "stride_3_1_2": ((67, 35, 19), _t(8, (2, 3, 1)), (3, 1, 2)),
    "stride_4_4_4_beyond_the_taps": ((67, 35, 19), _t(9, (1, 1, 1)), (4, 4, 4)),
    "eleven_points_stride_3": ((11, 11, 11), _t(10, (1, 2, 0)), (3, 3, 3)),
    "stride_equals_ntaps": ((40, 21, 10), _t(11, (1, 1, 1)), (3, 3, 3)),
    "no_taps_x": ((34, 18, 5), (None,) + _t(12, (0, 2, 1))[1:], (1, 2, 1)),
    "no_taps_x_z": ((34, 18, 5), (None, random_taps(40, 2), None), (2, 1, 1)),
    "no_taps": ((34, 18, 5), (None, None, None), (1, 1, 1)),
    "no_taps_strided": ((34, 18, 5), (None, None, None), (3, 2, 2)),
    # long taps at large strides stage so much that the tile shrinks (rs_plan_tiles): the tiles below 32 x 8, TILES below
    "tile_32x4": ((140, 24, 4), _t(13, (8, 8, 1)), (4, 4, 1)),
    "tile_32x2": ((240, 24, 3), _t(14, (8, 8, 0)), (7, 7, 1)),
    "tile_32x1": ((300, 30, 5), _t(15, (8, 8, 0)), (9, 9, 2)),
    "tile_16x1": ((300, 40, 3), _t(16, (8, 8, 0)), (17, 17, 1)),
}
# the tile of outputs rs_plan_tiles chooses, where the case's name promises one (test_resample_cpu.py checks it against the program)
TILES = {"one_past_a_tile": (32, 16), "shorter_than_the_radius": (32, 8), "tile_32x4": (32, 4), "tile_32x2": (32, 2), "tile_32x1": (32, 1), "tile_16x1": (16, 1)}
ALL_TYPE_CASES = {   # all five sample types: integers hit both clamps, f32 / f64 carry inf and NaN
    "types_one_past_a_tile": ((RS_TILE_X * 2 + 1, RS_TILE_Y + 1, 9), (CLAMPING, CLAMPING, CLAMPING), (1, 1, 1)),
    "types_stride_3_1_2": ((67, 35, 19), (CLAMPING, random_taps(50, 1), CLAMPING), (3, 1, 2)),
}


def field(dtype, shape_xyz, seed=0):
    """samples [z][y][x]: floats normal with a few +-inf, NaN and -0.0; integers a 0 / MAX checkerboard with random cells"""
    npx, npy, npz = shape_xyz
    rng = np.random.default_rng(77 + seed)
    dt = np.dtype(NP_DTYPES[dtype])
    if dt.kind == "f":
        F = rng.standard_normal((npz, npy, npx)).astype(dt)
        flat = F.reshape(-1)
        idx = rng.choice(flat.size, size=min(8, flat.size // 3), replace=False)
        flat[idx] = np.resize(np.array([np.inf, -np.inf, np.nan, -0.0], dt), idx.size)
        return F
    top = int(np.iinfo(dt).max)
    z, y, x = np.indices((npz, npy, npx))
    F = (((x + y + z) & 1) * top).astype(dt)
    some = rng.random((npz, npy, npx)) < 0.2
    F[some] = rng.integers(0, top, size=int(some.sum()), endpoint=True).astype(dt)
    return F


def finite_field(dtype, shape_xyz, seed=0):
    F = field(dtype, shape_xyz, seed)
    if F.dtype.kind == "f":
        F[~np.isfinite(F)] = 1.5
    return F


_results = {}


def case(name, dtype="f32"):
    """(F, taps, stride, the oracle's grid) of a case, computed once and left unchanged"""
    key = (name, dtype)
    if key not in _results:
        shape, taps, stride = (CASES.get(name) or ALL_TYPE_CASES[name])
        F = field(dtype, shape, seed=sum(name.encode())) if name in ALL_TYPE_CASES else finite_field(dtype, shape, seed=sum(name.encode()))
        want = ro.resample(F, taps, stride)
        F.setflags(write=False)
        want.setflags(write=False)
        _results[key] = (F, taps, stride, want)
    return _results[key]
