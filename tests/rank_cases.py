"""The case table of the rank filter, shared by the host build of the kernels' text (test_rank_cpu.py) and the
device (test_gpu_rank.py): shapes, ranks and radii at which a tiled, z-marching kernel can go wrong - the smallest such shapes,
not the workload's.  The oracle's result of a case is computed once, shared and left unchanged."""
import numpy as np

import rank_oracle as ko

# restated from mc33_c_library_amd/csrc/mc33_rank.hip.h (test_rank_cpu.py checks that they are the header's)
RK_ZCHUNK = 64
RK_TILE_X, RK_TILE_Y = 64, 16

NP_DTYPES = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
TYPE_CODE = {"f32": 0, "f64": 1, "u8": 2, "u16": 3, "u32": 4}
MIN, MEDIAN, MAX = ko.MIN, ko.MEDIAN, ko.MAX
MEDIAN_SHAPES = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]

# name -> ((npx, npy, npz), rank, radius per axis)
CASES = {
    "shorter_than_the_radius_min": ((2, 3, 2), MIN, (8, 8, 8)),
    "shorter_than_the_radius_median": ((2, 3, 2), MEDIAN, (1, 1, 1)),
    "one_past_a_tile_median": ((RK_TILE_X * 2 + 1, RK_TILE_Y + 1, 5), MEDIAN, (1, 1, 1)),
    "one_past_a_tile_max": ((RK_TILE_X * 2 + 1, RK_TILE_Y + 1, 5), MAX, (2, 1, 1)),
    "no_multiple_of_a_tile_median": ((67, 35, 19), MEDIAN, (1, 1, 1)),
    "no_multiple_of_a_tile_min": ((67, 35, 19), MIN, (1, 1, 1)),
}
for _name, _nz in (("z_chunk", RK_ZCHUNK), ("z_chunk_minus_1", RK_ZCHUNK - 1), ("z_chunk_plus_1", RK_ZCHUNK + 1), ("two_z_chunks_plus_1", 2 * RK_ZCHUNK + 1)):
    CASES[_name + "_median"] = ((5, 4, _nz), MEDIAN, (1, 1, 1))
    CASES[_name + "_max"] = ((5, 4, _nz), MAX, (1, 0, 2))
for _r in MEDIAN_SHAPES:
    CASES["median_%d%d%d" % _r] = ((37, 19, 7), MEDIAN, _r)
for _rank, _word in ((MIN, "min"), (MAX, "max")):
    CASES[_word + "_8_0_3"] = ((67, 35, 19), _rank, (8, 0, 3))
    CASES[_word + "_0_8_1"] = ((33, 20, 7), _rank, (0, 8, 1))
    CASES[_word + "_2_2_2"] = ((67, 35, 19), _rank, (2, 2, 2))
CASES["min_0_0_0"] = ((37, 19, 7), MIN, (0, 0, 0))
# the tile of outputs rk_plan_tiles chooses, where a case is there for it (test_rank_cpu.py checks it against the program):
# radius 8 along x, y and z does not fit the LDS budget at 64 x 16
TILES = {"one_past_a_tile_median": (64, 16), "one_past_a_tile_max": (64, 16), "shorter_than_the_radius_min": (64, 8), "max_8_0_3": (64, 16)}
ALL_TYPE_CASES = {   # all five sample types, on two shapes
    "types_median_one_past_a_tile": ((RK_TILE_X * 2 + 1, RK_TILE_Y + 1, 5), MEDIAN, (1, 1, 1)),
    "types_max_67": ((67, 35, 19), MAX, (2, 1, 1)),
    "types_min_67": ((67, 35, 19), MIN, (1, 2, 1)),
}

# bit patterns: numpy arithmetic may normalise a NaN, a view of integers does not
SPECIAL_BITS = {
    np.dtype(np.float32): np.array([0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7FC00001, 0xFFC00123, 0x7F800ABC, 0xFFFFFFFF], np.uint32),
    np.dtype(np.float64): np.array([0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0, 0x7FF8000000000001, 0xFFF8000000000123,
                                    0x7FF0000000000ABC, 0xFFFFFFFFFFFFFFFF], np.uint64),
}   # +inf, -inf, -0, +0, NaN without and with the sign bit, with payloads (a signalling one and all ones among them)


def field(dtype, shape_xyz, seed=0):
    """samples [z][y][x].  Floats: normal, one sample in eight one of SPECIAL_BITS, and -0 next to +0 in the first row; integers:
    random with one sample in eight 0 or MAX."""
    npx, npy, npz = shape_xyz
    rng = np.random.default_rng(177 + seed)
    dt = np.dtype(NP_DTYPES[dtype])
    n = npx * npy * npz
    some = rng.random(n) < 0.125
    if dt.kind == "f":
        F = rng.standard_normal(n).astype(dt)
        bits = F.view(SPECIAL_BITS[dt].dtype)
        bits[some] = rng.choice(SPECIAL_BITS[dt], size=int(some.sum()))
        bits[0], bits[1] = SPECIAL_BITS[dt][2], SPECIAL_BITS[dt][3]
        return F.reshape(npz, npy, npx)
    top = int(np.iinfo(dt).max)
    F = rng.integers(0, top, size=n, endpoint=True).astype(dt)
    F[some] = rng.choice(np.array([0, top], dt), size=int(some.sum()))
    F[0], F[1] = 0, top
    return F.reshape(npz, npy, npx)


def poison(dtype, rank):
    """the sample a padding holds: the one that would win the rank if it were read (for the median: the largest key)"""
    dt = np.dtype(NP_DTYPES[dtype])
    if dt.kind == "f":
        ut = SPECIAL_BITS[dt].dtype
        quiet = 0x7FC00000 if dt.itemsize == 4 else 0x7FF8000000000000
        sign = 1 << (8 * dt.itemsize - 1)
        return np.array([quiet | 0x55 | (sign if rank == MIN else 0)], ut).view(dt)[0]
    return dt.type(0 if rank == MIN else np.iinfo(dt).max)


def place(F, lay, fill):
    """a flat array full of `fill` with the grid F[z][y][x] in it at lay = (pitch, slice, off), cut behind the last grid point"""
    pitch, slc, off = lay
    npz, npy, npx = F.shape
    assert pitch >= npx and slc >= pitch * npy and off >= 0
    flat = np.full(off + (npz - 1) * slc + (npy - 1) * pitch + npx, fill, F.dtype)
    it = F.dtype.itemsize
    np.lib.stride_tricks.as_strided(flat[off:], F.shape, (slc * it, pitch * it, it))[...] = F
    return flat


_results = {}


def case(name, dtype="f32"):
    """(F, rank, radius, the oracle's grid) of a case, computed once and left unchanged"""
    key = (name, dtype)
    if key not in _results:
        shape, rank, radius = (CASES.get(name) or ALL_TYPE_CASES[name])
        F = field(dtype, shape, seed=sum(name.encode()))
        want = ko.rank_filter(F, rank, radius)
        F.setflags(write=False)
        want.setflags(write=False)
        _results[key] = (F, rank, radius, want)
    return _results[key]
