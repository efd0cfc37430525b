"""The definition of mc33hip_rank_grid (include/mc33_hip.h) in numpy: the oracle the device kernels, their host
build and the C API are held to bit for bit.

Every sample becomes its key - an unsigned integer whose order is the only one the filter uses -, the grid of keys is padded by
the radii with its edge samples (np.pad, mode="edge"), every output point's window is a sliding-window view of the padded grid,
the window's keys are sorted as integers and the key of rank k is turned back into the sample's bytes."""
import numpy as np

MIN, MEDIAN, MAX = 0, 1, 2
RANKS = {"min": MIN, "median": MEDIAN, "max": MAX}
LIMIT = {MIN: 8, MEDIAN: 1, MAX: 8}   # the largest radius per axis

_BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def keys(F):
    """the keys of samples F, as unsigned integers of the samples' width"""
    F = np.ascontiguousarray(F)
    if F.dtype.kind == "u":
        return F.copy()
    ut = _BITS[F.dtype]
    b = F.view(ut)
    top = ut(1) << ut(8 * F.dtype.itemsize - 1)
    return np.where(b & top != 0, ~b, b | top)


def samples(K, dtype):
    """the samples whose keys are K"""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return K.astype(dtype)
    ut = _BITS[dtype]
    top = ut(1) << ut(8 * dtype.itemsize - 1)
    return np.ascontiguousarray(np.where(K & top != 0, K & ~top, ~K)).view(dtype)


def rank_of(rank, n):
    return {MIN: 0, MEDIAN: (n - 1) // 2, MAX: n - 1}[rank]


def accepts(rank, radius):
    return rank in LIMIT and len(radius) == 3 and all(0 <= int(r) <= LIMIT[rank] for r in radius)


def rank_filter(F, rank, radius):
    """F[z][y][x] of one of the five sample types -> the filtered grid of the same type and size; radius per axis x, y, z."""
    F = np.asarray(F)
    rank = RANKS.get(rank, rank)
    assert F.ndim == 3 and F.dtype in (np.float32, np.float64, np.uint8, np.uint16, np.uint32) and accepts(rank, radius)
    r0, r1, r2 = (int(r) for r in radius)
    P = np.pad(keys(F), ((r2, r2), (r1, r1), (r0, r0)), mode="edge")
    W = np.lib.stride_tricks.sliding_window_view(P, (2 * r2 + 1, 2 * r1 + 1, 2 * r0 + 1)).reshape(F.shape + (-1,))
    n = W.shape[-1]
    assert n == (2 * r0 + 1) * (2 * r1 + 1) * (2 * r2 + 1) and n % 2 == 1
    K = np.sort(W, axis=-1)[..., rank_of(rank, n)]
    return np.ascontiguousarray(samples(K, F.dtype))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
