"""The definition of mc33hip_resample_grid (include/mc33_hip.h) in vectorised numpy: the oracle the device kernel,
its host build and the C API are held to bit for bit.

Per axis a correlation with an odd number of taps (at most 17), the edge samples replicated, then every stride-th point: three
passes over float64 arrays, x, then y, then z.  Every sum starts from its first product and adds the others in ascending tap
index - `acc = acc + w * shifted`, two numpy operations, which numpy does not fuse.  gaussian_taps restates MC33_gaussian_taps
with math.exp (the C library's exp)."""
import math

import numpy as np

MAX_RADIUS = 8
IDENTITY = (None, None, None)


def gaussian_taps(sigma, radius=0):
    """The taps as a list of Python floats, or None where MC33_gaussian_taps returns -1."""
    sigma = float(sigma)
    if not (sigma >= 0.0) or math.isinf(sigma):
        return None
    if sigma == 0.0:
        return [1.0]
    r = int(radius) if radius else max(1, int(math.ceil(3.0 * sigma)))
    if r > MAX_RADIUS:
        return None
    e = [math.exp(-float(i * i) / (2.0 * sigma * sigma)) for i in range(r + 1)]
    S = e[0]
    for i in range(1, r + 1):
        S = S + (e[i] + e[i])
    taps = [0.0] * (2 * r + 1)
    for i in range(r + 1):
        taps[r - i] = taps[r + i] = e[i] / S
    return taps


def out_points(n, stride):
    return (int(n) - 1) // int(stride) + 1


def _axis(A, taps, stride, axis):
    """one pass: sum_i taps[i] * A[cl(O * stride + i - r)] along `axis`, a float64 array"""
    w = [1.0] if taps is None else [float(x) for x in taps]
    assert len(w) % 2 == 1 and (len(w) - 1) // 2 <= MAX_RADIUS and all(math.isfinite(x) for x in w) and stride >= 1
    r = (len(w) - 1) // 2
    n = A.shape[axis]
    base = np.arange(out_points(n, stride), dtype=np.int64) * stride
    acc = None
    for i, wi in enumerate(w):
        shifted = np.take(A, np.clip(base + (i - r), 0, n - 1), axis=axis)
        term = np.float64(wi) * shifted
        acc = term if acc is None else acc + term
    return acc


def convert(v, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return v
    if dtype == np.float32:
        with np.errstate(over="ignore", invalid="ignore"):
            return v.astype(np.float32)
    top = float(np.iinfo(dtype).max)
    out = np.zeros(v.shape, dtype)
    hi = v >= top
    mid = (v > 0.0) & ~hi   # (a NaN is in neither)
    out[hi] = np.iinfo(dtype).max
    out[mid] = np.floor(v[mid] + 0.5).astype(dtype)
    return out


def resample(F, taps=IDENTITY, stride=(1, 1, 1)):
    """F[z][y][x] of one of the five sample types -> the resampled grid of the same type; taps and stride per axis x, y, z."""
    F = np.asarray(F)
    assert F.ndim == 3 and F.dtype in (np.float32, np.float64, np.uint8, np.uint16, np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        A = F.astype(np.float64)
        A = _axis(A, taps[0], int(stride[0]), 2)
        A = _axis(A, taps[1], int(stride[1]), 1)
        A = _axis(A, taps[2], int(stride[2]), 0)
    assert min(A.shape) >= 2, "an output axis below 2 points"
    return np.ascontiguousarray(convert(A, F.dtype))


def geometry(r0, d, stride):
    """(r0_out, d_out)"""
    return tuple(float(x) for x in r0), tuple(float(d[k]) * float(int(stride[k])) for k in range(3))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
