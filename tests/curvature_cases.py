"""Grids, fields and made-up vertices shared by tests/test_curvature_cpu.py and tests/test_gpu_curvature.py.  numpy only; the
expected values always come from tests/curvature_oracle.py."""
import numpy as np

import layouts

AWKWARD_R0, AWKWARD_D = (-1.3, 0.7, 2.9), (0.1, 0.07, 0.13)   # (of the property tests)
# powers of two: a float vertex on a grid plane inverts to the plane's integer exactly, so a vertex on a grid edge has two f == 0 and
# two nodes.  (With the awkward geometry it lands a hair beside the plane and has four or eight.)
EXACT_R0, EXACT_D = (-2.0, 0.5, 3.0), (0.25, 0.5, 0.125)
NP_DTYPES = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
TYPE_CODE = {"f32": 0, "f64": 1, "u8": 2, "u16": 3, "u32": 4}
# points per axis as (npz, npy, npx): the smallest grid the pass takes, one with three different sizes, one with cells that
# touch no face
SHAPES = {"3x3x3": (3, 3, 3), "5x4x3": (3, 4, 5), "9x8x7": (7, 8, 9)}


def real_of(dtype):
    return np.float64 if dtype == "f64" else np.float32


def field(dtype, shape, seed=0):
    """a smooth bump plus noise - every second difference is busy; integers over most of their range"""
    rng = np.random.default_rng(1000 + seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    f = np.cos(0.7 * x + 0.2) + np.cos(0.9 * y - 0.4) * np.cos(0.5 * z) + 0.05 * x * y + 0.25 * rng.standard_normal(shape)
    t = NP_DTYPES[dtype]
    if np.dtype(t).kind == "f":
        return f.astype(t)
    top = float(np.iinfo(t).max)
    return np.clip(np.rint((f + 3.0) / 6.0 * top), 0, top).astype(t)


def made_up_vertices(shape, r0, d, real, seed=0):
    """every node; the midpoint and a 1/3 point of every grid edge; cell centres; points outside every face (edges and corners of
    the box included); a NaN row in each coordinate - as rows of `real`, shuffled, so that the lanes of a wave hold vertices with
    1, 2, 4 and 8 nodes side by side"""
    npz, npy, npx = shape
    n = (npx, npy, npz)
    pts = []
    gx, gy, gz = np.meshgrid(np.arange(npx), np.arange(npy), np.arange(npz), indexing="ij")
    nodes = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(np.float64)
    pts.append(nodes)
    for a in range(3):
        on = nodes[nodes[:, a] < n[a] - 1]
        for t in (0.5, 1.0 / 3.0):
            e = on.copy()
            e[:, a] += t
            pts.append(e)
    cells = nodes[(nodes[:, 0] < npx - 1) & (nodes[:, 1] < npy - 1) & (nodes[:, 2] < npz - 1)]
    pts.append(cells + np.array([0.5, 0.5, 0.5]))
    pts.append(cells + np.array([0.25, 0.625, 0.875]))
    out = []
    for sx in (-1.5, 0.4, npx + 0.5):
        for sy in (-0.75, 1.3, npy + 2.0):
            for sz in (-3.0, 0.6, npz - 0.5):
                out.append((sx, sy, sz))
    pts.append(np.array(out))
    g = np.concatenate(pts)
    v = np.asarray(r0, np.float64) + g * np.asarray(d, np.float64)
    nan = np.array([[np.nan, v[1, 1], v[1, 2]], [v[2, 0], np.nan, v[2, 2]], [v[3, 0], v[3, 1], np.nan], [np.nan] * 3])
    v = np.concatenate([v, nan])
    np.random.default_rng(2000 + seed).shuffle(v)
    return np.ascontiguousarray(v.astype(real))


def divergent_vertices(shape, r0, d, real):
    """64 vertices that alternate between x-, y- and z-edges and cell interiors: one wave, every lane another walk"""
    npz, npy, npx = shape
    rng = np.random.default_rng(7)
    rows = []
    for k in range(64):
        i = np.array([rng.integers(0, npx - 1), rng.integers(0, npy - 1), rng.integers(0, npz - 1)], np.float64)
        t = rng.uniform(0.1, 0.9, 3)
        kind = k % 4
        g = i + (t if kind == 3 else np.where(np.arange(3) == kind, t, 0.0))
        rows.append(g)
    return np.ascontiguousarray((np.asarray(r0, np.float64) + np.array(rows) * np.asarray(d, np.float64)).astype(real))


def padded(F, name="all"):
    """(flat, (pitch, slice, off)): F in the named layout of tests/layouts.py inside a flat array whose every other sample is
    poison - NaN for floats, all bits set for integers - so that a read outside a row's npx points shows in the output"""
    lay = layouts.layout(name, F.shape, F.dtype.itemsize)
    pitch, slc, off = lay
    n = layouts.flat_size(F.shape, lay)
    flat = np.full(n, np.nan if F.dtype.kind == "f" else np.iinfo(F.dtype).max, F.dtype)
    it = F.dtype.itemsize
    np.lib.stride_tricks.as_strided(flat[off:], F.shape, (slc * it, pitch * it, it))[...] = F
    return flat, lay


def sphere_case(cells, radius, centre):
    """F = -|x - centre| on cells^3 cells of unit spacing, cast to float32; the isovalue -radius; the vertices of the cut grid
    edges by linear interpolation between the float32 samples, as float32 rows"""
    n = cells + 1
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
    F = (-np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)
    return F, edge_vertices(F, -float(radius))


def edge_vertices(F, iso):
    """the points where the grid edges of F (unit spacing, origin 0) cross iso, by linear interpolation in double"""
    G = F.astype(np.float64) - iso
    idx = np.stack(np.meshgrid(*(np.arange(s) for s in F.shape), indexing="ij"), axis=-1)   # [..., (z, y, x)]
    rows = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        a, b = G[tuple(lo)], G[tuple(hi)]
        cut = (a < 0) != (b < 0)
        t = a[cut] / (a[cut] - b[cut])
        p = idx[tuple(lo)][cut].astype(np.float64)
        p[:, axis] += t
        rows.append(p[:, ::-1])   # (x, y, z)
    return np.ascontiguousarray(np.concatenate(rows).astype(np.float32))
