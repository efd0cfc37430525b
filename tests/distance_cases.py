"""Made-up meshes and query points for the nearest-triangle search (tests/test_distance_cpu.py pins what the GPU tests rely on,
tests/test_gpu_distance.py runs them): where the lattice, the shells and the stopping bound can still go wrong.  Everything is
seeded; numpy only.  A case is (P, V, T): float32 points and vertices, uint32 triangles."""
import itertools

import numpy as np

LADDER_POINTS = (1, 63, 64, 65, 255, 256, 257, 1025)
LADDER_TRIANGLES = (1, 2, 64, 257, 5000)


def soup(nT, seed, size=0.25, lo=0.0, hi=1.0, dtype=np.float32):
    """nT triangles of their own three vertices each: a corner anywhere in the box lo .. hi, the other two within `size` of it"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo, hi, (nT, 1, 3))
    V = (a + np.concatenate([np.zeros((nT, 1, 3)), rng.uniform(-size, size, (nT, 2, 3))], axis=1)).reshape(-1, 3).astype(dtype)
    return V, np.arange(3 * nT, dtype=np.uint32).reshape(nT, 3)


def ladder(nP, nT, dtype=np.float32):
    """random triangles in the unit box, points in a box twice as large about the same centre: the first nP of one seeded set
    per nT, so that one oracle call over the largest nP serves every smaller one"""
    V, T = soup(nT, 1000 + nT, dtype=dtype)
    P = np.random.default_rng(7 + nT).uniform(-0.5, 1.5, (LADDER_POINTS[-1], 3)).astype(dtype)
    return np.ascontiguousarray(P[:nP]), V, T


def sheet(n=16, height=3.0):
    """n x n unit squares cut in two, integer coordinates in the plane z = 0; points above every vertex, every edge midpoint and
    every face centre at z = height: a point above a vertex is equally far from up to six triangles, one above an edge from two"""
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    V = np.stack([ii.ravel(), jj.ravel(), np.zeros(ii.size)], axis=1).astype(np.float32)
    v = lambda i, j: i * (n + 1) + j
    T = []
    for i in range(n):
        for j in range(n):
            T += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
    g = np.arange(2 * n + 1) * 0.5  # vertices, edge midpoints and face centres: every half step
    x, y = np.meshgrid(g, g, indexing="ij")
    P = np.stack([x.ravel(), y.ravel(), np.full(x.size, height)], axis=1).astype(np.float32)
    return P, V, np.array(T, np.uint32)


def two_equidistant():
    """two disjoint triangles mirrored in the plane x = 0 and a row of points in that plane"""
    V = np.array([[2, 0, 0], [4, 0, 0], [2, 3, 1], [-2, 0, 0], [-4, 0, 0], [-2, 3, 1]], np.float32)
    T = np.array([[3, 4, 5], [0, 1, 2]], np.uint32)
    P = np.stack([np.zeros(40), np.arange(40) - 20.0, np.arange(40) % 5 - 2.0], axis=1).astype(np.float32)
    return P, V, T


def doubled(nT=600, seed=5):
    """every triangle present twice, the copies nT indices apart, in a seeded order of the pairs"""
    V, T = soup(nT, seed)
    T2 = np.concatenate([T, T])
    P = np.random.default_rng(seed + 1).uniform(-0.2, 1.2, (700, 3)).astype(np.float32)
    return P, V, np.ascontiguousarray(T2)


DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]


def far_and_edge(nT=400, seed=11):
    """points 1, 10 and 1000 extents of the mesh's box outside it in all 26 directions; points exactly on the box's faces, edges
    and corners; points on planes that cut the box in 2 .. 9, 16 and 32 equal parts - the cell boundaries of lattices of those sizes"""
    V, T = soup(nT, seed)
    lo, hi = V.astype(np.float64).min(axis=0), V.astype(np.float64).max(axis=0)
    mid, ext = 0.5 * (lo + hi), hi - lo
    P = [mid + np.array(d) * ext * (0.5 + k) for k in (1.0, 10.0, 1000.0) for d in DIRECTIONS]
    P += [np.where(np.array(d) < 0, lo, np.where(np.array(d) > 0, hi, mid)) for d in DIRECTIONS]
    rng = np.random.default_rng(seed + 1)
    for n in (2, 3, 4, 5, 6, 7, 8, 9, 16, 32):
        for k in range(n + 1):
            for axis in range(3):
                p = rng.uniform(lo, hi)
                p[axis] = lo[axis] + ext[axis] * k / n
                P.append(p)
    return np.array(P).astype(np.float32), V, T


def far_from_the_origin(nT=300, seed=13):
    """triangles of size 2^-6 in a box of edge 1 translated by 4096: float32 coordinates 2^-11 apart, a relative slack would be
    as large as a triangle"""
    V, T = soup(nT, seed, size=2.0 ** -6)
    V = (V.astype(np.float64) + 4096.0).astype(np.float32)
    P = (np.random.default_rng(seed + 1).uniform(-0.25, 1.25, (500, 3)) + 4096.0).astype(np.float32)
    return P, V, T


def crowded(seed=17):
    """5000 triangles inside a box of edge 2^-7 - one cell of any lattice the 50 others, far apart in a box of edge 64, allow"""
    Va, Ta = soup(5000, seed, size=2.0 ** -9, lo=0.0, hi=2.0 ** -7)
    Vb, Tb = soup(50, seed + 1, size=1.0, lo=-32.0, hi=32.0)
    V, T = np.concatenate([Va, Vb]), np.concatenate([Ta, Tb + Va.shape[0]])
    rng = np.random.default_rng(seed + 2)
    P = np.concatenate([rng.uniform(-0.01, 0.02, (300, 3)), rng.uniform(-40.0, 40.0, (300, 3))]).astype(np.float32)
    return P, V, np.ascontiguousarray(T.astype(np.uint32))


def spanning(seed=19):
    """one triangle across the whole box, in the plane z = 0.5, LAST in T, among 5000 tiny ones; the first 200 points lie within
    0.01 of its middle, where the tiny ones were thinned out: they must find it from a cell in the lattice's interior"""
    V, T = soup(5000, seed, size=0.01)
    c = V.reshape(-1, 3, 3)[:, 0, :]
    keep = ~((np.abs(c[:, 2] - 0.5) < 0.1) & (np.abs(c[:, 0] - 0.5) < 0.2) & (np.abs(c[:, 1] - 0.4) < 0.2))
    V = V.reshape(-1, 3, 3)[keep].reshape(-1, 3)
    T = np.arange(V.shape[0], dtype=np.uint32).reshape(-1, 3)
    big = np.array([[-0.5, -0.5, 0.5], [1.5, -0.5, 0.5], [0.5, 1.5, 0.5]], np.float32)
    V, T = np.concatenate([V, big]), np.concatenate([T, [[V.shape[0], V.shape[0] + 1, V.shape[0] + 2]]]).astype(np.uint32)
    rng = np.random.default_rng(seed + 1)
    near = np.array([0.5, 0.4, 0.5]) + rng.uniform(-0.05, 0.05, (200, 3)) * [1.0, 1.0, 0.2]
    P = np.concatenate([near, rng.uniform(0.0, 1.0, (300, 3))]).astype(np.float32)
    return P, V, T


def hostile(seed=23):
    """collinear and single-point triangles, triangles with a NaN or an infinite corner, one outlier at 1e30 - among 500 sane
    ones; the points: 400 finite ones, then 12 with a NaN or an infinite coordinate.  Returns (P, V, T, bad: the indices of the
    triangles with a corner that is not finite, nonfinite points: how many)"""
    V, T = soup(500, seed)
    rng = np.random.default_rng(seed + 1)
    extra = []
    near = []
    for k in range(40):  # collinear: the third corner on the line through the first two
        a, d = rng.uniform(0, 1, 3), rng.uniform(-0.2, 0.2, 3)
        extra.append([a, a + d, a + d * rng.uniform(-2, 3)])
        near.append(a + 0.5 * d + 1e-3)
    for k in range(40):  # a single point, three times
        a = rng.uniform(0, 1, 3)
        extra.append([a, a, a])
        near.append(a - 1e-3)
    nan, inf = np.nan, np.inf
    for k, x in enumerate((nan, inf, -inf, nan, inf, -inf)):
        t = rng.uniform(0, 1, (3, 3))
        t[k % 3, (k + 1) % 3] = x
        extra.append(t)
    extra.append(np.array([[1e30, 1e30, 1e30], [1e30, 1.0000001e30, 1e30], [1e30, 1e30, 1.0000001e30]]))
    E = np.array(extra).reshape(-1, 3).astype(np.float32)
    n0 = V.shape[0]
    V = np.concatenate([V, E])
    T = np.concatenate([T, np.arange(n0, n0 + E.shape[0], dtype=np.uint32).reshape(-1, 3)])
    order = np.random.default_rng(seed + 2).permutation(T.shape[0])
    T = np.ascontiguousarray(T[order])
    bad = np.nonzero(~np.isfinite(V[T.astype(np.int64)].astype(np.float64)).all(axis=(1, 2)))[0]
    P = np.concatenate([np.array(near), rng.uniform(-0.5, 1.5, (320, 3))])  # (the first 80 next to the degenerate triangles: these do win)
    wild = rng.uniform(0, 1, (12, 3))
    for k, x in enumerate((nan, inf, -inf) * 4):
        wild[k, k % 3] = x
    wild[9] = [nan, inf, -inf]
    return np.concatenate([P, wild]).astype(np.float32), V, T, bad, 12


def all_unusable():
    """a target of which no triangle is usable: two with a NaN corner, one that names a vertex outside V"""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, np.nan], [np.inf, 0, 0]], np.float32)
    T = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.uint32)
    P = np.random.default_rng(3).uniform(0, 1, (70, 3)).astype(np.float32)
    return P, V, T


def pushed(V, N, d, seed=29):
    """the vertices V pushed along +N or -N (seeded, half each) by half a cell: a float32 array and the directions"""
    s = np.where(np.random.default_rng(seed).integers(0, 2, V.shape[0]) == 1, 1.0, -1.0)
    h = 0.5 * float(min(d))
    return (V.astype(np.float64) + (s * h)[:, None] * N.astype(np.float64)).astype(V.dtype), s
