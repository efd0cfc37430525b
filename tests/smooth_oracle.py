"""Taubin's lambda | mu smoothing and the recomputed vertex normals of include/mc33_hip.h (mc33hip_smooth_surface,
mc33hip_vertex_normals) restated in numpy float64, operation by operation - nothing fused, every sequential sum
made by a loop over the neighbour rank k with masked vector additions - so that each row is the very bits the device forms.
numpy only."""
import numpy as np


def valid_triangles(T, nV):
    T = np.asarray(T).astype(np.int64).reshape(-1, 3)
    return T[(T < nV).all(axis=1)]


class Adjacency:
    """start [nV + 1], nbr (the rows nb(v), ascending), deg, boundary, and the four counts of the call"""


def adjacency(T, nV):
    Tall = np.asarray(T).reshape(-1, 3)
    T = valid_triangles(Tall, nV)
    a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
    b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
    m = a != b  # a side a -> a is no use of any edge
    a, b = a[m], b[m]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key, uses = np.unique(lo * (1 << 32) + hi, return_counts=True)
    lo, hi = key >> 32, key & 0xFFFFFFFF
    src, dst = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    o = np.lexsort((dst, src))
    src, dst = src[o], dst[o]
    A = Adjacency()
    A.deg = np.bincount(src, minlength=nV).astype(np.int64)
    A.start = np.concatenate([[0], np.cumsum(A.deg)]).astype(np.int64)
    A.nbr = dst
    A.boundary = np.zeros(nV, bool)
    A.boundary[lo[uses == 1]] = True
    A.boundary[hi[uses == 1]] = True
    A.max_degree = int(A.deg.max()) if nV else 0
    A.isolated_vertices = int(np.count_nonzero(A.deg == 0))
    A.boundary_vertices = int(np.count_nonzero(A.boundary))
    A.invalid_triangles = int(Tall.shape[0] - T.shape[0])
    return A


def one_pass(P, A, fixed, f):
    """P -> P' with factor f: s = P[w1]; s = s + P[wk], ascending w; m = s / deg; L = m - P[v]; P'[v] = (real)(P[v] + f * L)"""
    s = np.zeros((P.shape[0], 3), np.float64)
    for k in range(A.max_degree):
        m = A.deg > k
        x = P[A.nbr[A.start[:-1][m] + k]].astype(np.float64)
        s[m] = (s[m] + x) if k else x
    move = ~fixed
    out = P.copy()  # (a fixed row is copied as it is)
    p = P[move].astype(np.float64)
    L = s[move] / A.deg[move].astype(np.float64)[:, None] - p
    out[move] = (p + f * L).astype(P.dtype)
    return out


def smooth(V, T, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, A=None):
    """(P, A): the smoothed rows in V's dtype and the adjacency with its counts.  A factor equal to 0 skips its pass."""
    V = np.asarray(V)
    A = A or adjacency(T, V.shape[0])
    fixed = (A.deg == 0) | (A.boundary if pin_boundary else False)
    P = V.copy()
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            for f in (lam, mu):
                if f != 0:
                    P = one_pass(P, A, fixed, float(f))
    return P, A


def vertex_normals(Q, T):
    """oN float32 [nV, 3] from the positions Q: per vertex the cross products of the valid triangles that name it, ascending,
    each once, added in that order starting from the first; divided by the length where that is > 0 and finite, else zeros"""
    Q = np.asarray(Q)
    nV = Q.shape[0]
    T = valid_triangles(T, nV)
    out = np.zeros((nV, 3), np.float32)
    if not T.shape[0]:
        return out
    with np.errstate(all="ignore"):
        p0, p1, p2 = (Q[T[:, k]].astype(np.float64) for k in range(3))
        u, w = p1 - p0, p2 - p0
        g = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        v = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])
        t = np.tile(np.arange(T.shape[0], dtype=np.int64), 3)
        key = np.unique(v * (1 << 32) + t)  # (a triangle that names v twice: once; sorted by vertex, then triangle)
        v, t = key >> 32, key & 0xFFFFFFFF
        cnt = np.bincount(v, minlength=nV)
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        n = np.zeros((nV, 3), np.float64)
        for k in range(int(cnt.max())):
            m = cnt > k
            x = g[t[start[m] + k]]
            n[m] = (n[m] + x) if k else x
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (ln > 0) & np.isfinite(ln) & (cnt > 0)
        out[ok] = (n[ok] / ln[ok][:, None]).astype(np.float32)
    return out


def face_normals(V, T):
    p0, p1, p2 = (np.asarray(V)[np.asarray(T)[:, k].astype(np.int64)].astype(np.float64) for k in range(3))
    return np.cross(p1 - p0, p2 - p0)


def random_mesh(nV, seed, fan=0):
    """Seeded random vertices and 2 nV triangles: most name vertices within 8 of a base, every 97th is fully random, some are
    degenerate, some exact duplicates (non-manifold and misoriented edges); fan: that many more triangles around vertex 0."""
    rng = np.random.default_rng(seed)
    nT = 2 * nV
    if nV > 8:
        base = rng.integers(0, nV, nT)
        T = (base[:, None] + rng.integers(0, 8, (nT, 3))) % nV
        T[::97] = rng.integers(0, nV, (len(T[::97]), 3))
        T[5::101, 1] = T[5::101, 0]
        T[7::103] = T[6::103][:len(T[7::103])]
    else:
        T = rng.integers(0, max(nV, 1), (nT, 3))
    if fan:
        assert nV > fan + 1
        k = np.arange(fan)
        T = np.concatenate([T, np.stack([np.zeros(fan, np.int64), 1 + k, 1 + (k + 1) % fan], 1)])
    V = rng.standard_normal((nV, 3)).astype(np.float32)
    return V, np.ascontiguousarray(T.astype(np.uint32).reshape(-1, 3))
