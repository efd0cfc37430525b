"""The surface measures of include/mc33_hip.h (mc33hip_measure_surface, mc33hip_label_components, mc33hip_measure_components;
DESIGN.md 10) restated in numpy float64, operation by operation - nothing fused, the additions of every term in the order the
definition writes them - so that each per-triangle term is the very double the device forms.  Sums are math.fsum of the terms;
what a device sum may differ by is sum_bound().  numpy only."""
import math

import numpy as np

import fixtures as fx

U = 2.0 ** -53


def reference_point(r0, d, shape):
    """c[a] = r0[a] + 0.5 * ((double)N[a] * d[a]); shape = the grid's [Nz, Ny, Nx] points, N = cells per axis"""
    N = (shape[2] - 1, shape[1] - 1, shape[0] - 1)
    return np.array([float(r0[a]) + 0.5 * (float(N[a]) * float(d[a])) for a in range(3)], np.float64)


def valid_triangles(T, nV):
    T = np.asarray(T).astype(np.int64)
    return T[(T < nV).all(axis=1)] if T.size else T.reshape(0, 3)


def triangle_terms(V, T, c, P=None):
    """dict of the per-triangle terms A, W, M (n x 3) and, with P, Q - float64 arrays over the triangles of T (every index < nV)"""
    V = np.asarray(V)
    T = np.asarray(T).astype(np.int64)
    c = np.asarray(c, np.float64)
    p0, p1, p2 = (V[T[:, k]].astype(np.float64) - c for k in range(3))
    u, w = p1 - p0, p2 - p0
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    A = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx = p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]
    my = p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2]
    mz = p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]
    W = ((p0[:, 0] * mx + p0[:, 1] * my) + p0[:, 2] * mz) / 6.0
    M = A[:, None] * (((p0 + p1) + p2) / 3.0)
    out = {"A": A, "W": W, "M": M}
    if P is not None:
        P = np.asarray(P, np.float32).astype(np.float64)
        out["Q"] = A * (((P[T[:, 0]] + P[T[:, 1]]) + P[T[:, 2]]) / 3.0)
    return out


def fsum(x, chunk=1 << 20):
    """math.fsum; over chunk sums for long arrays (the error that adds, chunks x 2^-53 x |sum|, is far inside sum_bound)"""
    x = np.asarray(x, np.float64)
    if x.size <= chunk:
        return math.fsum(x.tolist())
    return math.fsum(math.fsum(x[k:k + chunk].tolist()) for k in range(0, x.size, chunk))


def sum_bound(x):
    """|device sum - fsum(x)| <= (n + 8) 2^-53 fsum(|x|): (n - 1) u sum|x| bounds recursive summation in any order, the rest
    pays for last-place differences of a term itself"""
    x = np.asarray(x, np.float64)
    return (x.size + 8) * U * fsum(np.abs(x))


class Measures:
    pass


AWKWARD_R0, AWKWARD_D = (-1.3, 0.7, 2.9), (0.1, 0.07, 0.13)
# name -> (field: () -> (data, r0, d), isovalue, what the unmodified reference gives: nV, nT, components, unreferenced, open edges)
FIXTURES = {
    "sphere": (lambda: fx.sphere_field(), 1.0, (21030, 42056, 1, 0, 0)),
    "blobs": (lambda: fx.cos_field(96, -10.0, 10.0), 2.0, (26136, 52164, 27, 0, 0)),
    "sheet": (lambda: fx.cos_field(64), 0.0, (15072, 29432, 1, 0, 720)),
    "noise": (lambda: (fx.noise_f32(0, 9, (26, 31, 40)), AWKWARD_R0, AWKWARD_D), 0.05, (48809, 102884, 152, 0, 5778)),
    "quant": (lambda: (fx.noise_quant(24, 5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 0.0, (15800, 33948, 14, 25, 2603)),
}


class _Sum:
    """fsum of a stream of arrays of terms, with the count and the fsum of the magnitudes that sum_bound needs"""

    def __init__(self):
        self.parts, self.mags, self.n = [], [], 0

    def add(self, x):
        self.parts.append(fsum(x))
        self.mags.append(fsum(np.abs(x)))
        self.n += x.size

    def result(self):
        return math.fsum(self.parts), (self.n + 8) * U * math.fsum(self.mags)


def measure(V, T, r0, d, shape, P=None, c=None, chunk=1 << 22):
    """The measures and, beside each sum S, its bound as S_bound.  The terms are formed chunk triangles at a time (a mesh of
    6e7 triangles would not fit otherwise); with one chunk - every fixture but the large one - each sum is one math.fsum."""
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3)
    c = reference_point(r0, d, shape) if c is None else np.asarray(c, np.float64)
    names = ["A", "W", "M0", "M1", "M2"] + (["Q"] if P is not None else [])
    acc = {k: _Sum() for k in names}
    for k0 in range(0, max(T.shape[0], 1), chunk):
        t = triangle_terms(V, valid_triangles(T[k0:k0 + chunk], nV), c, P)
        for k in names:
            acc[k].add(t["M"][:, int(k[1])] if k[0] == "M" else t[k])
    m = Measures()
    m.nV, m.nT = nV, T.shape[0]
    m.origin = c
    m.area, m.area_bound = acc["A"].result()
    m.volume, m.volume_bound = acc["W"].result()
    mom = [acc["M%d" % a].result() for a in range(3)]
    m.moment, m.moment_bound = np.array([x[0] for x in mom]), np.array([x[1] for x in mom])
    m.has_property = int(P is not None)
    m.property_integral, m.property_bound = acc["Q"].result() if P is not None else (0.0, 0.0)
    m.bbox_min, m.bbox_max = np.full(3, np.inf), np.full(3, -np.inf)
    for a in range(3):
        col = V[:, a]
        col = col[~np.isnan(col)]
        if col.size:
            m.bbox_min[a], m.bbox_max[a] = float(col.min()), float(col.max())
    m.centroid = m.origin + m.moment / m.area if m.area else np.full(3, np.nan)
    return m


def label_components(T, nV):
    """(labels uint32 [nV], components, unreferenced, rounds): label[v] = the smallest vertex index connected to v.  Minimum
    propagation over the triangles with pointer jumping between the rounds, until nothing changes."""
    T = valid_triangles(T, nV)
    lab = np.arange(nV, dtype=np.int64)
    rounds = 0
    while T.shape[0]:
        rounds += 1
        m = lab[T].min(axis=1)
        new = lab.copy()
        for k in range(3):
            np.minimum.at(new, T[:, k], m)
            np.minimum.at(new, lab[T[:, k]], m)  # (the old label's own entry: hooks the whole set, not the vertex alone)
        while True:  # pointer jumping
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    referenced = np.zeros(nV, bool)
    referenced[T.reshape(-1)] = True
    owners = np.unique(lab[T[:, 0]]) if T.shape[0] else np.zeros(0, np.int64)
    return lab.astype(np.uint32), int(owners.size), int(nV - np.count_nonzero(referenced)), rounds


COMPONENT = np.dtype([("root", np.uint32), ("nV", np.uint32), ("nT", np.uint32), ("area", np.float64), ("volume", np.float64)], align=True)


def component_table(V, T, labels, c, chunk=1 << 22):
    """(table, area_bound, volume_bound): the component table in ascending order of root and the bound of each double entry"""
    nV = np.asarray(V).shape[0]
    T = valid_triangles(T, nV)
    labels = np.asarray(labels).astype(np.int64)
    A, W = np.empty(T.shape[0]), np.empty(T.shape[0])
    for k0 in range(0, T.shape[0], chunk):
        t = triangle_terms(V, T[k0:k0 + chunk], c)
        A[k0:k0 + chunk], W[k0:k0 + chunk] = t["A"], t["W"]
    owner = labels[T[:, 0]]
    referenced = np.zeros(nV, bool)
    referenced[T.reshape(-1)] = True
    order = np.argsort(owner, kind="stable")
    roots, cuts, counts = np.unique(owner[order], return_index=True, return_counts=True)
    A, W = A[order], W[order]
    vcount = np.bincount(labels[referenced], minlength=max(nV, 1))
    tab = np.zeros(roots.size, COMPONENT)
    ab, wb = np.zeros(roots.size), np.zeros(roots.size)
    for k, r in enumerate(roots):
        a, w = A[cuts[k]:cuts[k] + counts[k]], W[cuts[k]:cuts[k] + counts[k]]
        tab[k] = (r, vcount[r], counts[k], fsum(a), fsum(w))
        ab[k], wb[k] = sum_bound(a), sum_bound(w)
    return tab, ab, wb


def open_edges(T):
    """edges that belong to exactly one triangle (not a measure of the library: the fixtures' table quotes it)"""
    T = np.asarray(T).astype(np.int64)
    e = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])
    e.sort(axis=1)
    _, cnt = np.unique(e[:, 0] * (1 << 32) + e[:, 1], return_counts=True)
    return int(np.count_nonzero(cnt == 1))
