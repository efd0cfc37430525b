"""The vertex clustering of include/mc33_hip.h (mc33hip_simplify_surface) restated in numpy, operation by
operation: the keys in float64 with nothing fused, the sums of the quantised positions as exact uint64 integers, the duplicates
through a dictionary over sorted images.  uint64 -> float64 is numpy's astype, round to nearest even, which is what the device
does.  Nothing here has a tolerance.  numpy only."""
import numpy as np

NONE = 0xFFFFFFFF
MEAN, FIRST = 0, 1
CELLS = 2097152.0       # 2^21 cells per axis
UNIT = 4294967296.0     # 2^32 steps inside a cell


class Simplified:
    """V, T (uint32), attrs (list), vmap (uint32 [nV]), rep (int64 [nV], -1 where unreferenced), and the eight counts by the
    names of the struct: nV_out, nT_out, clusters, max_cluster, collapsed_triangles, duplicate_triangles, invalid_triangles,
    clamped_vertices"""
    COUNTS = ("nV_out", "nT_out", "clusters", "max_cluster", "collapsed_triangles", "duplicate_triangles", "invalid_triangles", "clamped_vertices")

    def counts(self):
        return tuple(int(getattr(self, n)) for n in self.COUNTS)


def keys(V, origin, cell):
    """(k int64 [n, 3], t float64 [n, 3], clamped bool [n]) of every row of V"""
    V = np.asarray(V)
    origin, cell = np.asarray(origin, np.float64), np.asarray(cell, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = (V.astype(np.float64) - origin) / cell
        low = ~(g >= 0.0)               # a NaN too
        high = g >= CELLS
        inside = ~low & ~high
        k = np.zeros(g.shape, np.float64)
        k[inside] = np.floor(g[inside])
        k[high] = CELLS - 1.0
        t = g - k
        t = np.where(t >= 0.0, np.minimum(t, 1.0), 0.0)   # NaN and negatives: 0
    return k.astype(np.int64), t, (low | high).any(axis=1)


def simplify(V, T, cell, origin=(0.0, 0.0, 0.0), mode=MEAN, drop_duplicates=True, attrs=()):
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    origin, cell = np.asarray(origin, np.float64), np.asarray(cell, np.float64)
    valid = (T < nV).all(axis=1) if T.shape[0] else np.zeros(0, bool)
    referenced = np.zeros(nV, bool)
    referenced[T[valid].reshape(-1)] = True
    members = np.nonzero(referenced)[0]
    k, t, clamped = keys(V[members], origin, cell)
    key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
    uniq, first, inverse, count = np.unique(key, return_index=True, return_inverse=True, return_counts=True)  # (first occurrence: the smallest member)
    inverse = inverse.reshape(-1)
    rep = np.full(nV, -1, np.int64)
    rep[members] = members[first][inverse]
    out = Simplified()
    out.rep = rep
    out.clusters, out.max_cluster = int(uniq.size), int(count.max()) if uniq.size else 0
    out.clamped_vertices = int(np.count_nonzero(clamped))
    out.invalid_triangles = int(T.shape[0] - np.count_nonzero(valid))
    # images
    image = np.full(T.shape, -1, np.int64)
    image[valid] = rep[T[valid]]
    collapsed = valid & ((image[:, 0] == image[:, 1]) | (image[:, 1] == image[:, 2]) | (image[:, 2] == image[:, 0]))
    alive = valid & ~collapsed
    out.collapsed_triangles = int(np.count_nonzero(collapsed))
    out.duplicate_triangles = 0
    if drop_duplicates:
        seen = {}
        srt = np.sort(image, axis=1)
        for i in np.nonzero(alive)[0].tolist():  # ascending: the first of a set is the smallest i
            s = (int(srt[i, 0]), int(srt[i, 1]), int(srt[i, 2]))
            if s in seen:
                alive[i] = False
                out.duplicate_triangles += 1
            else:
                seen[s] = i
    keep = np.zeros(nV, bool)
    keep[image[alive].reshape(-1)] = True
    new = np.cumsum(keep) - keep
    out.keep = keep
    out.nV_out, out.nT_out = int(np.count_nonzero(keep)), int(np.count_nonzero(alive))
    out.T = new[image[alive]].astype(np.uint32).reshape(-1, 3)
    out.survivors = np.nonzero(alive)[0]
    if mode == FIRST:
        out.V = V[keep].copy()
    else:
        q = np.floor(t * UNIT).astype(np.uint64)
        S = np.zeros((uniq.size, 3), np.uint64)
        np.add.at(S, inverse, q)
        n = count.astype(np.float64)
        m = S.astype(np.float64) / (n * UNIT)[:, None]
        kc = k[first].astype(np.float64)     # every member of a cluster has the cluster's k
        P = (origin + cell * (kc + m)).astype(V.dtype)
        row = np.full(nV, -1, np.int64)
        row[members[first]] = np.arange(uniq.size)
        out.V = P[row[np.nonzero(keep)[0]]]
    out.attrs = [np.asarray(a)[keep] for a in attrs]
    vmap = np.full(nV, NONE, np.int64)
    ok = referenced.copy()
    ok[members] = keep[rep[members]]
    vmap[ok] = new[rep[ok]]
    out.vmap = vmap.astype(np.uint32)
    return out
