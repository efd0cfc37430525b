"""The nearest triangle per point of include/mc33_hip.h (mc33hip_surface_distance) restated in numpy float64,
operation by operation - nothing fused, every dot product (x*x' + y*y') + z*z' - over ALL pairs of a point and a usable triangle,
in chunks of triangles.  It searches nothing cleverly: it is the brute force the device's lattice must equal, bit for bit.
numpy only."""
import types

import numpy as np

NONE = 0xFFFFFFFF
REGIONS = ("a", "b", "ab", "c", "ac", "bc", "face")  # the region a closest point came from, in the order the walk tests them
PAIRS = 1 << 19  # point-triangle pairs formed at a time


def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def usable_triangles(V, T):
    """(usable bool [nT], invalid, nonfinite): the indices below nV and the nine coordinates finite"""
    V = np.asarray(V)
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    valid = (T < V.shape[0]).all(axis=1) if T.shape[0] else np.zeros(0, bool)
    fin = np.zeros(T.shape[0], bool)
    if V.shape[0]:
        ok = np.isfinite(V.astype(np.float64)).all(axis=1)
        fin[valid] = ok[T[valid]].all(axis=1)
    return valid & fin, int(np.count_nonzero(~valid)), int(np.count_nonzero(valid & ~fin))


def closest(p, a, b, c):
    """q [.., 3] and the region [..] (an index into REGIONS) of the closest point of triangles a, b, c to points p - arrays that
    broadcast against each other.  Every branch is computed for every pair and the first whose test holds is taken."""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        shape = np.broadcast(d1, d3, d5).shape
        region = np.full(shape, 6, np.int8)
        for k in range(5, -1, -1):
            region = np.where(tests[k], np.int8(k), region)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        v, w = vb * den, vc * den
        full = shape + (3,)
        cand = [np.broadcast_to(a, full), np.broadcast_to(b, full), a + v_ab[..., None] * ab, np.broadcast_to(c, full), a + w_ac[..., None] * ac,
                b + w_bc[..., None] * (c - b), (a + ab * v[..., None]) + ac * w[..., None]]
        q = np.array(cand[6])
        for k in range(5, -1, -1):
            q = np.where((region == k)[..., None], cand[k], q)
        lo = np.where(b < a, b, a)
        lo = np.where(c < lo, c, lo)
        hi = np.where(b > a, b, a)
        hi = np.where(c > hi, c, hi)
        q = np.where(~(q >= lo), lo, q)
        q = np.where(~(q <= hi), hi, q)
    return q, region


def distance(P, V, T, signed=False):
    """The definition over all pairs.  Returns a namespace: D2 float64 [nP] (inf without a winner), tri uint32 [nP] (NONE without),
    q float64 [nP, 3] (NaN without), negative bool [nP] (e . (ab x ac) < 0 for the winner), region int8 [nP] (-1 without), dist
    float32 [nP] (signed when asked), point (q in P's dtype), matched bool [nP], the counts, max / min / argmax / argmin, the
    terms of sum and sum_sq, and counts() in the order of COUNTS."""
    P, V = np.asarray(P), np.asarray(V)
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    nP = P.shape[0]
    use, invalid, nonfinite = usable_triangles(V, T)
    idx = np.nonzero(use)[0]
    p64 = P.astype(np.float64).reshape(nP, 3)
    best = np.full(nP, np.inf)
    tri = np.full(nP, NONE, np.int64)
    step = max(1, PAIRS // max(nP, 1))
    with np.errstate(all="ignore"):
        for k0 in range(0, idx.size, step):
            i = idx[k0:k0 + step]
            a, b, c = (V[T[i, k]].astype(np.float64)[None, :, :] for k in range(3))
            q, _ = closest(p64[:, None, :], a, b, c)
            e = p64[:, None, :] - q
            D2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            D2 = np.where(np.isfinite(D2), D2, np.inf)  # (a NaN or infinite D2 never wins)
            j = np.argmin(D2, axis=1)  # (the first minimum: the smallest index of the chunk, and the chunks ascend)
            m = D2[np.arange(nP), j]
            better = m < best
            best = np.where(better, m, best)
            tri = np.where(better, i[j], tri)
        matched = tri != NONE
        w = np.nonzero(matched)[0]
        q = np.full((nP, 3), np.nan)
        region = np.full(nP, -1, np.int8)
        negative = np.zeros(nP, bool)
        if w.size:
            a, b, c = (V[T[tri[w], k]].astype(np.float64) for k in range(3))
            q[w], region[w] = closest(p64[w], a, b, c)
            e = p64[w] - q[w]
            ab, ac = b - a, c - a
            n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
            negative[w] = dot(e, n) < 0
        root = np.sqrt(best)
        dist = root.astype(np.float32)
        if signed:
            dist = np.where(negative, -dist, dist)
    r = types.SimpleNamespace(D2=best, tri=tri.astype(np.uint32), q=q, negative=negative, region=region, dist=dist.astype(np.float32), point=q.astype(P.dtype),
                              matched=matched, invalid_triangles=invalid, nonfinite_triangles=nonfinite)
    return _summary(r)


def _summary(r):
    """the fields the host fills, from the per-point arrays"""
    w = np.nonzero(r.matched)[0]
    best = r.D2
    r.matched_points, r.unmatched_points = int(w.size), int(r.matched.size - w.size)
    with np.errstate(all="ignore"):
        r.sum_terms, r.sum_sq_terms = np.sqrt(best[w]), best[w]
    if w.size:
        r.max, r.min = float(np.sqrt(best[w].max())), float(np.sqrt(best[w].min()))
        r.argmax, r.argmin = int(w[np.argmax(best[w])]), int(w[np.argmin(best[w])])  # (the first index that attains them)
    else:
        r.max = r.min = 0.0
        r.argmax = r.argmin = 0
    r.counts = lambda: (r.matched_points, r.unmatched_points, r.invalid_triangles, r.nonfinite_triangles)
    return r


def head(r, n):
    """the result for the first n points alone: a point's winner does not depend on the other points"""
    return _summary(types.SimpleNamespace(D2=r.D2[:n], tri=r.tri[:n], q=r.q[:n], negative=r.negative[:n], region=r.region[:n], dist=r.dist[:n], point=r.point[:n],
                                          matched=r.matched[:n], invalid_triangles=r.invalid_triangles, nonfinite_triangles=r.nonfinite_triangles))


def own_vertices(V, T):
    """For the vertices of a mesh against the mesh itself, from the INCIDENT triangles alone (every index of T below nV): (zero
    bool [nV] - an incident triangle has D2 == 0 exactly, so the winner's D2 is 0 -, first uint32 [nV] - the smallest index among
    those triangles, NONE where there is none: the winner's index is at most that)."""
    V = np.asarray(V)
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    a, b, c = (V[T[:, k]].astype(np.float64) for k in range(3))
    first = np.full(V.shape[0], NONE, np.int64)
    for k in range(3):
        p = V[T[:, k]].astype(np.float64)
        q, _ = closest(p, a, b, c)
        e = p - q
        D2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        i = np.nonzero(D2 == 0.0)[0]
        np.minimum.at(first, T[i, k], i)
    return first != NONE, first.astype(np.uint32)


COUNTS = ("matched_points", "unmatched_points", "invalid_triangles", "nonfinite_triangles")
