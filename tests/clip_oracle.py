"""The clipping by a plane of include/mc33_hip.h (mc33hip_clip_surface) restated in numpy, operation for operation:
s, t and every new row in float64 with nothing fused, float64 -> float32 by numpy's astype, round to nearest even, which is what
the device does; owners, ranks and places by sorting.  Nothing here has a tolerance.  numpy only.

clip_slow is the same definition a second time, a plain loop over the triangles that follows the walk word for word; the tests
hold the two against each other on small meshes."""
import numpy as np

NONE = 0xFFFFFFFF
COPY, LERP_F32 = 0, 1
OUT, ON, IN = 0, 1, 2


class Clipped:
    """V, N (None without normals), T (uint32), attrs (list of uint32 arrays), vmap (uint32 [nV]), keep (bool [nV]), edges (int64
    [cut_vertices, 2]: lo, hi of every new vertex in rank order), owners (int64 [cut_vertices, 2]: triangle and side), and the ten
    counts by the names of the struct"""
    COUNTS = ("nV_out", "nT_out", "kept_vertices", "cut_vertices", "on_plane_vertices", "whole_triangles", "cut_triangles", "dropped_triangles",
              "invalid_triangles", "nonfinite_vertices")

    def counts(self):
        return tuple(int(getattr(self, n)) for n in self.COUNTS)


def signed(V, plane):
    """s[v] = ((x a + y b) + z c) + w in float64"""
    x = np.asarray(V).astype(np.float64)
    a, b, c, w = (np.float64(p) for p in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((x[:, 0] * a + x[:, 1] * b) + x[:, 2] * c) + w


def classes(s):
    return np.where(s > 0.0, IN, np.where(s == 0.0, ON, OUT))  # (a NaN is out)


def new_rows(V, N, attrs, modes, s, lo, hi):
    """the rows of the new vertices of the cut edges {lo, hi}: (V rows, N rows or None, [attribute words])"""
    slo, shi = s[lo], s[hi]
    inn = np.where(slo > 0.0, lo, hi)
    copy = ~(np.isfinite(slo) & np.isfinite(shi))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = slo / (slo - shi)
        Vd = V.astype(np.float64)
        nv = (Vd[lo] + t[:, None] * (Vd[hi] - Vd[lo])).astype(V.dtype)
        nv[copy] = V[inn[copy]]
        nn = None
        if N is not None:
            Nd = N.astype(np.float64)
            x = Nd[lo] + t[:, None] * (Nd[hi] - Nd[lo])
            m = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
            ok = m > 0.0
            nn = np.zeros((lo.size, 3), np.float32)
            nn[ok] = (x[ok] / m[ok, None]).astype(np.float32)
            nn[copy] = N[inn[copy]]
        na = []
        for a, mode in zip(attrs, modes):
            a = np.ascontiguousarray(a).view(np.uint32)
            if mode == LERP_F32:
                f = a.view(np.float32).astype(np.float64)
                w = (f[lo] + t * (f[hi] - f[lo])).astype(np.float32).view(np.uint32)
                w[copy] = a[inn[copy]]
            else:
                w = a[inn]
            na.append(w)
    return nv, nn, na


def clip(V, N, T, plane, attrs=(), modes=()):
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    nT = T.shape[0]
    attrs = [np.ascontiguousarray(a) for a in attrs]
    modes = list(modes) + [COPY] * (len(attrs) - len(modes))
    s = signed(V, plane)
    cls = classes(s)
    valid = (T < nV).all(axis=1) if nT else np.zeros(0, bool)
    referenced = np.zeros(nV, bool)
    referenced[T[valid].reshape(-1)] = True
    c = np.zeros((nT, 3), np.int64)
    c[valid] = cls[T[valid]]
    has_in = valid & (c == IN).any(axis=1)
    has_out = (c == OUT).any(axis=1)
    p, q = T, T[:, [1, 2, 0]]                       # side e: T[e] -> T[(e + 1) % 3]
    cut_side = has_in[:, None] & ((c ^ c[:, [1, 2, 0]]) == 2)
    emit_p = has_in[:, None] & (c != OUT)
    keep = np.zeros(nV, bool)
    keep[T[emit_p]] = True
    new = np.cumsum(keep) - keep
    kept = int(np.count_nonzero(keep))
    # the cut edges: np.nonzero walks (i, e) in ascending order of i << 2 | e, so the first use of a key is its owner
    ti, te = np.nonzero(cut_side)
    a, b = p[ti, te], q[ti, te]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")        # the edges in ascending order of their owner
    rank_of = np.empty(uniq.size, np.int64)
    rank_of[order] = np.arange(uniq.size)
    side_rank = np.full((nT, 3), -1, np.int64)
    side_rank[ti, te] = rank_of[inverse]
    elo, ehi = lo[first][order], hi[first][order]
    out = Clipped()
    out.keep, out.edges = keep, np.stack([elo, ehi], axis=1)
    out.owners = np.stack([ti[first][order], te[first][order]], axis=1)
    nv, nn, na = new_rows(V, N, attrs, modes, s, elo, ehi)
    out.V = np.concatenate([V[keep], nv])
    out.N = np.concatenate([np.asarray(N)[keep], nn]) if N is not None else None
    out.attrs = [np.concatenate([x.view(np.uint32)[keep], w]) for x, w in zip(attrs, na)]
    # the walk: p0, cut 0, p1, cut 1, p2, cut 2 - the entries that exist, pushed to the front
    vals = np.empty((nT, 6), np.int64)
    mask = np.zeros((nT, 6), bool)
    vals[:, 0::2], mask[:, 0::2] = new[np.minimum(T, max(nV - 1, 0))] if nV else 0, emit_p
    vals[:, 1::2], mask[:, 1::2] = kept + side_rank, cut_side
    at = np.cumsum(mask, axis=1) - 1
    poly = np.full((nT, 4), -1, np.int64)
    for col in range(6):
        rows = np.nonzero(mask[:, col])[0]
        poly[rows, at[rows, col]] = vals[rows, col]
    n = mask.sum(axis=1)
    assert np.all((n[has_in] == 3) | (n[has_in] == 4)) and np.all(n[~has_in] == 0)
    both = np.stack([poly[:, [0, 1, 2]], poly[:, [0, 2, 3]]], axis=1)
    out.T = both[np.stack([has_in, n == 4], axis=1)].astype(np.uint32).reshape(-1, 3)
    out.outputs = np.where(has_in, n - 2, 0)        # output triangles per input triangle
    out.vmap = np.where(keep, new, NONE).astype(np.uint32)
    out.kept_vertices, out.cut_vertices = kept, int(uniq.size)
    out.nV_out, out.nT_out = kept + int(uniq.size), int(out.T.shape[0])
    out.on_plane_vertices = int(np.count_nonzero(keep & (cls == ON)))
    out.whole_triangles = int(np.count_nonzero(has_in & ~has_out))
    out.cut_triangles = int(np.count_nonzero(has_in & has_out))
    out.dropped_triangles = int(np.count_nonzero(valid & ~has_in))
    out.invalid_triangles = int(nT - np.count_nonzero(valid))
    out.nonfinite_vertices = int(np.count_nonzero(referenced & ~np.isfinite(s)))
    return out


def clip_slow(V, N, T, plane, attrs=(), modes=()):
    """the definition once more, a triangle at a time: the walk as include/mc33_hip.h words it"""
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    attrs = [np.ascontiguousarray(a) for a in attrs]
    modes = list(modes) + [COPY] * (len(attrs) - len(modes))
    s = signed(V, plane)
    cls = classes(s)
    owner = {}      # (lo, hi) -> the smallest (i, e)
    polys = []      # per output-bearing triangle: entries ("v", p) or ("c", lo, hi)
    keep = np.zeros(nV, bool)
    referenced = np.zeros(nV, bool)
    whole = cut = dropped = invalid = 0
    for i, tri in enumerate(T.tolist()):
        if any(x >= nV for x in tri):
            invalid += 1
            continue
        referenced[tri] = True
        if not any(cls[x] == IN for x in tri):
            dropped += 1
            continue
        poly = []
        for e in range(3):
            p, q = tri[e], tri[(e + 1) % 3]
            if cls[p] != OUT:
                poly.append(("v", p))
                keep[p] = True
            if (cls[p] == IN and cls[q] == OUT) or (cls[p] == OUT and cls[q] == IN):
                k = (min(p, q), max(p, q))
                poly.append(("c",) + k)
                if k not in owner or (i, e) < owner[k]:
                    owner[k] = (i, e)
        if any(cls[x] == OUT for x in tri):
            cut += 1
        else:
            whole += 1
        polys.append(poly)
    new = np.cumsum(keep) - keep
    kept = int(np.count_nonzero(keep))
    edges = sorted(owner, key=lambda k: owner[k])
    rank = {k: r for r, k in enumerate(edges)}
    tris = []
    for poly in polys:
        e = [int(new[x[1]]) if x[0] == "v" else kept + rank[(x[1], x[2])] for x in poly]
        tris.append([e[0], e[1], e[2]])
        if len(e) == 4:
            tris.append([e[0], e[2], e[3]])
    out = Clipped()
    lo = np.array([k[0] for k in edges], np.int64)
    hi = np.array([k[1] for k in edges], np.int64)
    nv, nn, na = new_rows(V, N, attrs, modes, s, lo, hi)
    out.V = np.concatenate([V[keep], nv])
    out.N = np.concatenate([np.asarray(N)[keep], nn]) if N is not None else None
    out.attrs = [np.concatenate([x.view(np.uint32)[keep], w]) for x, w in zip(attrs, na)]
    out.T = np.array(tris, np.uint32).reshape(-1, 3)
    out.keep = keep
    out.vmap = np.where(keep, new, NONE).astype(np.uint32)
    out.kept_vertices, out.cut_vertices = kept, len(edges)
    out.nV_out, out.nT_out = kept + len(edges), out.T.shape[0]
    out.on_plane_vertices = int(np.count_nonzero(keep & (cls == ON)))
    out.whole_triangles, out.cut_triangles, out.dropped_triangles, out.invalid_triangles = whole, cut, dropped, invalid
    out.nonfinite_vertices = int(np.count_nonzero(referenced & ~np.isfinite(s)))
    return out


def same(a, b):
    """two results, bit for bit"""
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)
    if a.counts() != b.counts() or not np.array_equal(a.T, b.T) or not np.array_equal(a.vmap, b.vmap) or not np.array_equal(bits(a.V), bits(b.V)):
        return False
    if (a.N is None) != (b.N is None) or (a.N is not None and not np.array_equal(bits(a.N), bits(b.N))):
        return False
    return len(a.attrs) == len(b.attrs) and all(np.array_equal(x, y) for x, y in zip(a.attrs, b.attrs))
