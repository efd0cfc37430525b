"""The section by a plane of include/mc33_hip.h (mc33hip_section_surface, mc33hip_section_ladder) restated in numpy,
operation for operation: classes, cut edges, owners, ranks and the rows of the cut points are those of tests/clip_oracle.py (the
section is the boundary clip opens); the on-plane entries of every polygon, the points, the segments and what is counted over
them by sorting and counting; the per-segment terms in float64 with nothing fused.  The integers and arrays have no tolerance;
the sums are math.fsum of the terms, and what a device sum may differ by is measure_oracle.sum_bound of them.  numpy only.

section_slow is the same definition a second time, a plain loop over the triangles that follows the walk word for word; the tests
hold the two against each other."""
import numpy as np

import clip_oracle as co
import measure_oracle as mo
import topology_oracle as to

NONE = co.NONE
OUT, ON, IN = co.OUT, co.ON, co.IN


class Sectioned:
    """P, S (uint32 [nS, 2]), attrs (list of uint32 arrays), label, next (uint32 [nP]), pmap (uint32 [nV]), edges (int64
    [cut_points, 2]: lo, hi of every cut point in rank order), per_triangle (bool [nT]: yields a kept segment), terms (float64
    [nS, 4]: length and the three components of the area vector per segment), the integers by the names of the struct, length,
    area_vector, area (math.fsum) and origin"""
    COUNTS = ("nP_out", "nS_out", "on_points", "cut_points", "isolated_points", "degenerate_segments", "crossing_triangles", "invalid_triangles",
              "nonfinite_vertices", "contours", "closed_contours", "open_ends", "branch_points")
    SIZES = COUNTS[:4] + COUNTS[5:9]  # what a call fills when the capacities are short

    def counts(self):
        return tuple(int(getattr(self, n)) for n in self.COUNTS)

    def sizes(self):
        return tuple(int(getattr(self, n)) for n in self.SIZES)


def segment_terms(P, S, origin):
    """float64 [nS, 4]: sqrt(((q-p).x^2 + (q-p).y^2) + (q-p).z^2) and 0.5 * (p x q), p and q relative to origin"""
    S = np.asarray(S).astype(np.int64).reshape(-1, 2)
    o = np.asarray(origin, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p, q = np.asarray(P)[S[:, 0]].astype(np.float64) - o, np.asarray(P)[S[:, 1]].astype(np.float64) - o
        d = q - p
        out = np.empty((S.shape[0], 4), np.float64)
        out[:, 0] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        out[:, 1] = 0.5 * (p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1])
        out[:, 2] = 0.5 * (p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2])
        out[:, 3] = 0.5 * (p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0])
    return out


def total(x):
    """math.fsum of the terms; NaN where one of them is not finite (a vertex at infinity: nothing is held to such a sum)"""
    x = np.asarray(x, np.float64)
    return mo.fsum(x) if np.isfinite(x).all() else float("nan")


def area_of(G, normal):
    a, b, c = (np.float64(x) for x in normal[:3])
    with np.errstate(invalid="ignore", over="ignore"):
        return float(((G[0] * a + G[1] * b) + G[2] * c) / np.sqrt((a * a + b * b) + c * c))


def finish(out, P, S, nP, plane, origin):
    """what is counted and summed over finished points and segments: the same code serves both restatements"""
    S = S.astype(np.int64).reshape(-1, 2)
    starts = np.bincount(S[:, 0], minlength=nP)[:nP] if nP else np.zeros(0, np.int64)
    stops = np.bincount(S[:, 1], minlength=nP)[:nP] if nP else np.zeros(0, np.int64)
    lab = to.loop_labels(S[:, 0], S[:, 1], nP)[0]
    out.label = lab.astype(np.uint32)
    nxt = np.full(nP, NONE, np.int64)
    nxt[S[:, 0]] = S[:, 1]
    nxt[starts != 1] = NONE
    out.next = nxt.astype(np.uint32)
    named = (starts + stops) > 0
    out.isolated_points = int(np.count_nonzero(~named))
    out.open_ends = int(np.count_nonzero(starts != stops))
    out.branch_points = int(np.count_nonzero((starts > 1) | (stops > 1)))
    roots = np.unique(lab[named])
    bad = np.unique(lab[named & ((starts != 1) | (stops != 1))])
    out.contours, out.closed_contours = int(roots.size), int(roots.size - bad.size)
    out.starts, out.stops = starts, stops
    out.origin = np.asarray(origin, np.float64)
    out.terms = segment_terms(P, S, origin)
    out.length = total(out.terms[:, 0])
    out.area_vector = np.array([total(out.terms[:, k]) for k in (1, 2, 3)])
    out.area = area_of(out.area_vector, plane)
    return out


def section(V, T, plane, attrs=(), modes=(), origin=(0.0, 0.0, 0.0)):
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    nT = T.shape[0]
    attrs = [np.ascontiguousarray(a) for a in attrs]
    modes = list(modes) + [co.COPY] * (len(attrs) - len(modes))
    s = co.signed(V, plane)
    cls = co.classes(s)
    valid = (T < nV).all(axis=1) if nT else np.zeros(0, bool)
    referenced = np.zeros(nV, bool)
    referenced[T[valid].reshape(-1)] = True
    c = np.zeros((nT, 3), np.int64)
    c[valid] = cls[T[valid]]
    has_in = valid & (c == IN).any(axis=1)
    has_out = (c == OUT).any(axis=1)
    p, q = T, T[:, [1, 2, 0]]
    cut_side = has_in[:, None] & ((c ^ c[:, [1, 2, 0]]) == 2)
    # the cut edges, their owners and ranks: clip's
    ti, te = np.nonzero(cut_side)
    a, b = p[ti, te], q[ti, te]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")
    rank_of = np.empty(uniq.size, np.int64)
    rank_of[order] = np.arange(uniq.size)
    side_rank = np.full((nT, 3), -1, np.int64)
    side_rank[ti, te] = rank_of[inverse]
    elo, ehi = lo[first][order], hi[first][order]
    # the walk: p0, cut 0, p1, cut 1, p2, cut 2 - the entries that exist, and which of them lie on the plane; an entry's id is
    # its vertex, or nV + rank for a cut vertex
    inpoly = np.zeros((nT, 6), bool)
    onpl = np.zeros((nT, 6), bool)
    ids = np.zeros((nT, 6), np.int64)
    inpoly[:, 0::2], inpoly[:, 1::2] = has_in[:, None] & (c != OUT), cut_side
    onpl[:, 0::2], onpl[:, 1::2] = has_in[:, None] & (c == ON), cut_side
    ids[:, 0::2], ids[:, 1::2] = T, nV + side_rank
    pos = np.cumsum(inpoly, axis=1) - 1
    two = onpl.sum(axis=1) == 2
    assert np.all(onpl.sum(axis=1) <= 2)
    rows = np.arange(nT)
    c1 = np.argmax(onpl, axis=1)
    c2 = 5 - np.argmax(onpl[:, ::-1], axis=1)
    fwd = pos[rows, c2] == pos[rows, c1] + 1  # (otherwise they are the last and the first entry of the polygon)
    ida = np.where(fwd, ids[rows, c1], ids[rows, c2])
    idb = np.where(fwd, ids[rows, c2], ids[rows, c1])
    degenerate = two & (ida == idb)
    kept = two & ~degenerate
    on = np.zeros(nV, bool)
    ends = np.concatenate([ida[kept], idb[kept]])
    on[ends[ends < nV]] = True
    new = np.cumsum(on) - on
    onp, cutv = int(np.count_nonzero(on)), int(uniq.size)

    def point(i):
        return np.where(i < nV, new[np.minimum(i, max(nV - 1, 0))] if nV else 0, onp + (i - nV))
    out = Sectioned()
    out.per_triangle = kept
    out.S = np.stack([point(ida[kept]), point(idb[kept])], axis=1).astype(np.uint32).reshape(-1, 2)
    nv, _, na = co.new_rows(V, None, attrs, modes, s, elo, ehi)
    out.P = np.concatenate([V[on], nv])
    out.attrs = [np.concatenate([x.view(np.uint32)[on], w]) for x, w in zip(attrs, na)]
    out.edges = np.stack([elo, ehi], axis=1)
    out.pmap = np.where(on, new, NONE).astype(np.uint32)
    out.on_points, out.cut_points, out.nP_out, out.nS_out = onp, cutv, onp + cutv, int(out.S.shape[0])
    out.degenerate_segments = int(np.count_nonzero(degenerate))
    out.crossing_triangles = int(np.count_nonzero(has_in & has_out))
    out.invalid_triangles = int(nT - np.count_nonzero(valid))
    out.nonfinite_vertices = int(np.count_nonzero(referenced & ~np.isfinite(s)))
    return finish(out, out.P, out.S, out.nP_out, plane, origin)


def section_slow(V, T, plane, attrs=(), modes=(), origin=(0.0, 0.0, 0.0)):
    """the definition once more, a triangle at a time: the walk as include/mc33_hip.h words it"""
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    attrs = [np.ascontiguousarray(a) for a in attrs]
    modes = list(modes) + [co.COPY] * (len(attrs) - len(modes))
    s = co.signed(V, plane)
    cls = co.classes(s)
    owner = {}      # (lo, hi) -> the smallest (i, e)
    segs = []       # per kept segment: its two entries ("v", p) or ("c", lo, hi)
    per_triangle = np.zeros(T.shape[0], bool)
    on = np.zeros(nV, bool)
    referenced = np.zeros(nV, bool)
    degenerate = crossing = invalid = 0
    for i, tri in enumerate(T.tolist()):
        if any(x >= nV for x in tri):
            invalid += 1
            continue
        referenced[tri] = True
        if not any(cls[x] == IN for x in tri):
            continue
        if any(cls[x] == OUT for x in tri):
            crossing += 1
        poly = []
        for e in range(3):
            p, q = tri[e], tri[(e + 1) % 3]
            if cls[p] != OUT:
                poly.append(("v", p))
            if (cls[p] == IN and cls[q] == OUT) or (cls[p] == OUT and cls[q] == IN):
                k = (min(p, q), max(p, q))
                poly.append(("c",) + k)
                if k not in owner or (i, e) < owner[k]:
                    owner[k] = (i, e)
        at = [j for j, x in enumerate(poly) if x[0] == "c" or cls[x[1]] == ON]
        assert len(at) <= 2
        if len(at) < 2:
            continue
        j, k = at
        assert k == j + 1 or (j == 0 and k == len(poly) - 1)  # neighbours in the cyclic polygon
        a, b = (poly[j], poly[k]) if k == j + 1 else (poly[k], poly[j])
        if a == b:
            degenerate += 1
            continue
        per_triangle[i] = True
        segs.append((a, b))
        for x in (a, b):
            if x[0] == "v":
                on[x[1]] = True
    new = np.cumsum(on) - on
    onp = int(np.count_nonzero(on))
    edges = sorted(owner, key=lambda k: owner[k])
    rank = {k: r for r, k in enumerate(edges)}

    def point(x):
        return int(new[x[1]]) if x[0] == "v" else onp + rank[(x[1], x[2])]
    out = Sectioned()
    out.per_triangle = per_triangle
    out.S = np.array([[point(a), point(b)] for a, b in segs], np.uint32).reshape(-1, 2)
    lo = np.array([k[0] for k in edges], np.int64)
    hi = np.array([k[1] for k in edges], np.int64)
    nv, _, na = co.new_rows(V, None, attrs, modes, s, lo, hi)
    out.P = np.concatenate([V[on], nv])
    out.attrs = [np.concatenate([x.view(np.uint32)[on], w]) for x, w in zip(attrs, na)]
    out.edges = np.stack([lo, hi], axis=1).reshape(-1, 2)
    out.pmap = np.where(on, new, NONE).astype(np.uint32)
    out.on_points, out.cut_points, out.nP_out, out.nS_out = onp, len(edges), onp + len(edges), len(segs)
    out.degenerate_segments, out.crossing_triangles, out.invalid_triangles = degenerate, crossing, invalid
    out.nonfinite_vertices = int(np.count_nonzero(referenced & ~np.isfinite(s)))
    return finish(out, out.P, out.S, out.nP_out, plane, origin)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)


def same(a, b):
    """two results, bit for bit"""
    if a.counts() != b.counts() or not np.array_equal(a.S, b.S) or not np.array_equal(bits(a.P), bits(b.P)):
        return False
    if not (np.array_equal(a.label, b.label) and np.array_equal(a.next, b.next) and np.array_equal(a.pmap, b.pmap)):
        return False
    if not np.array_equal(bits(a.terms), bits(b.terms)):
        return False
    return len(a.attrs) == len(b.attrs) and all(np.array_equal(x, y) for x, y in zip(a.attrs, b.attrs))


def contour_table(o):
    """one row per contour in ascending root: (root, points, segments, open_ends, branch_points, closed, length, area) as a list
    of tuples; length and area are math.fsum over the segments of the contour (a segment belongs to the label of its start)"""
    S = o.S.astype(np.int64)
    lab = o.label.astype(np.int64)
    named = (o.starts + o.stops) > 0
    rows = []
    for r in np.unique(lab[named]).tolist():
        pts = named & (lab == r)
        sg = lab[S[:, 0]] == r
        ends = int(np.count_nonzero(pts & (o.starts != o.stops)))
        branch = int(np.count_nonzero(pts & ((o.starts > 1) | (o.stops > 1))))
        closed = int(np.all(o.starts[pts] == 1) and np.all(o.stops[pts] == 1))
        G = [mo.fsum(o.terms[sg, k]) for k in (1, 2, 3)]
        rows.append((r, int(np.count_nonzero(pts)), int(np.count_nonzero(sg)), ends, branch, closed, mo.fsum(o.terms[sg, 0]), G))
    return rows


def ladder(V, T, normal, offsets, origin=(0.0, 0.0, 0.0)):
    """[Sectioned] per offset: what section() reports for the plane (a, b, c, w_k), over the triangles plane k crosses alone -
    the others yield no segment, so nS_out, degenerate_segments and the terms are those of the whole mesh (the numbering of the
    points is not).  base[v] + w_k with base = (x a + y b) + z c is the very s[v] of that plane."""
    V = np.asarray(V)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3)
    Ti = T.astype(np.int64)
    valid = (Ti < nV).all(axis=1) if Ti.shape[0] else np.zeros(0, bool)
    x = V.astype(np.float64)
    a, b, c = (np.float64(p) for p in normal)
    with np.errstate(invalid="ignore", over="ignore"):
        base = (x[:, 0] * a + x[:, 1] * b) + x[:, 2] * c
    out = []
    for w in offsets:
        with np.errstate(invalid="ignore", over="ignore"):
            inside = np.zeros(Ti.shape, bool)
            inside[valid] = (base + np.float64(w))[Ti[valid]] > 0.0
        crossed = valid & inside.any(axis=1) & ~inside.all(axis=1)
        out.append(section(V, T[crossed], (normal[0], normal[1], normal[2], w), origin=origin))
    return out
