"""The caps at the grid faces (include/mc33_hip.h: mc33hip_cap_surface) restated in numpy and plain loops, step for
step as the header numbers them: face bits of the vertices, the sides used once, their face cells, the regular cells and their
polygons, the new vertices in grid point order, the new triangles by face, cell and polygon.  Every decision is an integer
comparison or one IEEE double operation written on a line of its own; the device is held to this bit for bit.  numpy only."""
import numpy as np

COUNTS = ("nV_out", "nT_out", "cap_vertices", "cap_triangles", "rim_segments", "capped_cells", "skipped_cells", "off_face_edges", "invalid_triangles",
          "nonfinite_vertices", "solid_above", "closed")
WORD, F32 = 0, 1  # attr_mode: a new vertex gets the word 0 / the float NaN
QNAN = 0x7FC00000
FLIP = (1, 0, 0, 1, 1, 0)  # face f: P0 P1 P2 P3 in the (u, w) plane run clockwise as seen from outside the box


def in_plane(f):
    """the axes u (the faster one) and w of the face's plane: x faces (y, z), y faces (x, z), z faces (x, y)"""
    a = f >> 1
    return (1 if a == 0 else 0), (1 if a == 2 else 2)


def tolerance(r0, d, shape):
    """per axis, in grid units: 2^-21 max(|r0|, |r0 + N d|) / |d|, at most 1/4 (the header says why)"""
    N = (shape[2] - 1, shape[1] - 1, shape[0] - 1)
    out = []
    for a in range(3):
        m = max(abs(float(r0[a])), abs(float(r0[a]) + float(N[a]) * float(d[a])))
        t = np.ldexp(m, -21) / abs(float(d[a]))
        out.append(min(t, 0.25))
    return np.array(out, np.float64)


def grid_coords(V, r0, d, tol):
    """(g, gs): g = ((double)V - r0) * (1.0 / d), and g snapped to the nearest integer r = floor(g + 0.5) where |g - r| <= tol"""
    g = (np.asarray(V).astype(np.float64) - np.asarray(r0, np.float64)) * (1.0 / np.asarray(d, np.float64))
    r = np.floor(g + 0.5)
    with np.errstate(invalid="ignore"):
        return g, np.where(np.abs(g - r) <= tol, r, g)


def classes(data, iso, real):
    """(above, below, bad) of every sample: v = iso - F in MC33_real (a NaN sample stays NaN); bad: v == 0 or NaN"""
    F = np.asarray(data).astype(real)
    with np.errstate(invalid="ignore"):
        v = np.where(F != F, F, real(iso) - F)
    nan = v != v
    on = v == 0
    neg = np.signbit(v)
    return ~nan & ~on & neg, ~nan & ~on & ~neg, nan | on


class Box:
    def __init__(self, lo, hi):
        self.lo, self.hi = [int(x) for x in lo], [int(x) for x in hi]
        self.b = [self.hi[a] - self.lo[a] + 1 for a in range(3)]  # points per axis
        self.plane = self.b[0] * self.b[1]
        self.ring = 2 * self.b[0] + 2 * (self.b[1] - 2)
        self.points = 2 * self.plane + (self.b[2] - 2) * self.ring
        self.face_cells, self.face_off = [], []
        off = 0
        for f in range(6):
            u, w = in_plane(f)
            self.face_off.append(off)
            self.face_cells.append((self.b[u] - 1) * (self.b[w] - 1))
            off += self.face_cells[-1]
        self.cells = off

    def point_index(self, p):
        """the place of a point of the box's surface among all of them, in ascending order of the grid point index"""
        x, y, z = (p[a] - self.lo[a] for a in range(3))
        bx, by, bz = self.b
        if z == 0:
            return y * bx + x
        if z == bz - 1:
            return self.plane + (bz - 2) * self.ring + y * bx + x
        base = self.plane + (z - 1) * self.ring
        if y == 0:
            return base + x
        if y == by - 1:
            return base + bx + 2 * (by - 2) + x
        assert x == 0 or x == bx - 1
        return base + bx + 2 * (y - 1) + (1 if x == bx - 1 else 0)

    def corners(self, f, cu, cw):
        """the four grid points of face cell (cu, cw) - absolute indices - counterclockwise as seen from outside, from P0"""
        a = f >> 1
        u, w = in_plane(f)
        fixed = self.hi[a] if f & 1 else self.lo[a]
        out = []
        for du, dw in ((0, 0), (0, 1), (1, 1), (1, 0)) if FLIP[f] else ((0, 0), (1, 0), (1, 1), (0, 1)):
            p = [0, 0, 0]
            p[a], p[u], p[w] = fixed, cu + du, cw + dw
            out.append(tuple(p))
        return out


class Capped:
    def counts(self):
        return tuple(int(getattr(self, n)) for n in COUNTS)


def positive(f, u, w, ga, gb, c):
    """corner c lies on the positive side of b -> a in the plane of face f, counterclockwise as seen from outside"""
    p = (ga[u] - gb[u]) * (c[w] - gb[w])
    q = (ga[w] - gb[w]) * (c[u] - gb[u])
    s = p - q
    return (-s if FLIP[f] else s) > 0.0


def plan(f, segs, solid, Q, ends, gs):
    """the polygons of a regular cell as lists of entries ("v", vertex) / ("c", k: corner Q[k]) - or None: the cell is skipped.
    segs: the words i << 2 | e of its segments, ascending; solid: the four flags of Q; ends: word -> (a, b)."""
    ns = sum(solid)
    diagonal = ns == 2 and solid[0] == solid[2]
    expect = 0 if ns in (0, 4) else (2 if diagonal else 1)
    if len(segs) != expect:
        return None
    if ns == 0:
        return []
    if ns == 4:
        return [[("c", 0), ("c", 1), ("c", 2), ("c", 3)]]
    if expect == 1:
        a, b = ends[segs[0]]
        first = [k for k in range(4) if solid[k] and not solid[(k + 3) & 3]][0]
        return [[("v", b), ("v", a)] + [("c", (first + j) & 3) for j in range(ns)]]
    u, w = in_plane(f)
    pos = [[positive(f, u, w, gs[ends[s][0]], gs[ends[s][1]], Q[k]) for k in range(4)] for s in segs]
    sol = [k for k in range(4) if solid[k]]
    emp = [k for k in range(4) if not solid[k]]
    cut = [[k for k in sol if pos[j][k]] for j in range(2)]
    if len(cut[0]) == 1 and len(cut[1]) == 1 and cut[0] != cut[1]:  # every segment cuts off a solid corner of its own
        return [[("v", ends[segs[j]][1]), ("v", ends[segs[j]][0]), ("c", cut[j][0])] for j in range(2)]
    out = [[k for k in emp if not pos[j][k]] for j in range(2)]
    if len(cut[0]) == 2 and len(cut[1]) == 2 and len(out[0]) == 1 and len(out[1]) == 1 and out[0] != out[1]:
        poly = []
        for j in range(2):  # the solid corner that follows the empty corner the segment cuts off
            poly += [("v", ends[segs[j]][1]), ("v", ends[segs[j]][0]), ("c", (out[j][0] + 1) & 3)]
        return [poly]
    return None


def cap(V, N, T, data, iso, r0=(0.0, 0.0, 0.0), d=(1.0, 1.0, 1.0), lo=None, hi=None, invert=False, normal_neg=False, attrs=(), attr_modes=()):
    V, N, T = np.asarray(V), np.asarray(N, np.float32), np.asarray(T, np.uint32).reshape(-1, 3)
    real = V.dtype.type
    nV, nT = V.shape[0], T.shape[0]
    shape = data.shape
    box = Box(lo if lo is not None else (0, 0, 0), hi if hi is not None else (shape[2] - 1, shape[1] - 1, shape[0] - 1))
    o = Capped()
    o.solid_above = int(bool(invert) == bool(normal_neg))
    if invert:  # the second and third index exchanged, the normals negated: the caps are made for this surface
        T = np.ascontiguousarray(T[:, [0, 2, 1]])
        N = (N.view(np.uint32) ^ np.uint32(0x80000000)).view(np.float32)
    above, below, bad = classes(data, iso, real)
    solid_grid = above if o.solid_above else below
    # 1. the face bits of every vertex, the sides used once
    tol = tolerance(r0, d, shape)
    graw, gs = grid_coords(V, r0, d, tol)
    o.nonfinite_vertices = int(np.count_nonzero(~np.isfinite(V.astype(np.float64)).all(axis=1))) if nV else 0
    bits = np.zeros(nV, np.int64)
    for a in range(3):
        bits |= np.where(gs[:, a] == box.lo[a], 1 << (2 * a), 0) | np.where(gs[:, a] == box.hi[a], 2 << (2 * a), 0)
    Ti = T.astype(np.int64)
    ok = (Ti < nV).all(axis=1) if nT else np.zeros(0, bool)
    o.invalid_triangles = int(nT - np.count_nonzero(ok))
    rows = np.nonzero(ok)[0]
    sa = np.concatenate([Ti[rows, e] for e in range(3)]) if nT else np.zeros(0, np.int64)
    sb = np.concatenate([Ti[rows, (e + 1) % 3] for e in range(3)]) if nT else np.zeros(0, np.int64)
    word = np.concatenate([rows * 4 + e for e in range(3)]) if nT else np.zeros(0, np.int64)
    keep = sa != sb
    sa, sb, word = sa[keep], sb[keep], word[keep]
    key = (np.minimum(sa, sb).astype(np.uint64) << np.uint64(32)) | np.maximum(sa, sb).astype(np.uint64)
    _, inv, uses = np.unique(key, return_inverse=True, return_counts=True)
    once = np.nonzero(uses[inv] == 1)[0] if key.size else np.zeros(0, np.int64)
    # 2. the face cell of every rim segment
    o.rim_segments = o.off_face_edges = 0
    ends, cell_segs = {}, {}
    for s in once[np.argsort(word[once])]:
        a, b, wd = int(sa[s]), int(sb[s]), int(word[s])
        common = int(bits[a] & bits[b])
        if not common:
            o.off_face_edges += 1
            continue
        f = (common & -common).bit_length() - 1
        u, w = in_plane(f)
        mu = (gs[a, u] + gs[b, u]) * 0.5
        mw = (gs[a, w] + gs[b, w]) * 0.5
        if not (mu >= box.lo[u] and mu <= box.hi[u] and mw >= box.lo[w] and mw <= box.hi[w]):
            o.off_face_edges += 1
            continue
        ru = np.floor((graw[a, u] + graw[b, u]) * 0.5)  # the cell by the coordinates as they are, not the snapped ones
        rw = np.floor((graw[a, w] + graw[b, w]) * 0.5)
        cu = box.lo[u] if not ru > box.lo[u] else min(int(ru), box.hi[u] - 1)
        cw = box.lo[w] if not rw > box.lo[w] else min(int(rw), box.hi[w] - 1)
        o.rim_segments += 1
        ends[wd] = (a, b)
        cell_segs.setdefault((f, cu, cw), []).append(wd)
    # 3. - 4. the cells, face by face, row by row
    polygons, faces, used = [], [], {}
    o.capped_cells = o.skipped_cells = 0
    used_segments = 0
    for f in range(6):
        u, w = in_plane(f)
        for cw in range(box.lo[w], box.hi[w]):
            for cu in range(box.lo[u], box.hi[u]):
                Q = box.corners(f, cu, cw)
                segs = sorted(cell_segs.get((f, cu, cw), []))
                solid = [bool(solid_grid[p[2], p[1], p[0]]) for p in Q]
                if not any(solid) and not segs:
                    continue
                polys = None if any(bad[p[2], p[1], p[0]] for p in Q) else plan(f, segs, solid, Q, ends, gs)
                if polys is None:
                    o.skipped_cells += 1
                    continue
                used_segments += len(segs)
                if polys:
                    o.capped_cells += 1
                for poly in polys:
                    for kind, k in poly:
                        if kind == "c":
                            used[Q[k]] = used.get(Q[k], 0) | (1 << f)
                    polygons.append([("v", k) if kind == "v" else ("p", Q[k]) for kind, k in poly])
                    faces.append(f)
    # 5. the new vertices, in ascending order of the grid point index
    order = sorted(used, key=lambda p: (p[2] * shape[1] + p[1]) * shape[2] + p[0])
    assert [box.point_index(p) for p in order] == sorted(box.point_index(p) for p in order)
    new_id = {p: nV + k for k, p in enumerate(order)}
    o.cap_vertices = len(order)
    newV, newN = np.zeros((len(order), 3), V.dtype), np.zeros((len(order), 3), np.float32)
    for k, p in enumerate(order):
        for a in range(3):
            newV[k, a] = real(p[a]) * real(d[a]) + real(r0[a])
        n = [(1 if used[p] >> (2 * a + 1) & 1 else 0) - (1 if used[p] >> (2 * a) & 1 else 0) for a in range(3)]
        m = np.sqrt(np.float64((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        for a in range(3):
            newN[k, a] = np.float32(np.float64(n[a]) / m) if n[a] else np.float32(0.0)
    # 6. the new triangles: every polygon fanned from its first entry
    tris = []
    for poly in polygons:
        ids = [k if kind == "v" else new_id[k] for kind, k in poly]
        tris += [[ids[0], ids[j], ids[j + 1]] for j in range(1, len(ids) - 1)]
    o.cap_triangles = len(tris)
    o.V = np.concatenate([V, newV])
    o.N = np.concatenate([N, newN])
    o.T = np.concatenate([T, np.array(tris, np.uint32).reshape(-1, 3)])
    o.attrs = []
    for k, A in enumerate(attrs):
        fill = np.uint32(QNAN if attr_modes[k] == F32 else 0)
        o.attrs.append(np.concatenate([np.asarray(A).view(np.uint32), np.full(len(order), fill, np.uint32)]))
    o.nV_out, o.nT_out = nV + o.cap_vertices, nT + o.cap_triangles
    o.cap_faces = np.repeat(np.array(faces, np.int64), [len(p) - 2 for p in polygons]) if polygons else np.zeros(0, np.int64)  # the face of every new triangle
    o.polygon_sizes = [len(p) for p in polygons]
    o.used, o.box = used, box
    o.closed = int(o.skipped_cells == 0 and o.off_face_edges == 0 and used_segments == o.rim_segments)
    return o
