"""The topology figures of include/mc33_hip.h (mc33hip_surface_topology, mc33hip_component_topology) restated in
numpy: np.unique over the 64-bit edge keys lo << 32 | hi, minimum propagation over the boundary edges (a plain union-find beside it, to hold it against).  T and nV only; integers
only.  numpy only."""
import numpy as np

SURFACE_FIELDS = ("nV", "nT", "referenced_vertices", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges", "degenerate_triangles",
                  "boundary_loops", "components", "closed_components", "genus_sum", "euler", "closed", "manifold", "oriented", "genus_defined")
COUNTS = ("edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges", "degenerate_triangles", "boundary_loops")
COMPONENT = np.dtype([("root", np.uint32), ("nV", np.uint32), ("nT", np.uint32)] + [(n, np.uint64) for n in COUNTS] + [("euler", np.int64), ("genus", np.int32)],
                     align=True)


class EdgeTable:
    """the distinct edges of the valid triangles of T: lo, hi, forward and backward uses (int64 arrays), and what was left out"""

    def __init__(self, T, nV):
        T = np.asarray(T).reshape(-1, 3).astype(np.int64)
        ok = (T < nV).all(axis=1)
        self.invalid = int(T.shape[0] - np.count_nonzero(ok))
        self.T = T = T[ok]
        self.degenerate = (T[:, 0] == T[:, 1]) | (T[:, 1] == T[:, 2]) | (T[:, 2] == T[:, 0])
        a = np.concatenate([T[:, 0], T[:, 1], T[:, 2]])  # the sides T0 -> T1, T1 -> T2, T2 -> T0
        b = np.concatenate([T[:, 1], T[:, 2], T[:, 0]])
        keep = a != b
        a, b = a[keep], b[keep]
        fwd = a < b
        key = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
        uniq, inv = np.unique(key, return_inverse=True)
        self.lo, self.hi = (uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64)
        self.fwd = np.bincount(inv[fwd], minlength=uniq.size).astype(np.int64)
        self.bwd = np.bincount(inv[~fwd], minlength=uniq.size).astype(np.int64)
        self.uses = self.fwd + self.bwd
        self.boundary = self.uses == 1
        self.nonmanifold = self.uses > 2
        self.misoriented = (self.uses == 2) & (self.fwd != 1)


def loop_labels(lo, hi, nV):
    """(labels int64 [nV], rounds): label[v] = the smallest vertex connected to v through the edges lo - hi, by minimum propagation
    over the edges with pointer jumping between the rounds, until nothing changes (as measure_oracle.label_components does over
    triangles).  At the fixed point both ends of every edge carry one label, no label exceeds its vertex and labels only travel
    inside a connected set: the label is the set's smallest vertex.  Hooking the old label's own entry makes whole sets merge in
    a round, so the rounds grow with the logarithm of a loop's length, not with the length."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    lab = np.arange(nV, dtype=np.int64)
    rounds = 0
    while lo.size:
        rounds += 1
        m = np.minimum(lab[lo], lab[hi])
        new = lab.copy()
        for ends in (lo, hi):
            np.minimum.at(new, ends, m)
            np.minimum.at(new, lab[ends], m)  # (the old label's own entry: hooks the whole set, not the vertex alone)
        while True:  # pointer jumping
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    return lab, rounds


def loop_roots(lo, hi, nV):
    """the smallest vertex of every connected set of the graph with the edges lo - hi; tests/test_mesh_pieces_cpu.py holds it
    against loop_roots_plain"""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    return np.unique(loop_labels(lo, hi, nV)[0][np.concatenate([lo, hi])])


def loop_roots_plain(lo, hi, nV):
    """the same by a plain union-find, smaller root wins: one Python step per edge, for meshes of a few thousand edges"""
    parent = np.arange(nV, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for u, v in zip(lo.tolist(), hi.tolist()):
        u, v = find(u), find(v)
        if u != v:
            parent[max(u, v)] = min(u, v)
    ends = np.unique(np.concatenate([lo, hi]))
    return np.unique(np.array([find(x) for x in ends.tolist()], np.int64))


def genus_of(euler, loops, nonmanifold, degenerate, misoriented):
    twice = 2 - int(euler) - int(loops)
    return twice // 2 if not nonmanifold and not degenerate and not misoriented and twice >= 0 and twice % 2 == 0 else -1


def component_table(T, nV, labels, table=None):
    """the rows of mc33hip_component_topology in ascending order of root; labels as mc33hip_label_components makes them"""
    e = table or EdgeTable(T, nV)
    labels = np.asarray(labels).astype(np.int64)
    owner = labels[e.T[:, 0]]
    roots = np.unique(owner)
    row = np.full(max(nV, 1), -1, np.int64)
    row[roots] = np.arange(roots.size)
    referenced = np.zeros(nV, bool)
    referenced[e.T.reshape(-1)] = True
    n = roots.size

    def per(rows):
        return np.bincount(rows, minlength=n)[:n]
    tab = np.zeros(n, COMPONENT)
    tab["root"] = roots
    tab["nV"] = per(row[labels[referenced]])
    tab["nT"] = per(row[owner])
    edge_row = row[labels[e.lo]]
    tab["edges"] = per(edge_row)
    tab["boundary_edges"] = per(edge_row[e.boundary])
    tab["nonmanifold_edges"] = per(edge_row[e.nonmanifold])
    tab["misoriented_edges"] = per(edge_row[e.misoriented])
    tab["degenerate_triangles"] = per(row[owner[e.degenerate]])
    tab["boundary_loops"] = per(row[labels[loop_roots(e.lo[e.boundary], e.hi[e.boundary], nV)]])
    tab["euler"] = tab["nV"].astype(np.int64) - tab["edges"].astype(np.int64) + tab["nT"].astype(np.int64)
    tab["genus"] = [genus_of(r["euler"], r["boundary_loops"], r["nonmanifold_edges"], r["degenerate_triangles"], r["misoriented_edges"]) for r in tab]
    return tab


def surface(T, nV, labels, table=None):
    """dict of the fields of mc33hip_topology, and the component table"""
    T = np.asarray(T).reshape(-1, 3)
    nT = T.shape[0]
    s = dict.fromkeys(SURFACE_FIELDS, 0)
    s.update(nV=int(nV), nT=int(nT), closed=1, manifold=1, oriented=1, genus_defined=1)
    if not nT:
        return s, np.zeros(0, COMPONENT)
    e = table or EdgeTable(T, nV)
    tab = component_table(T, nV, labels, e)
    referenced = np.zeros(nV, bool)
    referenced[e.T.reshape(-1)] = True
    s["referenced_vertices"] = int(np.count_nonzero(referenced))
    s["edges"] = int(e.uses.size)
    s["boundary_edges"] = int(np.count_nonzero(e.boundary))
    s["nonmanifold_edges"] = int(np.count_nonzero(e.nonmanifold))
    s["misoriented_edges"] = int(np.count_nonzero(e.misoriented))
    s["degenerate_triangles"] = int(np.count_nonzero(e.degenerate))
    s["boundary_loops"] = int(loop_roots(e.lo[e.boundary], e.hi[e.boundary], nV).size)
    s["components"] = int(tab.shape[0])
    s["closed_components"] = int(np.count_nonzero(tab["boundary_edges"] == 0))
    s["genus_sum"] = int(tab["genus"][tab["genus"] >= 0].sum())
    s["euler"] = s["referenced_vertices"] - s["edges"] + (nT - e.invalid)
    s["closed"] = int(s["boundary_edges"] == 0)
    s["manifold"] = int(s["nonmanifold_edges"] == 0 and s["degenerate_triangles"] == 0)
    s["oriented"] = int(s["misoriented_edges"] == 0)
    s["genus_defined"] = int(not np.any(tab["genus"] < 0))
    return s, tab
