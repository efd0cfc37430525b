"""tests/mesh_pieces.py against the numpy oracles, and the oracles against mesh_pieces' closed forms: for every length set that
tests/test_gpu_mesh_pieces.py runs, in all six orders of vertices and triangles, measure_oracle.label_components,
measure_oracle.component_table and topology_oracle.surface must give the table that follows from the construction alone - strips
and tetrahedra have their edges, boundary, loops and Euler number in closed form.  No GPU."""
import numpy as np
import pytest

import measure_oracle as mo
import mesh_pieces as mp
import smooth_oracle as so
import topology_oracle as to

ORDERS = [(v, t) for v in mp.VERTEX_ORDERS for t in mp.TRIANGLE_ORDERS]
INTEGER_COLUMNS = [n for n in mp.ROW.names if n != "piece"]


def against_the_oracles(V, T, owner, exp):
    nV, nT = V.shape[0], T.shape[0]
    tab = exp["table"]
    lab, nc, nu, _ = mo.label_components(T, nV)
    assert np.array_equal(lab, exp["labels"]) and (nc, nu) == (exp["components"], exp["unreferenced"])
    root_of_piece = np.zeros(tab.shape[0], np.int64)
    root_of_piece[tab["piece"]] = tab["root"]
    assert np.array_equal(lab[T[:, 0].astype(np.int64)], root_of_piece[owner])  # owner names the piece whose root labels the triangle
    measured = mo.component_table(V, T, lab, np.zeros(3))[0]
    for col in ("root", "nV", "nT"):
        assert np.array_equal(measured[col], tab[col]), col
    assert np.all(np.diff(tab["root"].astype(np.int64)) > 0)
    surface, rows = to.surface(T, nV, lab)
    assert surface == exp["surface"], {k: (surface[k], exp["surface"][k]) for k in surface if surface[k] != exp["surface"][k]}
    assert rows.shape[0] == tab.shape[0]
    for col in INTEGER_COLUMNS:
        assert np.array_equal(rows[col], tab[col]), col


@pytest.mark.parametrize("vertex_order,triangle_order", ORDERS)
@pytest.mark.parametrize("name", list(mp.SETS))
def test_closed_forms_equal_the_oracles(name, vertex_order, triangle_order):
    kw = mp.SETS[name]
    L = np.asarray(kw["lengths"])
    V, T, owner, exp = mp.pieces(seed=7, vertex_order=vertex_order, triangle_order=triangle_order, **kw)
    closed = (L == 4) & (np.arange(L.size) % kw["closed_every"] == 0) if kw.get("closed_every") else np.zeros(L.size, bool)
    nV = int(np.where(closed, 4, L + 2).sum()) + kw.get("unreferenced", 0)
    assert V.dtype == np.float32 and V.shape == (nV, 3) and T.dtype == np.uint32 and T.shape == (int(L.sum()), 3)
    assert owner.dtype == np.int64 and np.array_equal(np.bincount(owner, minlength=L.size), L)
    if name.startswith("edge-"):
        assert nV == int(name.split("-")[1])
    against_the_oracles(V, T, owner, exp)


def test_the_sizes_the_issue_quotes():
    V, T, owner, exp = mp.pieces(seed=7, vertex_order="permuted", triangle_order="robin", **mp.LADDER)
    assert (V.shape[0], T.shape[0], exp["components"], exp["unreferenced"]) == (35623, 35376, 120, 7)
    V, T, owner, exp = mp.pieces(seed=7, vertex_order="permuted", triangle_order="runs", **mp.SMALL)
    assert (V.shape[0], exp["components"], exp["surface"]["closed_components"]) == (346673, 65000, 21667) and V.shape[0] > 262144
    V, T, owner, exp = mp.pieces(seed=7, vertex_order="permuted", triangle_order="robin", **mp.LONG)
    assert T.shape[0] > 524288 and V.shape[0] > 524288


def test_orders():
    """identity: contiguous ids, the root the first vertex; runs: piece after piece; robin: triangle k of every piece before
    triangle k + 1 of any; the same seed gives the same mesh, another seed another"""
    kw = dict(lengths=[3, 1, 4, 4, 2], unreferenced=2, closed_every=3)
    V, T, owner, exp = mp.pieces(seed=1, vertex_order="identity", triangle_order="runs", **kw)
    assert owner.tolist() == [0] * 3 + [1] + [2] * 4 + [3] * 4 + [4] * 2
    assert exp["table"]["root"].tolist() == [0, 5, 8, 14, 18] and exp["table"]["nV"].tolist() == [5, 3, 6, 4, 4] and V.shape[0] == 24
    assert T[:4].tolist() == [[0, 1, 2], [2, 1, 3], [2, 3, 4], [5, 6, 7]]
    assert exp["table"]["boundary_edges"].tolist() == [5, 3, 6, 0, 4] and exp["labels"][-2:].tolist() == [22, 23]
    against_the_oracles(V, T, owner, exp)
    V, T, owner, exp = mp.pieces(seed=1, vertex_order="identity", triangle_order="robin", **kw)
    assert owner.tolist() == [0, 1, 2, 3, 4, 0, 2, 3, 4, 0, 2, 3, 2, 3]
    for vo, order in ORDERS:
        a = mp.pieces(seed=5, vertex_order=vo, triangle_order=order, **kw)
        b = mp.pieces(seed=5, vertex_order=vo, triangle_order=order, **kw)
        c = mp.pieces(seed=6, vertex_order=vo, triangle_order=order, **kw)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3]["table"].tobytes() == b[3]["table"].tobytes()
        assert not np.array_equal(a[0], c[0])
        if vo == "permuted" or order == "shuffle":
            assert not np.array_equal(a[1], c[1])
        against_the_oracles(*a)
    # no piece at all
    V, T, owner, exp = mp.pieces([], 3, "permuted", "shuffle", unreferenced=300)
    assert V.shape == (300, 3) and T.shape == (0, 3)
    against_the_oracles(V, T, owner, exp)


@pytest.mark.parametrize("vertex_order,triangle_order", [("permuted", "shuffle"), ("identity", "runs")])
def test_spoiled_meshes_have_their_defects(vertex_order, triangle_order):
    """every defect class shows in the counts the oracle reports: a spoiled mesh that lost its defects fails here"""
    V, T, owner, exp = mp.pieces(seed=7, vertex_order=vertex_order, triangle_order=triangle_order, **mp.LADDER)
    nV = V.shape[0]
    field = {"duplicate": "nonmanifold_edges", "flip": "misoriented_edges", "degenerate": "degenerate_triangles"}
    before = T.copy()
    for what in mp.DEFECTS + (mp.DEFECTS,):
        S = mp.spoil(T, nV, 11, what)
        assert np.array_equal(T, before) and S.shape == T.shape and S.dtype == np.uint32 and np.array_equal(S, mp.spoil(T, nV, 11, what))
        names = (what,) if isinstance(what, str) else what
        assert np.count_nonzero((S != T).any(axis=1)) == mp.SPOILED_EACH * len(names)
        e = to.EdgeTable(S, nV)
        s = to.surface(S, nV, mo.label_components(S, nV)[0], e)[0]
        for w in mp.DEFECTS:
            got = e.invalid if w == "invalid" else s[field[w]]
            if w in names:
                assert got > 0, (what, w)
                if w in ("degenerate", "invalid"):
                    assert got == mp.SPOILED_EACH
            elif w in ("degenerate", "invalid") or names in (("flip",), ("invalid",)):
                assert got == 0, (what, w)  # (a copy and a degenerate triangle also use edges a third time, or twice in one direction)
        # the defects lie inside runs of one component, not only at their ends
        changed = np.nonzero((S != T).any(axis=1))[0]
        if triangle_order == "runs":
            inside = (changed > 0) & (changed < T.shape[0] - 1)
            inside &= (owner[np.maximum(changed - 1, 0)] == owner[changed]) & (owner[np.minimum(changed + 1, T.shape[0] - 1)] == owner[changed])
            assert np.count_nonzero(inside) > 0.9 * changed.size


def test_loop_roots_equal_the_plain_union_find():
    """topology_oracle.loop_roots against the union-find it replaced, on boundary edges that are loops and on some that are not"""
    V, T, owner, exp = mp.pieces(seed=7, vertex_order="permuted", triangle_order="shuffle", **mp.LADDER)
    for S, nV in ((T, V.shape[0]), (mp.spoil(T, V.shape[0], 11, mp.DEFECTS), V.shape[0]), (so.random_mesh(4097, 1)[1], 4097)):
        e = to.EdgeTable(S, nV)
        for pick in (e.boundary, e.nonmanifold, np.ones(e.lo.size, bool), np.zeros(e.lo.size, bool)):
            assert np.array_equal(to.loop_roots(e.lo[pick], e.hi[pick], nV), to.loop_roots_plain(e.lo[pick], e.hi[pick], nV))


def test_one_long_loop_takes_few_rounds():
    """the boundary of one strip of 1025 triangles, ids permuted: one loop of 1027 edges whose labels have no order along it.  The
    rounds of topology_oracle.loop_labels must grow like the logarithm of the length (each is several passes over all edges)."""
    for seed in range(5):
        V, T, owner, exp = mp.pieces([1025], seed, "permuted", "shuffle", unreferenced=100)
        e = to.EdgeTable(T, V.shape[0])
        lo, hi = e.lo[e.boundary], e.hi[e.boundary]
        assert lo.size == 1027
        lab, rounds = to.loop_labels(lo, hi, V.shape[0])
        root = int(exp["table"]["root"][0])
        assert np.all(lab[np.concatenate([lo, hi])] == root) and to.loop_roots(lo, hi, V.shape[0]).tolist() == [root]
        assert np.array_equal(to.loop_roots_plain(lo, hi, V.shape[0]), [root])
        print("seed %d: %d rounds" % (seed, rounds))
        assert rounds <= 2 * 11 + 2, rounds  # (2 log2(1027) and the round that finds nothing to do)


def test_random_meshes_are_not_manifold():
    """the two triangle soups of tests/smooth_oracle.py that the GPU test runs: what they hold"""
    V, T = so.random_mesh(4097, 1)
    s = to.surface(T, 4097, mo.label_components(T, 4097)[0])[0]
    assert min(s["nonmanifold_edges"], s["misoriented_edges"], s["degenerate_triangles"], s["boundary_loops"]) > 0
    V, T = so.random_mesh(262145, 1)
    s = to.surface(T, 262145, mo.label_components(T, 262145)[0])[0]
    assert (s["edges"], s["nonmanifold_edges"], s["misoriented_edges"], s["boundary_loops"]) == (832037, 127332, 74996, 315), s
