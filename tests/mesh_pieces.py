"""Made-up meshes for the stages that work on a finished mesh (labels, measures, topology): a disjoint union of triangle strips
and closed tetrahedra whose vertex ids and triangle order can be arranged at will, with the integer table every component must
get written down in closed form - no oracle is asked - and a way to spoil a triangle list with seeded defects.  numpy only."""
import numpy as np

# a closed, consistently oriented tetrahedron on the vertices 0 .. 3
TETRAHEDRON = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
COUNTS = ("edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges", "degenerate_triangles", "boundary_loops")
# the columns of the component table of the topology (tests/topology_oracle.py has the same names), then the piece the row describes
ROW = np.dtype([("root", np.uint32), ("nV", np.uint32), ("nT", np.uint32)] + [(n, np.uint64) for n in COUNTS] + [("euler", np.int64), ("genus", np.int32),
                                                                                                                   ("piece", np.int64)])
VERTEX_ORDERS = ("identity", "permuted")
TRIANGLE_ORDERS = ("runs", "robin", "shuffle")
DEFECTS = ("duplicate", "flip", "degenerate", "invalid")
SPOILED_EACH = 300  # triangles per defect


def pieces(lengths, seed, vertex_order, triangle_order, unreferenced=0, closed_every=0):
    """(V float32 [nV, 3], T uint32 [nT, 3], owner int64 [nT], expected).  Piece c is a strip of lengths[c] triangles on
    lengths[c] + 2 vertices - triangle k names the strip's vertices k, k + 1, k + 2, the first two exchanged where k is odd, so
    that the strip is consistently oriented - or, where closed_every divides c and lengths[c] == 4, a closed tetrahedron;
    `unreferenced` vertices that no triangle names follow.  owner[i] is the piece of triangle i.

    vertex_order "identity": piece c owns a contiguous range of ids and its root - its smallest id - is its first vertex;
    "permuted": one seeded permutation of all ids.  triangle_order "runs": piece after piece; "robin": triangle k of every
    piece before triangle k + 1 of any; "shuffle": seeded.

    expected: dict of `table` (ROW, ascending root), `labels` (uint32 [nV]: the root of the vertex's piece, its own id where
    no triangle names it), `components`, `unreferenced` and `surface` (the totals, by the names of the topology's struct)."""
    assert vertex_order in VERTEX_ORDERS and triangle_order in TRIANGLE_ORDERS
    rng = np.random.default_rng(seed)
    L = np.asarray(lengths, np.int64).reshape(-1)
    assert np.all(L >= 1)
    n = L.size
    closed = (L == 4) & (np.arange(n) % closed_every == 0) if closed_every else np.zeros(n, bool)
    pv = np.where(closed, 4, L + 2)  # vertices per piece
    voff = np.concatenate([[0], np.cumsum(pv)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    nref, nT = int(voff[-1]), int(toff[-1])
    nV = nref + int(unreferenced)
    owner = np.repeat(np.arange(n, dtype=np.int64), L)
    k = np.arange(nT, dtype=np.int64) - toff[owner]
    odd = k & 1
    T = np.stack([k + odd, k + 1 - odd, k + 2], axis=1)
    tet = closed[owner]
    T[tet] = TETRAHEDRON[k[tet]]
    T += voff[owner][:, None]
    ids = rng.permutation(nV).astype(np.int64) if vertex_order == "permuted" else np.arange(nV, dtype=np.int64)
    T = ids[T]
    if triangle_order == "robin":
        order = np.lexsort((owner, k))
    elif triangle_order == "shuffle":
        order = rng.permutation(nT)
    else:
        order = np.arange(nT)
    T, owner = T[order], owner[order]
    V = rng.standard_normal((nV, 3)).astype(np.float32)
    # the closed forms
    roots = np.minimum.reduceat(ids[:nref], voff[:-1]) if n else np.zeros(0, np.int64)
    labels = np.arange(nV, dtype=np.int64)
    labels[ids[:nref]] = np.repeat(roots, pv)
    tab = np.zeros(n, ROW)
    tab["root"], tab["nV"], tab["nT"], tab["piece"] = roots, pv, L, np.arange(n)
    tab["edges"] = np.where(closed, 6, 2 * L + 1)
    tab["boundary_edges"] = np.where(closed, 0, L + 2)
    tab["boundary_loops"] = np.where(closed, 0, 1)
    tab["euler"] = np.where(closed, 2, 1)
    tab = tab[np.argsort(roots, kind="stable")]
    s = {"nV": nV, "nT": nT, "referenced_vertices": nref if nT else 0, "edges": int(tab["edges"].sum()), "boundary_edges": int(tab["boundary_edges"].sum()),
         "nonmanifold_edges": 0, "misoriented_edges": 0, "degenerate_triangles": 0, "boundary_loops": int(tab["boundary_loops"].sum()), "components": n,
         "closed_components": int(np.count_nonzero(closed)), "genus_sum": 0, "euler": int(tab["euler"].sum()), "closed": int(np.all(closed)),
         "manifold": 1, "oriented": 1, "genus_defined": 1}
    expected = {"table": tab, "labels": labels.astype(np.uint32), "components": n, "unreferenced": int(unreferenced), "surface": s}
    return V, np.ascontiguousarray(T.astype(np.uint32)), owner, expected


def spoil(T, nV, seed, what):
    """A copy of T with seeded defects; `what`: one of DEFECTS or several of them.  Each defect takes SPOILED_EACH triangles of its
    own, drawn from all of T - so most of them lie inside a run of triangles of one component, not at its ends:
    "duplicate": the triangle becomes an exact copy of another, untouched one (edges with more uses than two);
    "flip": its first two indices are exchanged (edges used twice in the same direction);
    "degenerate": T[i, 2] = T[i, 0];  "invalid": one index, any of the three, is set to nV."""
    what = (what,) if isinstance(what, str) else tuple(what)
    assert what and all(w in DEFECTS for w in what)
    T = np.array(T, dtype=np.uint32).reshape(-1, 3)
    nT = T.shape[0]
    assert nT >= (len(DEFECTS) + 1) * SPOILED_EACH
    rng = np.random.default_rng(seed)
    pick = rng.permutation(nT)[:(len(DEFECTS) + 1) * SPOILED_EACH].reshape(len(DEFECTS) + 1, SPOILED_EACH)  # (the last row: what is copied)
    column = rng.integers(0, 3, SPOILED_EACH)
    for w in what:
        i = pick[DEFECTS.index(w)]
        if w == "duplicate":
            T[i] = T[pick[-1]]
        elif w == "flip":
            T[i, 0], T[i, 1] = T[i, 1].copy(), T[i, 0].copy()
        elif w == "degenerate":
            T[i, 2] = T[i, 0]
        else:
            T[i, column] = nV
    return T


# ---- the length sets the tests use (tests/test_mesh_pieces_cpu.py pins every one of them, tests/test_gpu_mesh_pieces.py runs them) ---

STRIP = 61  # triangles of the strips of tile_edge: 63 vertices, so that the pieces' ends drift across lanes and tiles


def tile_edge(nV, unreferenced):
    """lengths for exactly nV vertices, `unreferenced` of them behind the pieces: strips of STRIP triangles, one or two shorter
    strips that take what is left over, and a single triangle last - in "identity" order its root is nV - 3 - unreferenced"""
    body = nV - unreferenced - 3
    assert body == 0 or body >= 3  # (0: the single triangle alone)
    q, r = divmod(body, STRIP + 2)
    if r in (1, 2):  # too few vertices for a strip: a full strip less, and two shorter ones
        q, r = q - 1, r + STRIP + 2
        pads = [r // 2, r - r // 2]
    else:
        pads = [r] if r else []
    assert q >= 0 and all(p >= 3 for p in pads)
    return [STRIP] * q + [p - 2 for p in pads] + [1]


LADDER = dict(lengths=[1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025] * 8, unreferenced=7)  # run lengths around a wave, a block, a tile
SMALL = dict(lengths=[4] * 65000, unreferenced=7, closed_every=3)  # 65 000 components, every third a tetrahedron; more than 256 tiles of vertices
SINGLE = dict(lengths=[1] * 87000)  # runs of one
# Above 8 blocks per CU x 256 lanes - 524 288 triangles or vertices on 256 CUs - a block's piece is more than one step of its waves,
# and only then does a lane hold a row from one step into the next: the smallest round figures past that
LONG = dict(lengths=[64] * 8800)
TILE_EDGE_SIZES = (1023, 1024, 1025, 1026, 262143, 262144, 262145, 262146, 263169)  # around 1 and 256 tiles of 1024 vertices; 257 tiles + 1: 258 tiles, the last of one vertex
TILE_EDGE_MORE = (1027, 262147)  # the last tile holds three vertices: the single triangle's, its root first
SETS = {"ladder": LADDER, "small": SMALL, "single": SINGLE, "long": LONG}
SETS.update({"edge-%d-%d" % (nV, u): dict(lengths=tile_edge(nV, u), unreferenced=u) for nV in TILE_EDGE_SIZES + TILE_EDGE_MORE for u in (0, 1)})
