"""Made-up meshes for the clipping by a plane (tests/test_clip_cpu.py, tests/test_gpu_clip.py): the triangle lists of
tests/mesh_pieces.py with positions assigned here, so that the plane z = 0 meets them where the test chooses, and the tiny mesh
with every in / on / out pattern; and what the CPU and the GPU tests of the part share: the cases on the reference's meshes with
the oracle's results, made once, and the structs of the C API filled."""
import ctypes as C

import numpy as np

import clip_oracle as co
import mesh_pieces as mp
import simplify_cases as sc
from mc33_c_library_amd.api import SurfaceClip
from mesh_checks import reference_mesh

PLANE_Z = (0.0, 0.0, 1.0, 0.0)  # z >= 0 stays
RUNS = (1, 2, 63, 64, 65, 255, 256, 257, 1025)

# ---- the tiny mesh: the plane is z = 0; vertices 0-2 are in, 3-5 on the plane, 6-8 out; 9 has a NaN, 10 is in with z = +inf ----
TINY_V = np.array([[0.0, 0.0, 1.0], [4.0, 0.0, 1.0], [0.0, 4.0, 3.0],
                   [1.0, 1.0, 0.0], [5.0, 1.0, 0.0], [1.0, 5.0, -0.0],
                   [2.0, 2.0, -1.0], [6.0, 2.0, -3.0], [2.0, 6.0, -1.0],
                   [np.nan, 1.0, 1.0], [7.0, 7.0, np.inf]], np.float32)
TINY_N = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0],
                   [0.0, 0.0, -1.0], [0.0, 0.6, 0.8], [0.6, 0.0, 0.8],
                   [0.0, 0.0, -1.0], [0.0, -1.0, 0.0], [0.0, 1.0, 0.0],
                   [0.5, 0.5, 0.5], [0.25, 0.5, 0.75]], np.float32)
TINY_A = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 10.0, 9.0, 11.0, 12.0], np.float32)


def tiny_triangles():
    """every class triple (c0, c1, c2), c in in / on / out: corner k takes vertex 3 c + k - all 27 patterns, every pattern in
    its three rotations -, then the cut edge {0, 6} once more in the other direction, a triangle with two equal indices across
    the plane, the NaN vertex (out, its s is not finite), the infinite one (in) and an invalid triangle"""
    T = [[3 * c0 + 0, 3 * c1 + 1, 3 * c2 + 2] for c0 in range(3) for c1 in range(3) for c2 in range(3)]
    T += [[6, 0, 1], [0, 6, 0], [0, 9, 1], [10, 6, 3], [0, 1, 11]]
    return np.array(T, np.uint32)


def tiny_repeated(copies):
    """the tiny mesh `copies` times, every copy on vertices of its own (the invalid triangle names the row behind all of them)"""
    T = tiny_triangles().astype(np.int64)
    nv = TINY_V.shape[0]
    bad = T == nv
    Ts = []
    for k in range(copies):
        t = T + k * nv
        t[bad] = copies * nv
        Ts.append(t)
    return np.tile(TINY_V, (copies, 1)), np.tile(TINY_N, (copies, 1)), np.concatenate(Ts).astype(np.uint32), np.tile(TINY_A, copies)


def normals(nV, seed):
    """unit vectors, finite and none of them zero"""
    n = np.random.default_rng(seed).standard_normal((nV, 3))
    n[np.abs(n).sum(axis=1) == 0.0] = 1.0
    return (n / np.sqrt((n * n).sum(axis=1))[:, None]).astype(np.float32)


def floats(nV, seed):
    return np.random.default_rng(seed).standard_normal(nV).astype(np.float32)


def tile_edge(nV, seed, unreferenced=5):
    """(V, N, T): mesh_pieces' strips over exactly nV vertices with its standard-normal positions, the triangles shuffled: the
    plane z = 0 cuts about half of them, and a seeded tenth of the vertices lies exactly on it"""
    V, T, _, _ = mp.pieces(mp.tile_edge(nV, unreferenced), seed, "identity", "shuffle", unreferenced=unreferenced)
    V = V.copy()
    V[np.random.default_rng(seed + 1).random(nV) < 0.1, 2] = 0.0
    return V, normals(nV, seed + 2), T


def runs(seed, lengths=RUNS):
    """(V, N, T, kinds): strips in the order of T - for every length of `lengths` a strip of that many triangles that are all cut
    (its vertices alternate between z = 1 and z = -3), then a strip of three whole triangles and one of two dropped ones; kinds
    int64 [nT]: 0 cut, 1 whole, 2 dropped"""
    L, kind = [], []
    for n in lengths:
        L += [n, 3, 2]
        kind += [0, 1, 2]
    V, T, owner, _ = mp.pieces(L, seed, "identity", "runs")
    L, kind = np.asarray(L), np.asarray(kind)
    voff = np.concatenate([[0], np.cumsum(L + 2)])
    piece = np.repeat(np.arange(L.size), L + 2)
    k = np.arange(V.shape[0]) - voff[piece]
    V = V.copy()
    V[:, 2] = np.where(kind[piece] == 1, 2.0, np.where(kind[piece] == 2, -2.0, np.where(k % 2 == 0, 1.0, -3.0)))
    return V, normals(V.shape[0], seed + 1), T, kind[owner]


def shared_edge(seed, uses=5000, nT=60000):
    """(V, N, T, first): the cut edge {0, 1} - vertex 0 in, vertex 1 out - named by `uses` triangles (0, 1, x) and (1, 0, x),
    every x a vertex of its own, at seeded rows of a T of nT triangles, the others strips that the plane z = 0 cuts at random;
    first: the smallest of those rows - the owner, well behind the start of T"""
    rng = np.random.default_rng(seed)
    V0, T0, _, _ = mp.pieces(mp.tile_edge(nT, 0), seed, "identity", "shuffle")
    T0 = T0[:nT - uses].astype(np.int64) + 2
    nV0 = V0.shape[0] + 2
    x = nV0 + np.arange(uses)
    fan = np.stack([np.zeros(uses, np.int64), np.ones(uses, np.int64), x], axis=1)
    fan[1::2] = fan[1::2][:, [1, 0, 2]]
    fan = np.stack([np.roll(row, int(s)) for row, s in zip(fan, rng.integers(0, 3, uses))])
    rows = np.sort(rng.permutation(np.arange(3000, nT))[:uses])
    rows = rows[rng.permutation(uses)]
    T = np.empty((nT, 3), np.int64)
    mask = np.zeros(nT, bool)
    mask[rows] = True
    T[rows] = fan
    T[~mask] = T0
    V = np.concatenate([np.array([[0.0, 0.0, 1.0], [1.0, 0.0, -1.0]], np.float32), V0, rng.standard_normal((uses, 3)).astype(np.float32)])
    return V, normals(V.shape[0], seed + 1), np.ascontiguousarray(T.astype(np.uint32)), int(rows.min())


def duplicated(seed):
    """(V, N, T): a tile_edge mesh with 300 copies of its triangles planted among them, every second with the opposite winding,
    all rotated, copies before originals and behind them (simplify_cases.plant_duplicates): cut edges with more than two uses, in
    both directions"""
    V, N, T = tile_edge(6000, seed)
    T2, _ = sc.plant_duplicates(T, 300, seed + 3)
    return V, N, T2


def nonfinite(seed):
    """(V, N, T): a tile_edge mesh of 5000 vertices, seeded vertices of which have a NaN, +inf or -inf coordinate"""
    V, N, T = tile_edge(5000, seed)
    rng = np.random.default_rng(seed + 4)
    rows = rng.permutation(5000)[:300]
    V[rows, rng.integers(0, 3, 300)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), 300)
    return V, N, T


# ---- the cases on the reference's meshes (tests/test_clip_cpu.py pins the oracle to TABLE, tests/test_gpu_clip.py the device) ----

PLANES = ("oblique", "on-grid", "miss", "all")
MODES = (co.LERP_F32, co.COPY)

# (fixture, plane) -> nV_out, nT_out, kept, cut vertices, on the plane, whole, cut, dropped triangles (no invalid triangle, no
# vertex whose s is not finite)
TABLE = {
    ("sphere", "oblique"): (11112, 21625, 10515, 597, 0, 20730, 597, 20729),
    ("sphere", "on-grid"): (11793, 23316, 11793, 0, 268, 23316, 0, 18740),
    ("sphere", "miss"): (21030, 42056, 21030, 0, 0, 42056, 0, 0),
    ("sphere", "all"): (0, 0, 0, 0, 0, 0, 0, 42056),
    ("blobs", "oblique"): (13564, 26578, 13068, 496, 0, 25834, 496, 25834),
    ("blobs", "on-grid"): (13596, 26610, 13596, 0, 528, 26610, 0, 25554),
    ("blobs", "miss"): (26136, 52164, 26136, 0, 0, 52164, 0, 0),
    ("blobs", "all"): (0, 0, 0, 0, 0, 0, 0, 52164),
    ("sheet", "oblique"): (7993, 15171, 7536, 457, 0, 14486, 455, 14491),
    ("sheet", "on-grid"): (11648, 22496, 11648, 0, 288, 22496, 0, 6936),
    ("sheet", "miss"): (15072, 29432, 15072, 0, 0, 29432, 0, 0),
    ("sheet", "all"): (0, 0, 0, 0, 0, 0, 0, 29432),
    ("noise", "oblique"): (27552, 54401, 24307, 3245, 0, 49592, 3212, 50080),
    ("noise", "on-grid"): (25547, 53093, 25547, 0, 822, 53093, 0, 49791),
    ("noise", "miss"): (48809, 102884, 48809, 0, 0, 102884, 0, 0),
    ("noise", "all"): (0, 0, 0, 0, 0, 0, 0, 102884),
    ("quant", "oblique"): (9289, 18449, 7946, 1343, 16, 16454, 1358, 16136),
    ("quant", "on-grid"): (8499, 17781, 8499, 0, 480, 17781, 0, 16167),
    ("quant", "miss"): (15775, 33948, 15775, 0, 0, 33948, 0, 0),
    ("quant", "all"): (0, 0, 0, 0, 0, 0, 0, 33948),
}


def plane_of(V, which):
    """the four planes of a mesh, exact functions of its vertices: oblique through the middle of the bounding box; x - x0 with x0
    the most frequent x of the vertices - a whole grid plane of them has s == 0 exactly; one that misses; one that removes all"""
    lo, hi = V.min(axis=0).astype(np.float64), V.max(axis=0).astype(np.float64)
    if which == "oblique":
        n = np.array([0.3, -0.5, 0.8])
        c = 0.5 * (lo + hi)
        return (n[0], n[1], n[2], -float((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]))
    if which == "on-grid":
        x, count = np.unique(V[:, 0], return_counts=True)
        inner = (x > lo[0] + 0.25 * (hi[0] - lo[0])) & (x < hi[0] - 0.25 * (hi[0] - lo[0]))
        return (1.0, 0.0, 0.0, -float(x[inner][np.argmax(count[inner])]))
    if which == "miss":
        return (1.0, 0.0, 0.0, 1.0 - float(lo[0]))
    return (1.0, 0.0, 0.0, -1.0 - float(hi[0]))


def attributes(nV):
    """a float per vertex (interpolated) and a word per vertex (copied)"""
    return (floats(nV, 11), np.random.default_rng(12).integers(0, 1 << 32, nV, dtype=np.uint64).astype(np.uint32))


_results = {}


def clipped(reflibs, name, which):
    """the oracle's result of one case on a fixture row's reference surface, computed once, shared and left unchanged"""
    key = (name, which)
    if key not in _results:
        s = reference_mesh(reflibs, name)[4]
        _results[key] = co.clip(s.V, s.N, s.T, plane_of(s.V, which), attributes(s.nV), MODES)
    return _results[key]


def cclip(planes):
    """an mc33_clip of the planes"""
    cl = SurfaceClip(len(planes))
    for k, pl in enumerate(planes[:6]):
        for j in range(4):
            cl.plane[k][j] = pl[j]
    return cl


def cbox(lib, lo, hi):
    """MC33_clip_box of an MC33Lib: the mc33_clip and its six planes as tuples"""
    three = C.c_double * 3
    cl = SurfaceClip()
    assert lib.lib.MC33_clip_box(C.byref(three(*lo)), C.byref(three(*hi)), C.byref(cl)) == 0
    return cl, [tuple(cl.plane[k][j] for j in range(4)) for k in range(6)]
