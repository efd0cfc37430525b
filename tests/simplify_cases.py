"""Made-up meshes for the vertex clustering (tests/test_gpu_simplify.py): the triangle lists of tests/mesh_pieces.py with positions
assigned here, so that the referenced vertices fall into lattice cells in numbers the test chooses; and what the CPU and the GPU
tests of the part share: the cases on the reference's meshes with the oracle's results, made once."""
import ctypes as C

import numpy as np

import mesh_pieces as mp
import simplify_oracle as sp
from mc33_c_library_amd.api import SurfaceSimplification
from mesh_checks import reference_mesh

ORIGIN, CELL = (-3.0, 1.0, 0.5), (0.5, 0.25, 2.0)  # cells whose edges float32 holds exactly
SIDE = 160  # clusters per row and rows per layer of the made-up lattices: 65 000 clusters take three layers


def clustered(sizes, seed, scattered, unreferenced=5, vertex_order="identity"):
    """(V float32 [nV, 3], T uint32 [nT, 3]): strips over sum(sizes) + unreferenced vertices (mesh_pieces.tile_edge: exactly that
    many), the referenced ones - the ids below sum(sizes) - dealt to len(sizes) lattice cells, sizes[c] of them to cell c:
    consecutive ids (the strips then wander through the ids by a seeded renaming), or, scattered, a seeded permutation, so that
    the members of a cluster and its representative lie anywhere in the array.  Cell c is (c % SIDE, c / SIDE % SIDE, c / SIDE^2) of the lattice ORIGIN, CELL; a vertex lies at a seeded place
    between 1/8 and 7/8 of its cell on every axis, far enough from the faces that float32 keeps it inside.  The unreferenced
    vertices get places of their own, NaN among them.  vertex_order "permuted": the ids of V and T renamed by one seeded
    permutation afterwards."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    nref = int(sizes.sum())
    nV = nref + unreferenced
    V0, T, _, _ = mp.pieces(mp.tile_edge(nV, unreferenced), seed, "identity", "shuffle", unreferenced=unreferenced)
    assert V0.shape[0] == nV
    cluster = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    if scattered:
        cluster = cluster[rng.permutation(nref)]
    else:  # the clusters stay runs of ids; the strips are led through them by a seeded renaming, or nearly every triangle would collapse
        ids = np.arange(nV, dtype=np.int64)
        ids[:nref] = rng.permutation(nref)
        T = ids[T.astype(np.int64)].astype(np.uint32)
    k = np.stack([cluster % SIDE, cluster // SIDE % SIDE, cluster // (SIDE * SIDE)], axis=1).astype(np.float64)
    frac = rng.integers(1, 8, (nref, 3)).astype(np.float64) / 8.0 + rng.integers(0, 1 << 16, (nref, 3)).astype(np.float64) / float(1 << 20)
    V = np.empty((nV, 3), np.float32)
    V[:nref] = (np.asarray(ORIGIN) + np.asarray(CELL) * (k + frac)).astype(np.float32)
    V[nref:] = rng.standard_normal((unreferenced, 3)).astype(np.float32)
    if unreferenced:
        V[nref, 0] = np.nan
    if vertex_order == "permuted":
        ids = rng.permutation(nV)
        W = np.empty_like(V)
        W[ids] = V
        V, T = W, ids[T.astype(np.int64)].astype(np.uint32)
    return V, np.ascontiguousarray(T)


def plant_duplicates(T, n, seed):
    """a copy of T with n more triangles, copies of seeded triangles of T, every second with the opposite winding and all with
    their corners rotated, put at seeded places among the others: (T2, where) - where[j]: the row of T2 that holds copy j"""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, np.uint32).reshape(-1, 3)
    src = rng.permutation(T.shape[0])[:n]
    copies = T[src].copy()
    copies[1::2] = copies[1::2][:, [1, 0, 2]]
    copies = np.stack([np.roll(row, int(s)) for row, s in zip(copies, rng.integers(0, 3, n))]) if n else copies
    order = rng.permutation(T.shape[0] + n)
    T2 = np.concatenate([T, copies])[order]
    where = np.argsort(order)[T.shape[0]:]
    return np.ascontiguousarray(T2), where


def edge_of_the_lattice(seed):
    """(V, T, clamped): a strip mesh of 4 000 referenced vertices at cell 1 from origin 0, among them keys that differ only in the
    top bits of one axis (k and k + 2^20), cells at k = 2097151, and vertices that are clamped - negative, at and beyond the far
    end, infinite, NaN - on one axis or on all; clamped: how many referenced vertices that makes"""
    rng = np.random.default_rng(seed)
    nref, un = 4000, 3
    _, T, _, _ = mp.pieces(mp.tile_edge(nref + un, un), seed, "identity", "shuffle", unreferenced=un)
    k = rng.integers(3, 9, (nref, 3)).astype(np.float64)
    axis = rng.integers(0, 3, nref)
    kind = rng.integers(0, 8, nref)
    rows = np.arange(nref)
    k[rows[kind == 1], axis[kind == 1]] += 1048576.0          # the same low bits, another top bit
    k[rows[kind == 2], axis[kind == 2]] = 2097151.0           # the last cell
    V = (k + rng.integers(1, 4, (nref, 3)).astype(np.float64) / 4.0).astype(np.float32)  # (quarters: exact in float32 up to 2^22)
    V[rows[kind == 3], axis[kind == 3]] = -rng.integers(1, 50, np.count_nonzero(kind == 3)).astype(np.float32) / 4.0
    V[rows[kind == 4], axis[kind == 4]] = np.float32(2097152.0)
    V[rows[kind == 5], axis[kind == 5]] = rng.choice(np.array([3e9, np.inf, -np.inf, 4194304.5], np.float32), np.count_nonzero(kind == 5))
    V[rows[kind == 6], axis[kind == 6]] = np.nan
    V[rows[kind == 7][::9]] = np.nan                          # every axis
    clamped = int(np.count_nonzero((kind >= 3) & (kind <= 6))) + int(rows[kind == 7][::9].size)
    V = np.concatenate([V, np.array([[np.nan] * 3, [-1.0, 5.0, 5.0], [5.0, 5.0, 5.0]], np.float32)])
    return V, np.ascontiguousarray(T), clamped


# ---- the cases on the reference's meshes (tests/test_simplify_cpu.py pins the oracle to TABLE, tests/test_gpu_simplify.py the device) ----

CELLS = {"2x2x2": (2.0, 2.0, 2.0), "3x2x5": (3.0, 2.0, 5.0)}  # in grid cells
MODES = {"mean": sp.MEAN, "first": sp.FIRST}

# (fixture, cell) -> nV_out, nT_out, clusters, max_cluster, collapsed, duplicates (duplicates dropped; the mode changes none of them)
TABLE = {
    ("sphere", "2x2x2"): (4568, 9132, 4568, 14, 32924, 0),
    ("sphere", "3x2x5"): (2136, 4268, 2136, 31, 37788, 0),
    ("blobs", "2x2x2"): (5611, 11114, 5611, 15, 41050, 0),
    ("blobs", "3x2x5"): (2551, 5045, 2551, 36, 47062, 57),
    ("sheet", "2x2x2"): (3220, 6106, 3220, 11, 23326, 0),
    ("sheet", "3x2x5"): (1558, 2889, 1558, 27, 26542, 1),
    ("noise", "2x2x2"): (3892, 17388, 3898, 38, 83001, 2495),
    ("noise", "3x2x5"): (1258, 6913, 1258, 90, 92975, 2996),
    ("quant", "2x2x2"): (1728, 7271, 1728, 20, 25911, 766),
    ("quant", "3x2x5"): (480, 2596, 480, 55, 30313, 1039),
}

_results = {}


def simplified(reflibs, name, cell, mode, drop=True):
    """the oracle's result of one case on a fixture row's reference surface, computed once, shared and left unchanged"""
    key = (name, cell, mode, drop)
    if key not in _results:
        data, r0, d, iso, s = reference_mesh(reflibs, name)
        c = tuple(CELLS[cell][k] * d[k] for k in range(3))
        _results[key] = sp.simplify(s.V, s.T, c, r0, MODES[mode], drop)
    return _results[key]


def csimp(cell, mode, drop):
    """an mc33_simplification"""
    return SurfaceSimplification((C.c_double * 3)(*cell), mode, int(drop))
