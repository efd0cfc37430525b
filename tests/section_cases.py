"""Made-up meshes for the section by a plane (tests/test_section_cpu.py, tests/test_gpu_section.py): those of tests/clip_cases.py
- the section is the boundary clip opens, so where clip can go wrong the section can - and the tiny mesh with what a section
adds to it.  numpy only."""
import numpy as np

import clip_cases as cc
import section_oracle as so
from mesh_checks import reference_mesh

PLANE_Z = cc.PLANE_Z
RUNS = cc.RUNS
TINY_V, TINY_A = cc.TINY_V, cc.TINY_A
TINY_WORDS = np.arange(11, dtype=np.uint32) * 3 + 1


def tiny_triangles():
    """clip_cases.tiny_triangles - all 27 class patterns in their rotations, the cut edge {0, 6} in both directions, (0, 6, 0)
    whose two cut sides are one point, a NaN and an infinite vertex, an invalid triangle - and then: an ON vertex named twice
    beside an IN one in the three rotations (both ends of the segment are one point: dropped), a triangle that names one ON
    vertex three times (no IN corner: nothing), and the segment 4 -> 3 of pattern (in, on, on) a second time (a point that
    starts two segments)"""
    extra = [[3, 3, 0], [0, 3, 3], [3, 0, 3], [4, 4, 4], [0, 4, 3]]
    return np.concatenate([cc.tiny_triangles(), np.array(extra, np.uint32)])


def tiny_repeated(copies):
    """the tiny mesh `copies` times, every copy on vertices of its own (the invalid triangle names the row behind all of them):
    (V, T, floats, words)"""
    T = tiny_triangles().astype(np.int64)
    nv = TINY_V.shape[0]
    bad = T == nv
    Ts = []
    for k in range(copies):
        t = T + k * nv
        t[bad] = copies * nv
        Ts.append(t)
    return np.tile(TINY_V, (copies, 1)), np.concatenate(Ts).astype(np.uint32), np.tile(TINY_A, copies), np.arange(copies * nv, dtype=np.uint32) * 3 + 1


def tile_edge(nV, seed):
    V, _, T = cc.tile_edge(nV, seed)
    return V, T


def runs(seed, lengths=RUNS):
    V, _, T, kinds = cc.runs(seed, lengths)
    return V, T, kinds


def shared_edge(seed):
    V, _, T, first = cc.shared_edge(seed)
    return V, T, first


def duplicated(seed):
    V, _, T = cc.duplicated(seed)
    return V, T


def nonfinite(seed):
    V, _, T = cc.nonfinite(seed)
    return V, T


def ladder_offsets(V, normal, n):
    """n offsets, strictly ascending, such that the planes sweep the whole mesh: with n > 1 the first and the last miss it"""
    V = np.asarray(V, np.float64)
    V = V[np.isfinite(V).all(axis=1)]
    b = V @ np.asarray(normal, np.float64)
    lo, hi = float(b.min()), float(b.max())
    pad = 0.05 * (hi - lo) + 1e-3
    return [-(hi + pad) + (hi - lo + 2 * pad) * (k / (n - 1) if n > 1 else 0.5) for k in range(n)]


# ---- the cases on the reference's meshes: the planes, attributes and modes of tests/clip_cases.py ----------------------------------

ORIGIN = (1.5, 1.5, 1.5)  # the reference point of the context of mesh_harness.tiny_grid: r0 + 0.5 * N * d of a 4^3 grid

_results = {}


def sectioned(reflibs, name, which):
    """the oracle's result of one case on a fixture row's reference surface, computed once, shared and left unchanged"""
    key = (name, which)
    if key not in _results:
        s = reference_mesh(reflibs, name)[4]
        _results[key] = so.section(s.V, s.T, cc.plane_of(s.V, which), cc.attributes(s.nV), cc.MODES, ORIGIN)
    return _results[key]
