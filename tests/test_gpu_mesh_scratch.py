"""GPU test of the scratch the passes over a finished mesh share (mc33_c_library_amd/csrc/mc33_mesh.hip.h): keep
flags, new indices and tile sums are one set of arrays on the context, so a call finds in them what a LARGER call of another part
left.  One context; compaction, clipping, simplification (with the normals of its output), vertex normals, compaction, clipping,
on meshes of 263169, 1025, 4097, 1025, 262145 and 3 vertices: 263169 and 262145 are the smallest sizes that reach the second
round of 256 tiles of the top scan, 1025 is one tile and one vertex, 3 is one triangle.  Every result is compared bit for bit
with the oracle of its part, as the tests of the parts do."""
import numpy as np
import pytest

import clip_cases as cc
import clip_oracle as co
import filter_oracle as fo
import measure_oracle as mo
import simplify_oracle as sp
import smooth_oracle as so
from clip_cases import MODES
from mesh_harness import ClipCall as Clip, CompactCall as Compact, SimplifyCall as Simplify, bits, tiny_grid, to_device, words

pytestmark = pytest.mark.gpu

CELL, ORIGIN = (0.5, 0.5, 0.5), (-16.0, -16.0, -16.0)  # standard-normal positions: several vertices to a cell, none clamped


def compact(g, nV):
    V, N, T = cc.tile_edge(nV, nV)
    lab = mo.label_components(T, nV)[0]
    own = np.unique(lab[T[:, 0]])
    roots = own[np.random.default_rng(nV).random(own.size) < 0.5].astype(np.uint32)
    A = (words(nV, 31), words(nV, 32))
    want = fo.compact(V, N, T, lab, roots, False, attrs=A)
    assert 0 < want.nV_out < nV - 5 and want.left_out == 0
    call = Compact(g, to_device(V), to_device(N), to_device(T), to_device(lab), roots, False, attrs=[to_device(x) for x in A])
    assert call.rc == 0, call.message
    call.check(want)


def clip(g, nV):
    V, N, T = cc.tile_edge(nV, nV, unreferenced=5 if nV > 3 else 0)
    A = (cc.floats(nV, 21), words(nV, 22))
    want = co.clip(V, N, T, cc.PLANE_Z, A, MODES)
    assert want.invalid_triangles == 0 and (nV == 3 or want.cut_triangles > nV // 4)
    call = Clip(g, to_device(V), to_device(N), to_device(T), cc.PLANE_Z, [to_device(x) for x in A], MODES)
    assert call.rc == 0, call.message
    call.check(want)


def simplify(g, nV):
    V, _, T = cc.tile_edge(nV, nV)
    A = (words(nV, 41), words(nV, 42))
    want = sp.simplify(V, T, CELL, ORIGIN, sp.MEAN, True)
    assert 0 < want.nV_out < (nV - 5) // 2 and want.clamped_vertices == 0 and want.nT_out > 0  # (the lattice merges vertices)
    call = Simplify(g, to_device(V), to_device(T), CELL, ORIGIN, sp.MEAN, True, attrs=[to_device(x) for x in A])
    assert call.rc == 0, call.message
    call.check(want, A)  # (oN too: the normals of the output, by the passes of mc33hip_vertex_normals)


def vertex_normals(g, nV):
    V, _, T = cc.tile_edge(nV, nV)
    got = g.vertex_normals(to_device(V), to_device(T))
    assert np.array_equal(bits(got.cpu().numpy()), bits(so.vertex_normals(V, T)))


def test_one_context_calls_of_shrinking_sizes():
    g = tiny_grid()
    try:
        for call, nV in ((compact, 263169), (clip, 1025), (simplify, 4097), (vertex_normals, 1025), (compact, 262145), (clip, 3)):
            call(g, nV)
    finally:
        g.close()
