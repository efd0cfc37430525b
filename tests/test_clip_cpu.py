"""Clipping extracted surfaces by planes, the part that needs no GPU: the numpy oracle on the unmodified reference's
meshes against figures computed once from them, its invariants, a tiny mesh whose result is written out by hand, the new names
in the headers, the libraries and the code objects, MC33_clip_box, and the host-logic build of mc33_capi.c, whose emulated device
layer cannot clip.

test_oracle_on_the_reference_meshes, the invariant tests and the tiny mesh test the oracle and the fixtures, not the product: the
rows of TABLE pin tests/clip_oracle.py and pass without the feature.  The product is held to that oracle by the name, struct,
export, code-object, clip-box and host-logic tests below - these fail without the feature - and, on the device, by
tests/test_gpu_clip.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clip_cases as cc
import clip_oracle as co
import measure_oracle as mo
import topology_oracle as to
from clip_cases import MODES, PLANES, TABLE, attributes, clipped, plane_of
from mc33_c_library_amd.api import SurfaceClip
from mesh_checks import assert_exported, assert_kernels, host_logic, launched, reference_mesh as mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_clip_surface"]
C_NAMES = ["MC33_calculate_clipped_isosurface", "MC33_clip_box"]
KERNELS = ["k_clip_tri", "k_clip_own", "k_clip_emit"] + launched("k_mesh_clear", "k_mesh_tile_sum<MeshFlag>", "k_mesh_tile_sum<ClipOwned>", "k_mesh_tile_sum<ClipOutputs>",
                                                           "k_mesh_scan_top", "k_mesh_place<MeshFlag, 1>")
@pytest.mark.parametrize("which", PLANES)
@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_oracle_on_the_reference_meshes(reflibs, name, which):
    o = clipped(reflibs, name, which)
    print('    ("%s", "%s"): %r,' % (name, which, o.counts()[:8]))
    assert o.counts()[:8] == TABLE[(name, which)] and o.counts()[8:] == (0, 0)
    if which == "on-grid":
        assert o.on_plane_vertices > 50  # a whole grid plane of vertices lies in the plane, exactly


@pytest.mark.parametrize("which", PLANES)
@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_oracle_invariants(reflibs, name, which):
    s = mesh(reflibs, name)[4]
    o = clipped(reflibs, name, which)
    T = o.T.astype(np.int64)
    assert o.whole_triangles + o.cut_triangles + o.dropped_triangles + o.invalid_triangles == s.nT
    assert o.nT_out == int(o.outputs.sum()) and o.whole_triangles <= o.nT_out <= o.whole_triangles + 2 * o.cut_triangles
    assert T.shape == (o.nT_out, 3) and o.V.shape == (o.nV_out, 3) and o.N.shape == (o.nV_out, 3) and o.V.dtype == s.V.dtype
    assert np.all(T < o.nV_out)  # every index is below nV_out
    named = np.zeros(o.nV_out, bool)
    named[T.reshape(-1)] = True
    assert np.all(named)  # every output vertex is named
    # oMap is consistent with oT: a whole triangle, through the map, IS its output triangle; the kept rows are the input's
    at = np.cumsum(o.outputs) - o.outputs
    c = co.classes(co.signed(s.V, plane_of(s.V, which)))[s.T.astype(np.int64)]
    whole = (c == co.IN).any(axis=1) & ~(c == co.OUT).any(axis=1)
    assert np.array_equal(o.vmap[s.T[whole].astype(np.int64)], o.T[at[whole]])
    inside = o.vmap != co.NONE
    assert np.array_equal(o.vmap[inside], np.arange(o.kept_vertices)) and np.array_equal(inside, o.keep)
    assert np.array_equal(o.V[:o.kept_vertices].view(np.uint32), s.V[o.keep].view(np.uint32))
    assert np.array_equal(o.N[:o.kept_vertices].view(np.uint32), s.N[o.keep].view(np.uint32))
    # the new vertices lie on the plane up to the rounding of their rows, and in the order of their owners
    if o.cut_vertices:
        scale = np.abs(s.V).max() * 8.0 * np.finfo(np.float32).eps
        assert np.all(np.abs(co.signed(o.V[o.kept_vertices:], plane_of(s.V, which))) <= scale)
        word = o.owners[:, 0] * 4 + o.owners[:, 1]
        assert np.all(np.diff(word) > 0)
    # a manifold, oriented input stays manifold and oriented; no triangle without area is planted
    before = to.EdgeTable(s.T, s.nV)
    after = to.EdgeTable(o.T, o.nV_out)
    assert np.count_nonzero(after.nonmanifold) <= np.count_nonzero(before.nonmanifold)
    assert np.count_nonzero(after.misoriented) <= np.count_nonzero(before.misoriented)
    assert np.count_nonzero(after.degenerate) <= np.count_nonzero(before.degenerate) and after.invalid == 0
    if name in ("sphere", "blobs", "sheet"):
        assert not np.any(after.nonmanifold) and not np.any(after.misoriented) and not np.any(after.degenerate)
    if name == "sphere" and which in ("oblique", "on-grid"):  # a sphere cut by a plane: a cap with one rim
        assert to.loop_roots(after.lo[after.boundary], after.hi[after.boundary], o.nV_out).size == 1
    if which == "on-grid":  # no output triangle has two equal vertex rows
        P = o.V[T]
        assert not np.any((P[:, 0] == P[:, 1]).all(axis=1) | (P[:, 1] == P[:, 2]).all(axis=1) | (P[:, 2] == P[:, 0]).all(axis=1))


@pytest.mark.parametrize("name", ["sheet", "quant"])
def test_the_two_restatements_agree(reflibs, name):
    """the vectorised oracle against the loop that follows the walk word for word, on whole fixtures and every plane"""
    s = mesh(reflibs, name)[4]
    for which in PLANES:
        slow = co.clip_slow(s.V, s.N, s.T, plane_of(s.V, which), attributes(s.nV), MODES)
        assert co.same(clipped(reflibs, name, which), slow)


def test_oracle_definitions_on_a_tiny_mesh():
    """clip_cases.tiny_triangles: every in / on / out pattern in its three rotations, a cut edge used in both directions, a
    triangle with two equal indices, a NaN and an infinite vertex, an invalid triangle; the plane is z = 0.  The expected arrays
    were worked out by hand from the definition."""
    T = cc.tiny_triangles()
    words = np.arange(11, dtype=np.uint32) * 3 + 1
    for fn in (co.clip, co.clip_slow):
        o = fn(cc.TINY_V, cc.TINY_N, T, cc.PLANE_Z, (cc.TINY_A, words), (co.LERP_F32, co.COPY))
        assert o.counts() == (17, 29, 7, 10, 3, 7, 16, 8, 1, 2)
        assert o.vmap.tolist() == [0, 1, 2, 3, 4, 5, co.NONE, co.NONE, co.NONE, co.NONE, 6]
        # the new vertices in the order of their owners: (triangle 2, side 1), (2, 2), (6, 0), (6, 1), (18, 0), (18, 2), (27, 0), (29, 0), (29, 1), (30, 0)
        inf = float("inf")
        assert o.V.tolist() == [[0, 0, 1], [4, 0, 1], [0, 4, 3], [1, 1, 0], [5, 1, 0], [1, 5, -0.0], [7, 7, inf],
                                [3, 3, 0], [1, 3, 0], [1.5, 0.5, 0], [3, 3, 0], [3, 1, 0], [1.5, 2.5, 0], [1, 1, 0],
                                [0, 0, 1], [4, 0, 1], [7, 7, inf]]  # the last three: byte copies of the end that is in
        assert np.signbit(o.V[5, 2]) and not np.signbit(o.V[3, 2])
        r2, r10 = np.float32(np.sqrt(0.5)), np.sqrt(10.0)
        want_N = [[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, np.float32(0.6), np.float32(0.8)], [np.float32(0.6), 0, np.float32(0.8)], [0.25, 0.5, 0.75],
                  [0, 1, 0], [0, r2, r2], [0, np.float32(-1 / r10), np.float32(3 / r10)], [r2, -r2, 0], [0, r2, -r2], [np.float32(1 / r10), 0, np.float32(-3 / r10)],
                  [0, 0, 0],  # (N of 0 and 6 cancel: no direction)
                  [0, 0, 1], [0, 1, 0], [0.25, 0.5, 0.75]]
        assert o.N.tolist() == [[float(x) for x in row] for row in want_N]
        assert o.attrs[0].view(np.float32).tolist() == [1, 2, 3, 4, 5, 6, 12, 5.5, 5, 3.25, 6.5, 4.5, 6, 4, 1, 2, 12]
        assert o.attrs[1].tolist() == [1, 4, 7, 10, 13, 16, 31, 4, 1, 1, 7, 4, 7, 1, 1, 4, 31]
        assert o.T.tolist() == [[0, 1, 2], [0, 1, 5], [0, 1, 7], [0, 7, 8], [0, 4, 2], [0, 4, 5], [0, 4, 8], [0, 9, 10], [0, 10, 2], [0, 9, 5], [0, 9, 8],
                                [3, 1, 2], [3, 1, 5], [3, 1, 7], [3, 4, 2], [3, 10, 2], [11, 1, 2], [11, 2, 12], [11, 1, 5], [11, 1, 7], [4, 2, 12], [10, 2, 12],
                                [13, 0, 1], [13, 1, 11], [0, 13, 13], [0, 13, 0], [0, 14, 15], [0, 15, 1], [6, 16, 3]]
    # the other side of the same plane: what was in is out, the vertices on the plane stay on it
    n = co.clip(cc.TINY_V, cc.TINY_N, T, (0.0, 0.0, -1.0, 0.0))
    assert n.counts() == (14, 25, 6, 8, 3, 7, 15, 9, 1, 2) and n.vmap.tolist() == [co.NONE] * 3 + [0, 1, 2, 3, 4, 5] + [co.NONE] * 2
    # no triangles at all: everything is 0
    e = co.clip(cc.TINY_V, cc.TINY_N, np.zeros((0, 3), np.uint32), cc.PLANE_Z)
    assert e.counts() == (0,) * 10 and np.all(e.vmap == co.NONE)


def test_made_up_meshes_are_what_they_claim():
    V, N, T, kinds = cc.runs(4)
    o = co.clip(V, N, T, cc.PLANE_Z)
    assert (o.cut_triangles, o.whole_triangles, o.dropped_triangles) == tuple(int(np.count_nonzero(kinds == k)) for k in range(3))
    assert o.cut_triangles == sum(cc.RUNS) and np.array_equal(o.outputs > 0, kinds != 2)
    V, N, T, first = cc.shared_edge(5)
    o = co.clip(V, N, T, cc.PLANE_Z)
    row = np.nonzero((o.edges == [0, 1]).all(axis=1))[0]
    assert row.size == 1 and o.owners[row[0], 0] == first and first >= 3000
    uses = np.nonzero(((T == 0).any(axis=1)) & ((T == 1).any(axis=1)))[0]
    assert uses.size == 5000 and uses.min() == first and o.V[o.kept_vertices + row[0]].tolist() == [0.5, 0.0, 0.0]
    Vt, Nt, Tt, At = cc.tiny_repeated(400)
    o = co.clip(Vt, Nt, Tt, cc.PLANE_Z, (At,), (co.LERP_F32,))
    assert o.counts() == tuple(400 * x for x in (17, 29, 7, 10, 3, 7, 16, 8, 1, 2)) and Tt.shape[0] > 8 * 1024


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_clip_surface\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_clipping;", hip)
    assert re.search(r"#define MC33HIP_CLIP_COPY 0\b", hip) and re.search(r"#define MC33HIP_CLIP_LERP_F32 1\b", hip)
    assert re.search(r"\bsurface \*MC33_calculate_clipped_isosurface\(MC33 \*", pub) and re.search(r"\} mc33_clip;", pub)
    assert re.search(r"\bint MC33_clip_box\(const double lo\[3\], const double hi\[3\], mc33_clip \*", pub)
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)
    from mc33_c_library_amd import DeviceGrid, clip_box
    assert callable(DeviceGrid.clip) and callable(DeviceGrid.extract_clipped) and callable(clip_box)
    from mc33_c_library_amd import build
    assert "mc33_clip.hip.h" in build.HIP_HEADERS
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert '#include "mc33_simplify.hip.h"\n#include "mc33_clip.hip.h"\n' in kernels and "k_clip_tri" in kernels  # (behind the parts it builds on)
    assert " mc33_clip.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_clipping_kernels_are_in_the_code_object(dtype):
    real = "double" if dtype == "f64" else "float"
    assert_kernels(dtype, KERNELS + ["k_clip_class<%s>" % real, "k_clip_rows<%s>" % real, "k_clip_new<%s>" % real])


def test_clip_box_is_exact_and_refuses_bad_bounds():
    """host C of the product library; no GPU is touched"""
    from mc33_c_library_amd import load_library
    L = load_library("f32")
    three = C.c_double * 3

    def box(lo, hi, out):
        return L.MC33_clip_box(C.byref(three(*lo)), C.byref(three(*hi)), C.byref(out))
    out = SurfaceClip()
    lo, hi = (0.1, -2.5, 1e-300), (0.30000000000000004, 7.0, 1e300)
    assert box(lo, hi, out) == 0 and out.n == 6
    got = [[out.plane[k][j] for j in range(4)] for k in range(6)]
    assert got == [[1, 0, 0, -lo[0]], [-1, 0, 0, hi[0]], [0, 1, 0, -lo[1]], [0, -1, 0, hi[1]], [0, 0, 1, -lo[2]], [0, 0, -1, hi[2]]]
    inf, nan = float("inf"), float("nan")
    bad = [((0, 0, 0), (1, 1, 0)), ((0, 2, 0), (1, 1, 1)), ((0, 0, 0), (inf, 1, 1)), ((-inf, 0, 0), (1, 1, 1)), ((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, nan, 1))]
    for lo, hi in bad:
        canary = SurfaceClip()
        canary.n = 77
        canary.plane[5][3] = 42.0
        assert box(lo, hi, canary) == -1 and canary.n == 77 and canary.plane[5][3] == 42.0, (lo, hi)
    assert L.MC33_clip_box(None, C.byref(three(1, 1, 1)), C.byref(out)) == -1 and L.MC33_clip_box(C.byref(three(0, 0, 0)), C.byref(three(1, 1, 1)), None) == -1
    from mc33_c_library_amd import clip_box
    assert clip_box((0.0, 0.0, 0.0), (1.0, 2.0, 3.0)) == [(1, 0, 0, 0), (-1, 0, 0, 1), (0, 1, 0, 0), (0, -1, 0, 2), (0, 0, 1, 0), (0, 0, -1, 3)]
    with pytest.raises(ValueError):
        clip_box((0.0, 0.0, 0.0), (1.0, 0.0, 1.0))


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_clip(dtype):
    """mc33_capi.c linked with the emulated device layer, which cannot clip: the library still loads (a weak reference),
    MC33_calculate_clipped_isosurface returns NULL and leaves the object alone - for good arguments and, which needs no device
    in any build, for a null struct, too many planes and every refused plane -, MC33_clip_box works, and the object extracts as
    before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        L.free_surface_memory(S)
        three = C.c_double * 3
        boxed = SurfaceClip()
        assert L.MC33_clip_box(C.byref(three(1, 1, 1)), C.byref(three(9, 9, 9)), C.byref(boxed)) == 0 and boxed.n == 6
        inf, nan = float("inf"), float("nan")
        cases = [boxed, SurfaceClip(0), SurfaceClip(7)]
        for pl in ((1, 0, 0, -5), (0, 0, 0, 1), (nan, 0, 1, 0), (1, inf, 0, 0), (1, 0, 0, -inf)):
            one = SurfaceClip(1)
            for j in range(4):
                one.plane[0][j] = pl[j]
            cases.append(one)
        for cl in cases:
            assert not L.MC33_calculate_clipped_isosurface(M, lib.real(iso + 1), C.byref(cl))
            assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        assert not L.MC33_calculate_clipped_isosurface(M, lib.real(iso + 1), None)
        assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
