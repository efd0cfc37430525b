"""The distance between surfaces, the part that needs no GPU: the numpy oracle against cases computed by hand, the
conditions on the made-up fixtures that tests/test_gpu_distance.py relies on - a fixture that stops exercising a path fails here -,
the new names in the headers, the libraries and the code objects, the place of the new part in the translation unit, and the
host-logic build of mc33_capi.c, whose emulated device layer has no distance.

The oracle and fixture tests test tests/distance_oracle.py and tests/distance_cases.py, not the product, and pass without the
feature.  The product is held to that oracle by the name, struct, export, code-object and host-logic tests below - these fail
without the feature - and, on the device, by tests/test_gpu_distance.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distance_cases as dc
import distance_oracle as do
import measure_oracle as mo
from mc33_c_library_amd.api import SurfaceDistance, SurfaceSimplification
from mesh_checks import assert_exported, assert_kernels, host_logic, launched, reference_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_surface_distance", "mc33hip_distance_timing"]
C_NAMES = ["MC33_isosurface_distance", "MC33_simplification_error"]
KERNELS = ["k_dist_arg", "k_dist_sum"] + launched("k_mesh_tile_sum<MeshCount>", "k_mesh_scan_top", "k_mesh_place<MeshCount, 2>")
MAX_VGPRS = 168  # the closest-point walk in doubles: three waves per SIMD (512 / 3, in granules of 8) - three blocks of 256 per CU


# ---- the oracle against hand-computed cases ----------------------------------------------------------------------------------------

A, B, Cc = (0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0)
# point -> region, closest point, squared distance: the triangle (0,0,0) (4,0,0) (0,4,0), integer coordinates, exact in binary
BY_HAND = [((-1.0, -2.0, 3.0), "a", (0.0, 0.0, 0.0), 14.0),
           ((6.0, -1.0, 0.0), "b", (4.0, 0.0, 0.0), 5.0),
           ((2.0, -3.0, 1.0), "ab", (2.0, 0.0, 0.0), 10.0),
           ((-1.0, 7.0, 2.0), "c", (0.0, 4.0, 0.0), 14.0),
           ((-2.0, 1.0, 0.0), "ac", (0.0, 1.0, 0.0), 4.0),
           ((4.0, 4.0, 0.0), "bc", (2.0, 2.0, 0.0), 8.0),
           ((1.0, 1.0, -5.0), "face", (1.0, 1.0, 0.0), 25.0)]


def test_oracle_by_hand_in_every_region():
    V, T = np.array([A, B, Cc], np.float32), np.array([[0, 1, 2]], np.uint32)
    P = np.array([p for p, _, _, _ in BY_HAND], np.float32)
    r = do.distance(P, V, T, signed=True)
    assert [do.REGIONS[k] for k in r.region] == [name for _, name, _, _ in BY_HAND]
    assert r.q.tolist() == [list(q) for _, _, q, _ in BY_HAND] and r.D2.tolist() == [d2 for _, _, _, d2 in BY_HAND]
    assert r.tri.tolist() == [0] * 7 and r.counts() == (7, 0, 0, 0)
    # ab x ac = (0, 0, 16): the sign of e.z, positive where e.z == 0
    assert r.negative.tolist() == [False, False, False, False, False, False, True]
    assert r.dist.tolist() == [np.float32(np.sqrt(d2)) * (-1 if k == 6 else 1) for k, (_, _, _, d2) in enumerate(BY_HAND)]
    assert (r.max, r.min, r.argmax, r.argmin) == (5.0, 2.0, 6, 4)
    assert do.distance(P, V, T).dist[6] == 5.0  # unsigned


def test_oracle_ties_clamp_and_unusable_triangles():
    # two copies of one triangle and a third, nearer to nothing: the smallest index wins
    V = np.array([A, B, Cc, (0, 0, 9), (4, 0, 9), (0, 4, 9)], np.float32)
    T = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2], [0, 1, 7]], np.uint32)
    P = np.array([[1, 1, 1], [1, 1, 8.5], [1, 1, 4.5], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    r = do.distance(P, V, T)
    assert r.tri.tolist() == [1, 0, 0, do.NONE, do.NONE] and r.counts() == (3, 2, 1, 0)  # (4.5: equally far from both planes)
    assert np.isinf(r.dist[3:]).all() and np.isnan(r.point[3:]).all() and r.D2[:3].tolist() == [1.0, 0.25, 20.25]
    # a corner that is not finite: counted, never a winner; nothing usable: nobody is matched
    V2 = V.copy()
    V2[1, 1] = np.inf
    r = do.distance(P, V2, T)
    assert r.counts() == (3, 2, 1, 2) and r.tri.tolist()[:3] == [0, 0, 0]
    r = do.distance(P, V2, T[1:])
    assert r.counts() == (0, 5, 1, 2) and (r.max, r.min, r.argmax) == (0.0, 0.0, 0)
    # a single-point and a collinear triangle: q is a corner or on the segment, never NaN
    V3 = np.array([(1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 0, 0), (6, 0, 0)], np.float32)
    r = do.distance(np.array([[1, 2, 1], [3, 1, 0], [9, 0, 0]], np.float32), V3, np.array([[0, 1, 2], [3, 4, 5]], np.uint32))
    assert r.tri.tolist() == [0, 1, 1] and r.D2.tolist() == [1.0, 1.0, 9.0] and not np.isnan(r.q).any()


# ---- the conditions on the fixtures that the GPU tests rely on -----------------------------------------------------------------------

def test_ladder_reaches_every_region():
    seen = set()
    for nT in dc.LADDER_TRIANGLES:
        P, V, T = dc.ladder(dc.LADDER_POINTS[-1], nT)
        assert P.shape[0] * T.shape[0] <= 2e7
        seen |= set(np.unique(do.distance(P, V, T).region).tolist())
    assert seen == set(range(7))


def test_tie_fixtures_hold_ties():
    P, V, T = dc.sheet()
    r = do.distance(P, V, T)
    assert np.all(r.D2 == 9.0) and r.counts() == (P.shape[0], 0, 0, 0)
    # how many triangles are at exactly the winning distance: up to six above a vertex, two above an edge, one above a face
    a, b, c = (V[T[:, k].astype(np.int64)].astype(np.float64)[None] for k in range(3))
    q, _ = do.closest(P.astype(np.float64)[:, None, :], a, b, c)
    ties = np.count_nonzero(((P.astype(np.float64)[:, None, :] - q) ** 2).sum(axis=2) == 9.0, axis=1)
    assert set(np.unique(ties).tolist()) >= {1, 2, 6}
    P, V, T = dc.two_equidistant()
    assert np.all(do.distance(P, V, T).tri == 0) and np.all(do.distance(P, V, T[::-1]).tri == 0)
    P, V, T = dc.doubled()
    r = do.distance(P, V, T)
    assert np.all(r.tri < T.shape[0] // 2)
    perm = np.random.default_rng(1).permutation(T.shape[0])
    r2 = do.distance(P, V, T[perm])
    assert np.array_equal(r2.D2, r.D2) and not np.array_equal(r2.tri, r.tri) and np.any(r2.tri >= T.shape[0] // 2)


def test_far_crowded_spanning_and_hostile_fixtures():
    P, V, T = dc.far_and_edge()
    r = do.distance(P, V, T)
    ext = (V.max(axis=0) - V.min(axis=0)).max()
    assert r.max > 900 * ext and r.counts() == (P.shape[0], 0, 0, 0)
    P, V, T = dc.far_from_the_origin()
    assert V.min() > 4095 and np.unique(do.distance(P, V, T).tri).size > 100
    P, V, T = dc.crowded()
    r = do.distance(P, V, T)
    assert np.count_nonzero(r.tri < 5000) > 250 and np.count_nonzero(r.tri >= 5000) > 100
    P, V, T = dc.spanning()
    r = do.distance(P, V, T)
    assert np.all(r.tri[:200] == T.shape[0] - 1) and np.all(r.region[:200] == 6) and np.count_nonzero(r.tri[200:] != T.shape[0] - 1) > 100
    P, V, T, bad, wild = dc.hostile()
    r = do.distance(P, V, T)
    assert r.counts() == (400, wild, 0, bad.size) and bad.size == 6 and not np.isin(r.tri, bad).any()
    corners = V[T.astype(np.int64)].astype(np.float64)
    single = np.nonzero(np.ptp(corners, axis=1).max(axis=1) == 0)[0]
    n = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    flat = np.setdiff1d(np.nonzero(np.abs(n).max(axis=1) < 1e-7)[0], single)
    assert single.size == 40 and flat.size >= 40  # single points and collinear triangles do win
    assert np.count_nonzero(np.isin(r.tri, single)) >= 30 and np.count_nonzero(np.isin(r.tri, flat)) >= 30
    P, V, T = dc.all_unusable()
    assert do.distance(P, V, T).counts() == (0, P.shape[0], 1, 2)


def test_pushed_sphere_has_both_signs(reflibs):
    data, r0, d, iso, s = reference_mesh(reflibs, "sphere")
    P, side = dc.pushed(s.V[::41], s.N[::41], d)
    r = do.distance(P, s.V, s.T, signed=True)
    neg = np.count_nonzero(r.negative)
    assert 100 < neg < P.shape[0] - 100 and np.all(r.matched)
    # the push decides the side (the reference's normals point one way all over the sphere)
    agree = np.count_nonzero(r.negative == (side < 0))
    assert agree in (0, P.shape[0]), agree


@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_fixture_vertices_lie_on_their_own_triangles(reflibs, name):
    """every referenced vertex has an incident triangle at D2 == 0 exactly - as corner a or b by the walk's first two tests, as
    corner c unless a sliver's rounding takes an earlier branch: the GPU test asks for +0.0 at exactly these vertices"""
    data, r0, d, iso, s = reference_mesh(reflibs, name)
    zero, first = do.own_vertices(s.V, s.T)
    named = np.zeros(s.nV, bool)
    named[s.T.reshape(-1).astype(np.int64)] = True
    assert np.array_equal(zero, named) and np.count_nonzero(named) == s.nV - mo.FIXTURES[name][2][3]
    assert np.all(first[zero] < s.nT)


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_surface_distance\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_distance;", hip)
    assert "only as good" in hip and "MC33_HIP_DISTANCE_CELLS" in hip
    assert re.search(r"\bint MC33_isosurface_distance\(MC33 \*", pub) and re.search(r"\bint MC33_simplification_error\(MC33 \*", pub)
    assert re.search(r"\} mc33_distance;", pub)
    import mc33_c_library_amd as pkg
    assert set(HIP_NAMES) <= set(pkg.HIP_API) and set(C_NAMES) <= set(pkg.REFERENCE_API)
    assert pkg.Distance and pkg.SurfaceDistance
    G = pkg.DeviceGrid
    assert callable(G.distance) and callable(G.surface_distance) and "vertices only" in G.surface_distance.__doc__.lower()
    import inspect
    for f in (G.extract_simplified, G.extract_smoothed):
        assert inspect.signature(f).parameters["error"].default is False


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_distance_kernels_are_in_the_code_object(dtype):
    real = "double" if dtype == "f64" else "float"
    ks = assert_kernels(dtype, KERNELS)
    ks = assert_kernels(dtype, ["k_dist_bounds<%s>" % real, "k_dist_bin<%s, false>" % real, "k_dist_bin<%s, true>" % real, "k_dist_query<%s>" % real], MAX_VGPRS)
    print({n: (k["vgpr_count"], k.get("group_segment_fixed_size")) for n, k in ks.items() if "k_dist" in n})


def test_the_part_is_built_and_included_behind_the_renderer():
    from mc33_c_library_amd import build
    assert "mc33_distance.hip.h" in build.HIP_HEADERS
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert '#include "mc33_render.hip.h"\n#include "mc33_distance.hip.h"\n#include "mc33_simplify.hip.h"\n' in kernels and "k_dist_query" in kernels
    assert kernels.index('#include "mc33_mesh.hip.h"') < kernels.index('#include "mc33_distance.hip.h"')
    mk = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()
    assert "mc33_distance.hip.h" in mk
    context = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_context.hip.h")).read()
    assert "distance_cells_switch()" in context  # the knob is read where the renderer's is: when a context is created


def test_documents_name_the_part():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 25\.", design, re.M) and "profiles/distance_timing.txt" in design and "mc33_distance.hip.h" in open(os.path.join(ROOT, "README.md")).read()
    assert "MC33_isosurface_distance" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_the_distance_calls(dtype):
    """mc33_capi.c linked with the emulated device layer, which has no mc33hip_surface_distance: the library still loads (a weak
    reference), both calls return -1 and leave the object alone, and the object extracts as before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        L.free_surface_memory(S)
        out = (SurfaceDistance * 2)()
        sm = SurfaceSimplification((C.c_double * 3)(2, 2, 2), 0, 1)
        assert L.MC33_isosurface_distance(M, lib.real(iso + 1), lib.real(iso), out) == -1
        assert L.MC33_isosurface_distance(M, lib.real(iso + 1), lib.real(iso), None) == -1
        assert L.MC33_simplification_error(M, lib.real(iso + 1), C.byref(sm), out) == -1
        assert L.MC33_simplification_error(M, lib.real(iso + 1), None, out) == -1
        assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
