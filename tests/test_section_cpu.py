"""Sections of extracted surfaces by planes, the part that needs no GPU: the numpy oracle on the unmodified
reference's meshes - its two restatements against each other, against the clip oracle and against the topology oracle of the
clipped mesh -, a tiny mesh whose result is written out, the sign and the size of the sphere's area, the new names in the headers,
the libraries and the code objects, and the host-logic build of mc33_capi.c, whose emulated device layer cannot section.

The oracle tests test tests/section_oracle.py and the fixtures, not the product, and pass without the feature.  The product is held
to that oracle by the name, struct, export, code-object and host-logic tests below - these fail without the feature - and, on the
device, by tests/test_gpu_section.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import clip_oracle as co
import measure_oracle as mo
import section_cases as sc
import section_oracle as so
import topology_oracle as to
from clip_cases import MODES, PLANES, attributes, clipped, plane_of
from mesh_checks import assert_exported, assert_kernels, host_logic, launched, reference_mesh as mesh
from section_cases import ORIGIN, sectioned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_section_surface", "mc33hip_section_contours", "mc33hip_section_ladder"]
C_NAMES = ["MC33_section_isosurface", "MC33_free_section", "MC33_section_contours", "MC33_section_profile"]
KERNELS = ["k_section_tri", "k_section_init", "k_section_emit", "k_section_points", "k_section_count", "k_section_finish", "k_section_table_degree",
           "k_section_table_points", "k_section_table_roots", "k_mesh_scan_top3", "k_clip_tri", "k_clip_own"] + \
    launched("k_mesh_clear", "k_mesh_tile_sum<MeshFlag>", "k_mesh_tile_sum<ClipOwned>", "k_mesh_scan_top", "k_mesh_place<MeshFlag, 0>", "k_mesh_place<MeshFlag, 1>")
TEMPLATED = ["k_section_rows", "k_section_new", "k_section_sums", "k_section_table_segments", "k_section_ladder", "k_clip_class"]
@pytest.mark.parametrize("which", PLANES)
@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_the_two_restatements_agree_and_the_cut_points_are_clips(reflibs, name, which):
    s = mesh(reflibs, name)[4]
    o = sectioned(reflibs, name, which)
    slow = so.section_slow(s.V, s.T, plane_of(s.V, which), attributes(s.nV), MODES, ORIGIN)
    assert so.same(o, slow)
    cl = clipped(reflibs, name, which)
    assert o.cut_points == cl.cut_vertices and o.crossing_triangles == cl.cut_triangles and np.array_equal(o.edges, cl.edges)
    assert np.array_equal(so.bits(o.P[o.on_points:]), so.bits(cl.V[cl.kept_vertices:]))
    for x, w in zip(o.attrs, cl.attrs):
        assert np.array_equal(x[o.on_points:], w[cl.kept_vertices:])
    # an ON point is its vertex; the map is the inverse of the first on_points rows
    at = np.nonzero(o.pmap != so.NONE)[0]
    assert np.array_equal(o.pmap[at], np.arange(o.on_points)) and np.array_equal(so.bits(o.P[:o.on_points]), so.bits(s.V[at]))
    assert o.on_points <= cl.on_plane_vertices and (o.invalid_triangles, o.nonfinite_vertices, o.degenerate_segments, o.isolated_points) == (0, 0, 0, 0)
    if which in ("miss", "all"):
        assert o.counts() == (0,) * 13 and o.length == 0.0 and o.area == 0.0
    else:
        assert o.nS_out > 200 and np.all(o.label <= np.arange(o.nP_out)) and np.all(o.S < o.nP_out)
    # every segment lies in the plane up to the rounding of its rows
    if o.nS_out:
        scale = np.abs(s.V).max() * 8.0 * np.finfo(np.float32).eps
        assert np.all(np.abs(co.signed(o.P, plane_of(s.V, which))) <= scale)


@pytest.mark.parametrize("name", ["sphere", "blobs"])
def test_a_closed_surface_gives_closed_contours_the_boundary_of_the_clipped_mesh(reflibs, name):
    """an oblique plane that meets no vertex exactly: the segments are the boundary edges clip opens, the contours its loops"""
    assert mo.FIXTURES[name][2][4] == 0  # no open edge
    o = sectioned(reflibs, name, "oblique")
    cl = clipped(reflibs, name, "oblique")
    assert o.on_points == 0 and cl.on_plane_vertices == 0
    et = to.EdgeTable(cl.T, cl.nV_out)
    blo, bhi = et.lo[et.boundary], et.hi[et.boundary]
    assert o.nS_out == blo.size > 100
    assert o.contours == to.loop_roots(blo, bhi, cl.nV_out).size and o.closed_contours == o.contours and o.open_ends == 0 and o.branch_points == 0
    # the very edges: a point of the section is vertex kept_vertices + r of the clipped mesh
    S = o.S.astype(np.int64) + cl.kept_vertices
    mine = np.unique((np.minimum(S[:, 0], S[:, 1]) << 32) | np.maximum(S[:, 0], S[:, 1]))
    assert np.array_equal(mine, np.unique((blo << 32) | bhi))
    # next walks every loop: following it from a root comes back after as many steps as the loop has points
    nxt = o.next.astype(np.int64)
    for r in np.unique(o.label).tolist():
        n, p = 0, r
        while True:
            p, n = int(nxt[p]), n + 1
            if p == r:
                break
        assert n == np.count_nonzero(o.label == r)


@pytest.mark.parametrize("which", ["oblique", "on-grid"])
@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_contour_rows_add_up_to_the_totals(reflibs, name, which):
    o = sectioned(reflibs, name, which)
    rows = so.contour_table(o)
    assert len(rows) == o.contours and [r[0] for r in rows] == sorted(r[0] for r in rows)
    assert sum(r[1] for r in rows) == o.nP_out - o.isolated_points and sum(r[2] for r in rows) == o.nS_out
    assert sum(r[3] for r in rows) == o.open_ends and sum(r[4] for r in rows) == o.branch_points and sum(r[5] for r in rows) == o.closed_contours
    assert abs(math.fsum(r[6] for r in rows) - o.length) <= 4 * mo.U * o.length * len(rows)
    G = [math.fsum(r[7][k] for r in rows) for k in range(3)]
    assert np.allclose(G, o.area_vector, rtol=0, atol=mo.sum_bound(o.terms[:, 1:].ravel()))


def test_oracle_definitions_on_a_tiny_mesh():
    """section_cases.tiny_triangles, the plane z = 0.  The expected arrays were worked out from the definition: the ON vertices 3,
    4, 5 are points 0, 1, 2; the cut points follow in clip's owner order ((2, 1), (2, 2), (6, 0), (6, 1), (18, 0), (18, 2),
    (27, 0), (29, 0), (29, 1), (30, 0)); triangle 2 = (0, 1, 8), polygon 0, 1, c{1, 8}, c{0, 8}, gives 3 -> 4; triangle 4 =
    (0, 4, 5), polygon 0, 4, 5, gives 1 -> 2; triangle 5 = (0, 4, 8), polygon 0, 4, c{0, 8}, gives 1 -> 4; and so on."""
    T = sc.tiny_triangles()
    none = so.NONE
    inf = float("inf")
    for fn in (so.section, so.section_slow):
        o = fn(sc.TINY_V, T, sc.PLANE_Z, (sc.TINY_A, sc.TINY_WORDS), (co.LERP_F32, co.COPY))
        # nP, nS, on, cut, isolated, degenerate ((0, 6, 0), (3, 3, 0) in its rotations), crossing, invalid, nonfinite, contours,
        # closed, open ends, branch points
        assert o.counts() == (13, 19, 3, 10, 0, 4, 16, 1, 2, 2, 0, 12, 9)
        assert o.S.tolist() == [[3, 4], [1, 2], [1, 4], [5, 6], [5, 2], [5, 4], [2, 0], [3, 0], [0, 1], [0, 6], [8, 7], [2, 7], [3, 7], [8, 1], [8, 6], [7, 9],
                                [10, 11], [12, 0], [1, 0]]
        assert o.P.tolist() == [[1, 1, 0], [5, 1, 0], [1, 5, -0.0], [3, 3, 0], [1, 3, 0], [1.5, 0.5, 0], [3, 3, 0], [3, 1, 0], [1.5, 2.5, 0], [1, 1, 0],
                                [0, 0, 1], [4, 0, 1], [7, 7, inf]]  # the last three: byte copies of the end that is in
        assert np.signbit(o.P[2, 2]) and not np.signbit(o.P[0, 2])
        assert o.label.tolist() == [0] * 10 + [10, 10, 0]
        assert o.next.tolist() == [none] * 7 + [9, none, none, 11, none, 0]
        assert o.pmap.tolist() == [none, none, none, 0, 1, 2] + [none] * 5
        assert o.attrs[0].view(np.float32).tolist() == [4, 5, 6, 5.5, 5, 3.25, 6.5, 4.5, 6, 4, 1, 2, 12]
        assert o.attrs[1].tolist() == [10, 13, 16, 4, 1, 1, 7, 4, 7, 1, 1, 4, 31]
        assert o.per_triangle.sum() == 19 and not o.per_triangle[[0, 1, 3, 28, 32, 33, 34, 35]].any() and o.per_triangle[36]
    # without the two vertices that are not finite: lengths by hand - 3 -> 4 is (3, 3, 0) -> (1, 3, 0)
    o = so.section(sc.TINY_V, T[:27], sc.PLANE_Z)
    assert o.terms[0].tolist() == [2.0, 0.0, 0.0, 0.5 * (3 * 3 - 3 * 1)] and o.nS_out == 15 and math.isfinite(o.length)
    # the other side of the same plane: what was in is out, the vertices on the plane stay on it
    n = so.section(sc.TINY_V, T[:27], (0.0, 0.0, -1.0, 0.0))
    assert n.nS_out == 15 and n.on_points == 3 and n.cut_points == o.cut_points == 6  # ({0, 7}, {1, 6}, {1, 8}, {2, 7}, {2, 6}, {0, 8})
    # no triangles at all: everything is 0
    e = so.section(sc.TINY_V, np.zeros((0, 3), np.uint32), sc.PLANE_Z)
    assert e.counts() == (0,) * 13 and np.all(e.pmap == none)


AREA_SIGN = "area is SIGNED"
SPHERE_MARGIN = 1.0e-3  # relative; see test_the_sphere


def test_the_sphere(reflibs):
    """The reference's sphere (r = 1 about (2, 2, 2), samples growing outwards): its stored winding makes the volume negative,
    and the area of a section has the sign of the volume - what both headers state.  |area| against pi (r^2 - h^2), h the
    distance of the plane from the centre: the contour is a polygon inscribed in the circle up to the error of linear
    interpolation on a grid of step 0.03, which makes it too small.  MEASURED on the reference-extracted mesh (this test prints
    the figures): oblique plane through the centre 3.1401355 against 3.1415927, relative -4.6e-4; the grid plane x = x0
    3.0954479 against pi (1 - h^2) = 3.0963537, relative -2.9e-4; both of the order step^2 / 2 = 4.5e-4.  The margin is 1e-3, twice the
    larger."""
    data, r0, d, iso, s = mesh(reflibs, "sphere")
    m = mo.measure(s.V, s.T, r0, d, data.shape)
    assert m.volume < 0.0
    for which in ("oblique", "on-grid"):
        pl = plane_of(s.V, which)
        o = sectioned(reflibs, "sphere", which)
        assert o.contours == 1 and o.closed_contours == 1
        assert o.area < 0.0  # the sign of the volume
        h = abs((pl[0] * 2.0 + pl[1] * 2.0 + pl[2] * 2.0) + pl[3]) / math.sqrt(pl[0] ** 2 + pl[1] ** 2 + pl[2] ** 2)
        want = math.pi * (1.0 - h * h)
        print("sphere %s: area %.9g, pi (r^2 - h^2) %.9g, relative %.3g" % (which, o.area, want, (abs(o.area) - want) / want))
        assert abs(abs(o.area) - want) <= SPHERE_MARGIN * want
        # the other side of the plane: every segment and the normal turn round, the area stays - up to the segments on the plane
        # itself, which belong to one side only
        other = so.section(s.V, s.T, tuple(-x for x in pl), origin=ORIGIN)
        print("  the other side: area %.9g" % other.area)
        assert other.area < 0.0 and abs(other.area - o.area) <= (64 * mo.sum_bound(o.terms[:, 1:].ravel()) if which == "oblique" else 0.02 * abs(o.area))
        # the reference point does not matter for a closed contour, up to rounding
        far = so.section(s.V, s.T, pl, origin=(-7.0, 11.0, 3.0))
        assert abs(far.area - o.area) <= 64 * mo.sum_bound(far.terms[:, 1:].ravel())
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    for text in (hip, pub):
        flat = re.sub(r"[\s*]+", " ", text)
        assert AREA_SIGN in flat and "area has the sign of the volume" in flat


def test_the_ladder_oracle_is_the_single_plane_oracle(reflibs):
    s = mesh(reflibs, "sheet")[4]
    normal = (0.0, 0.0, 1.0)
    ws = sc.ladder_offsets(s.V, normal, 7)
    assert all(b > a for a, b in zip(ws, ws[1:]))
    rungs = so.ladder(s.V, s.T, normal, ws, ORIGIN)
    assert rungs[0].nS_out == 0 and rungs[-1].nS_out == 0 and rungs[3].nS_out > 100
    for w, r in zip(ws, rungs):
        full = so.section(s.V, s.T, normal + (w,), origin=ORIGIN)
        assert (r.nS_out, r.degenerate_segments) == (full.nS_out, full.degenerate_segments)
        assert np.array_equal(np.sort(so.bits(r.terms), axis=0), np.sort(so.bits(full.terms), axis=0))


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_section_surface\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_section;", hip) and re.search(r"\} mc33hip_contour;", hip)
    assert re.search(r"\bint mc33hip_section_contours\(mc33hip_ctx \*", hip) and re.search(r"\bint mc33hip_section_ladder\(mc33hip_ctx \*", hip)
    assert re.search(r"\bmc33_section \*MC33_section_isosurface\(MC33 \*", pub) and re.search(r"\bvoid MC33_free_section\(mc33_section \*", pub)
    assert re.search(r"\bint MC33_section_contours\(MC33 \*", pub) and re.search(r"\bint MC33_section_profile\(MC33 \*", pub)
    assert re.search(r"\} mc33_section;", pub) and re.search(r"\} mc33_contour;", pub) and re.search(r"\} mc33_section_level;", pub)
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)
    from mc33_c_library_amd import DeviceGrid
    for n in ("section", "section_contours", "section_ladder", "extract_section", "section_profile"):
        assert callable(getattr(DeviceGrid, n))
    from mc33_c_library_amd import build
    assert "mc33_section.hip.h" in build.HIP_HEADERS
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    # behind the parts it builds on - mesh, measure, clip; the file still ends with the spectrum, which tests/test_spectrum_cpu.py pins
    assert '#include "mc33_simplify.hip.h"\n#include "mc33_clip.hip.h"\n#include "mc33_section.hip.h"\n#include "mc33_resample.hip.h"\n' in kernels
    assert "k_section_" in kernels
    assert " mc33_section.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_section_kernels_are_in_the_code_object(dtype):
    real = "double" if dtype == "f64" else "float"
    assert_kernels(dtype, KERNELS + ["%s<%s>" % (k, real) for k in TEMPLATED])  # no scratch, no spill, at most 64 registers


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_section(dtype):
    """mc33_capi.c linked with the emulated device layer, which cannot section: the library still loads (weak references), the
    three calls refuse - NULL, -1 - and leave the object alone, for good arguments and for refused ones, and the object extracts
    as before."""
    from mc33_c_library_amd.api import Contour, SectionLevel
    with host_logic(dtype) as h:
        lib, M, iso = h.lib, h.M, h.iso
        L = lib.lib
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        L.free_surface_memory(S)
        four, three = C.c_double * 4, C.c_double * 3
        nan = float("nan")
        table, n = (Contour * 4)(), C.c_uint(77)
        levels = (SectionLevel * 2)()
        ws = (C.c_double * 2)(-10.0, -9.0)
        for pl in ((1, 0, 0, -5), (0, 0, 0, 1), (nan, 0, 1, 0)):
            assert not L.MC33_section_isosurface(M, lib.real(iso + 1), C.byref(four(*pl)))
            assert L.MC33_section_contours(M, lib.real(iso + 1), C.byref(four(*pl)), table, 4, C.byref(n)) == -1
            assert L.MC33_section_profile(M, lib.real(iso + 1), C.byref(three(*pl[:3])), ws, 2, levels) == -1
            assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        assert not L.MC33_section_isosurface(M, lib.real(iso + 1), None) and not L.MC33_section_isosurface(None, lib.real(iso), C.byref(four(1, 0, 0, 0)))
        L.MC33_free_section(None)  # as free() takes it
        assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
