"""Caps at the grid faces, the part that needs no GPU: the numpy oracle on the surfaces of the CPU extractor held to
facts it does not compute itself - the topology oracle, an area of the solid region of every face from the samples, the closed-
surface identities of the measures -, the new names in the headers, the libraries and the code objects, and the host-logic build of
mc33_capi.c, whose emulated device layer cannot cap.

The tests over cap_cases pin tests/cap_oracle.py and the fixtures and pass without the feature.  The product is held to that
oracle by the name, struct, export, code-object and host-logic tests below - these fail without the feature - and, on the device,
by tests/test_gpu_cap.py.

Two things the cases settle differently from what one might expect.  (1) The extractor leaves no hole around a NaN sample: it puts
vertices with NaN coordinates on the grid edges of that sample.  The `hole` case therefore drops the triangles that name such a
vertex (cap_cases.without_nonfinite), which is what a caller does with them, and that hole's rim lies on no face.  (2) The solid
side is the side the winding turns its back on, so a capped surface is wound outwards from its solid in every flavour and with
invert: its signed volume is positive both times, and the two add up to the volume of the box."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cap_cases as cc
import cap_oracle as co
import measure_oracle as mo
import topology_oracle as to
from mc33_c_library_amd.api import SurfaceCap, SurfaceCapInfo
from mesh_checks import assert_exported, assert_kernels, host_logic, launched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_cap_surface"]
C_NAMES = ["MC33_calculate_capped_isosurface"]
# (the tile scans over what this part counts are instances of its own of the shared kernels)
KERNELS = ["k_cap_sides", "k_cap_invert", "k_mesh_tile_sum<CapTris>", "k_mesh_tile_sum<CapNamed>", "k_mesh_place<CapTris, 0>", "k_mesh_place<CapNamed, 1>"] + \
          launched("k_mesh_clear", "k_mesh_scan_top")
ALL = cc.ALL
CLOSED = tuple(n for n in ALL if n not in cc.OPEN)

_results = {}


def capped(oracles, name, invert=False):
    """(case, the extractor's surface, the oracle's result), computed once per case, shared and left unchanged"""
    key = (name, invert)
    if key not in _results:
        c = cc.case(name)
        data, r0 = cc.extraction(c)
        s = oracles[c.dtype].isosurface(data, c.iso, r0, c.d)
        T = cc.without_nonfinite(s.V, s.T) if name == "hole" else s.T
        _results[key] = (c, (s.V, s.N, T), co.cap(s.V, s.N, T, c.data, c.iso, c.r0, c.d, c.lo, c.hi, invert=invert))
    return _results[key]


def box_volume_area(c):
    e = [(c.hi[a] - c.lo[a]) * c.d[a] for a in range(3)]
    return e[0] * e[1] * e[2], 2.0 * ((e[0] * e[1] + e[1] * e[2]) + e[0] * e[2])


# ---- the oracle against independent facts -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CLOSED)
def test_capped_surfaces_are_closed_manifold_and_oriented(oracles, name):
    c, (V, N, T), o = capped(oracles, name)
    print("    %s: %r" % (name, dict(zip(co.COUNTS, o.counts()))))
    assert o.skipped_cells == 0 and o.off_face_edges == 0 and o.closed == 1 and o.solid_above == 1
    assert o.V.shape == (o.nV_out, 3) and o.N.shape == (o.nV_out, 3) and o.T.shape == (o.nT_out, 3) and o.V.dtype == V.dtype
    e = to.EdgeTable(o.T, o.nV_out)
    assert e.invalid == 0 and not e.boundary.any() and not e.nonmanifold.any() and not e.misoriented.any() and not e.degenerate.any()
    named = np.zeros(o.nV_out, bool)
    named[o.T.astype(np.int64).reshape(-1)] = True
    assert named[V.shape[0]:].all() and np.array_equal(named[:V.shape[0]], np.isin(np.arange(V.shape[0]), T))  # every new vertex is named
    # the rows of the surface keep their bytes
    assert o.V[:V.shape[0]].tobytes() == V.tobytes() and o.N[:V.shape[0]].tobytes() == N.tobytes() and o.T[:T.shape[0]].tobytes() == T.tobytes()


@pytest.mark.parametrize("name", CLOSED)
def test_cap_triangles_face_outwards_and_vertices_sit_on_the_grid(oracles, name):
    c, (V, N, T), o = capped(oracles, name)
    P = o.V[o.T[T.shape[0]:].astype(np.int64)].astype(np.float64)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    for f in range(6):
        a, sign = f >> 1, (1.0 if f & 1 else -1.0)
        rows = n[o.cap_faces == f]
        assert np.all(rows[:, a] * sign > 0.0) and np.all(np.delete(rows, a, axis=1) == 0.0), (name, f)
    # a new vertex: a grid point of the box's surface, its normal the unit sum of the outward normals of the faces that name it
    real = V.dtype.type
    for k, p in enumerate(sorted(o.used, key=lambda p: (p[2] * c.data.shape[1] + p[1]) * c.data.shape[2] + p[0])):
        row = o.V[V.shape[0] + k]
        assert [float(x) for x in row] == [float(real(p[a]) * real(c.d[a]) + real(c.r0[a])) for a in range(3)]
        on = [(-1 if p[a] == c.lo[a] else 0) + (1 if p[a] == c.hi[a] else 0) for a in range(3)]
        nn = o.N[V.shape[0] + k].astype(np.float64)
        assert abs(np.sqrt((nn * nn).sum()) - 1.0) < 1e-6 and all(nn[a] * on[a] >= 0.0 and (on[a] != 0 or nn[a] == 0.0) for a in range(3))


def edge_vertices(V, c, tol):
    """{(axis, grid point below): row of V} of the vertices that lie on a grid edge: one coordinate between two grid planes"""
    g = (V.astype(np.float64) - np.array(c.r0)) / np.array(c.d)
    r = np.rint(g)
    between = np.abs(g - r) > tol
    out = {}
    for v in np.nonzero(between.sum(axis=1) == 1)[0]:
        a = int(np.argmax(between[v]))
        p = [int(x) for x in r[v]]
        p[a] = int(np.floor(g[v, a]))
        out[(a, tuple(p))] = v
    return out


def solid_area_of_face(c, V, f, edges):
    """the area of the solid region of face f by marching squares over the samples in float64: the polygon of every cell walked
    counterclockwise - a solid corner, then the vertex of V on the cell edge behind it where the next corner is not solid - and
    measured by the shoelace formula; two diagonal solid corners are joined when the bilinear interpolant says so (f0 f2 > f1 f3
    for the solid pair 0, 2), separated otherwise.  Returns (area, the length of the rim on the face)."""
    box = co.Box(c.lo, c.hi)
    u, w = co.in_plane(f)
    F = c.data.astype(np.float64) - np.float64(np.float32(c.iso) if c.dtype != "f64" else c.iso)
    area, rim = 0.0, 0.0

    def world(p):
        return np.array([c.r0[a] + p[a] * c.d[a] for a in range(3)], np.float64)

    def shoelace(pts):
        s = 0.0
        for k in range(len(pts)):
            p, q = pts[k], pts[(k + 1) % len(pts)]
            s += p[u] * q[w] - q[u] * p[w]
        return (-s if co.FLIP[f] else s) * 0.5

    for cw in range(c.lo[w], c.hi[w]):
        for cu in range(c.lo[u], c.hi[u]):
            Q = box.corners(f, cu, cw)
            val = [F[p[2], p[1], p[0]] for p in Q]
            sol = [x > 0.0 for x in val]
            X = {}
            for k in range(4):
                p, q = Q[k], Q[(k + 1) & 3]
                if sol[k] != sol[(k + 1) & 3]:
                    a = [i for i in range(3) if p[i] != q[i]][0]
                    X[k] = V[edges[(a, tuple(min(p[i], q[i]) for i in range(3)))]].astype(np.float64)
            if sum(sol) == 2 and sol[0] == sol[2]:
                k0 = 0 if sol[0] else 1  # the solid pair k0, k0 + 2
                if val[k0] * val[k0 + 2] > val[(k0 + 1) & 3] * val[(k0 + 3) & 3]:
                    polys = [[world(Q[k0]), X[k0], X[k0 + 1], world(Q[k0 + 2]), X[(k0 + 2) & 3], X[(k0 + 3) & 3]]]
                    cuts = [(X[k0], X[k0 + 1]), (X[(k0 + 2) & 3], X[(k0 + 3) & 3])]
                else:
                    polys = [[world(Q[k0]), X[k0], X[(k0 + 3) & 3]], [world(Q[k0 + 2]), X[(k0 + 2) & 3], X[k0 + 1]]]
                    cuts = [(X[k0], X[(k0 + 3) & 3]), (X[(k0 + 2) & 3], X[k0 + 1])]
            else:
                poly = []
                for k in range(4):
                    if sol[k]:
                        poly.append(world(Q[k]))
                    if k in X:
                        poly.append(X[k])
                polys = [poly] if len(poly) >= 3 else []
                cuts = [tuple(X.values())] if len(X) == 2 else []
            area += sum(shoelace(p) for p in polys)
            rim += sum(float(np.sqrt(((a - b) ** 2).sum())) for a, b in cuts)
    return area, rim


@pytest.mark.parametrize("name", CLOSED)
def test_cap_area_is_the_solid_area_of_every_face(oracles, name):
    """The bound is derived: the cap's polygon and the formula's differ by where the rim runs, every rim vertex is a row of V, a
    float (double) whose last place is 2^-23 (2^-52) of its size, and moving a rim of length L sideways by h changes the area by
    L h: per face, rim length x largest |coordinate| x 2^-23.  (Both sides read the same rows of V, so what is left is the
    rounding of two float64 sums, far inside it; for the dome the bound comes to about 5e-5 on areas of 60 to 130.)"""
    c, (V, N, T), o = capped(oracles, name)
    edges = edge_vertices(V, c, co.tolerance(c.r0, c.d, c.data.shape).max())
    P = o.V[o.T[T.shape[0]:].astype(np.int64)].astype(np.float64)
    areas = 0.5 * np.sqrt((np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) ** 2).sum(axis=1))
    largest = float(np.abs(o.V.astype(np.float64)).max()) if o.nV_out else 0.0
    for f in range(6):
        want, rim = solid_area_of_face(c, V, f, edges)
        got = mo.fsum(areas[o.cap_faces == f])
        bound = rim * largest * 2.0 ** -23
        print("    %s face %d: area %.9g, formula %.9g, rim %.6g, bound %.3g" % (name, f, got, want, rim, bound))
        assert abs(got - want) <= bound + 8 * np.finfo(np.float64).eps * want, (name, f)


@pytest.mark.parametrize("name", CLOSED)
def test_closed_surface_identities(oracles, name):
    """The area vectors of a closed oriented surface sum to zero, and its volume does not depend on the origin.  Bounds: a cross
    product component is a difference of two products of at most |u||w|, each a few rounding errors, and n terms are summed:
    (n + 8) 2^-53 sum |u||w|; for the volumes, measure_oracle's own bounds of its two sums."""
    c, (V, N, T), o = capped(oracles, name)
    if not o.nT_out:
        return
    P = o.V[o.T.astype(np.int64)].astype(np.float64)
    u, w = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    bound = (o.nT_out + 8) * 2.0 ** -53 * mo.fsum(np.sqrt((u * u).sum(axis=1)) * np.sqrt((w * w).sum(axis=1)))
    x = np.cross(u, w)
    for a in range(3):
        assert abs(mo.fsum(x[:, a])) <= bound, (name, a)
    m1 = mo.measure(o.V, o.T, c.r0, c.d, c.data.shape)
    m2 = mo.measure(o.V, o.T, c.r0, c.d, c.data.shape, c=np.array([17.25, -40.5, 3.0]))
    print("    %s: volume %.12g / %.12g, bounds %.3g + %.3g" % (name, m1.volume, m2.volume, m1.volume_bound, m2.volume_bound))
    assert abs(m1.volume - m2.volume) <= m1.volume_bound + m2.volume_bound and m1.volume > 0.0


def test_cases_show_what_they_are_for(oracles):
    sizes = {n: capped(oracles, n)[2].polygon_sizes for n in cc.NAMES}
    segs = {n: capped(oracles, n)[2] for n in cc.NAMES}
    for name in ("saddle", "noise"):  # diagonal cells of both resolutions: a hexagon, and two triangles in one cell
        o = segs[name]
        assert 6 in sizes[name]
        assert o.capped_cells < len(sizes[name]), name  # (a cell with two polygons)
    box = co.Box(*[getattr(cc.case("corner"), k) for k in ("lo", "hi")])
    o = segs["corner"]
    assert (0, 0, 0) in o.used and o.used[(0, 0, 0)] == 0b010101  # the box corner, named by three faces
    assert sum(1 for m in o.used.values() if bin(m).count("1") == 2) >= 3 and box.points > len(o.used)
    assert capped(oracles, "one")[2].capped_cells == 6
    assert cc.case("quant").on_faces > 0 and cc.case("sub").lo[2] == 2 and cc.case("sub").hi[2] == 6


def test_full_and_empty_boxes(oracles):
    c, _, o = capped(oracles, "full")
    box = co.Box(c.lo, c.hi)
    assert o.cap_triangles == 2 * box.cells and o.cap_vertices == box.points and o.nV_out == box.points and o.rim_segments == 0
    m = mo.measure(o.V, o.T, c.r0, c.d, c.data.shape)
    vol, area = box_volume_area(c)
    assert abs(m.volume - vol) <= m.volume_bound and abs(m.area - area) <= m.area_bound
    c, _, o = capped(oracles, "none")
    assert o.counts() == (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1)


def test_cells_with_a_sample_on_the_isovalue_are_skipped(oracles):
    c, (V, N, T), o = capped(oracles, "quant")
    before = to.EdgeTable(T, V.shape[0])
    assert not before.nonmanifold.any() and not before.misoriented.any()
    e = to.EdgeTable(o.T, o.nV_out)
    assert o.skipped_cells > 0 and o.closed == 0 and o.capped_cells > 0
    assert not e.nonmanifold.any() and not e.misoriented.any() and e.boundary.any() and e.invalid == 0


def test_a_hole_off_the_faces_is_counted_and_left_alone(oracles):
    c, (V, N, T), o = capped(oracles, "hole")
    dome = capped(oracles, "dome")[2]
    assert o.off_face_edges > 0 and o.closed == 0 and o.nonfinite_vertices > 0
    assert (o.skipped_cells, o.capped_cells, o.cap_triangles, o.cap_vertices, o.rim_segments) == (0, dome.capped_cells, dome.cap_triangles, dome.cap_vertices, dome.rim_segments)
    e = to.EdgeTable(o.T, o.nV_out)
    assert int(e.boundary.sum()) == o.off_face_edges and not e.nonmanifold.any() and not e.misoriented.any()


def test_invert_caps_the_other_side(oracles):
    c, (V, N, T), o = capped(oracles, "dome")
    _, _, i = capped(oracles, "dome", invert=True)
    assert (o.solid_above, i.solid_above) == (1, 0) and i.closed == 1 and i.skipped_cells == 0
    assert np.array_equal(i.T[:T.shape[0]], T[:, [0, 2, 1]]) and np.array_equal(i.N[:V.shape[0]], -N) and i.V[:V.shape[0]].tobytes() == V.tobytes()
    e = to.EdgeTable(i.T, i.nV_out)
    assert not e.boundary.any() and not e.nonmanifold.any() and not e.misoriented.any()
    m, mi = mo.measure(o.V, o.T, c.r0, c.d, c.data.shape), mo.measure(i.V, i.T, c.r0, c.d, c.data.shape)
    vol, _ = box_volume_area(c)
    # both are wound outwards from their solid: the two volumes are positive and fill the box
    assert m.volume > 0.0 and mi.volume > 0.0 and abs((m.volume + mi.volume) - vol) <= m.volume_bound + mi.volume_bound
    # the other flavour of the library: the opposite winding has the opposite solid side
    n = co.cap(V, -N, T[:, [1, 0, 2]], c.data, c.iso, c.r0, c.d, c.lo, c.hi, normal_neg=True)
    assert n.solid_above == 0 and n.closed == 1 and n.cap_triangles == i.cap_triangles


def test_attributes_of_new_vertices(oracles):
    c, (V, N, T), o = capped(oracles, "corner")
    A = (np.arange(V.shape[0], dtype=np.float32), np.arange(V.shape[0], dtype=np.uint32) + 7)
    a = co.cap(V, N, T, c.data, c.iso, c.r0, c.d, c.lo, c.hi, attrs=A, attr_modes=(co.F32, co.WORD))
    assert a.counts() == o.counts() and np.isnan(a.attrs[0].view(np.float32)[V.shape[0]:]).all() and not a.attrs[1][V.shape[0]:].any()
    assert np.array_equal(a.attrs[1][:V.shape[0]], A[1])


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_cap_surface\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_capping;", hip)
    assert re.search(r"#define MC33HIP_CAP_WORD 0\b", hip) and re.search(r"#define MC33HIP_CAP_F32 1\b", hip)
    assert re.search(r"\bsurface \*MC33_calculate_capped_isosurface\(MC33 \*", pub) and re.search(r"\} mc33_cap;", pub) and re.search(r"\} mc33_cap_info;", pub)
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)
    from mc33_c_library_amd import DeviceGrid
    assert callable(DeviceGrid.cap) and callable(DeviceGrid.extract_capped)
    from mc33_c_library_amd import build
    assert "mc33_cap.hip.h" in build.HIP_HEADERS
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert '#include "mc33_smooth.hip.h"\n#include "mc33_cap.hip.h"\n' in kernels and "k_cap_sides" in kernels  # (behind the parts it builds on)
    assert kernels.index('#include "mc33_measure.hip.h"') < kernels.index('#include "mc33_cap.hip.h"')
    assert " mc33_cap.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_cap_kernels_are_in_the_code_object(dtype):
    real = "double" if dtype == "f64" else "float"
    assert_kernels(dtype, KERNELS + ["k_cap_%s<%s>" % (k, real) for k in ("flag", "rim", "cell", "emit", "verts")])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_cap(dtype):
    """mc33_capi.c linked with the emulated device layer, which cannot cap: the library still loads (a weak reference),
    MC33_calculate_capped_isosurface returns NULL and leaves the object and the info alone - for good arguments and, which needs
    no device in any build, for a refused box -, and the object extracts as before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        before = (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        L.free_surface_memory(S)
        info = SurfaceCapInfo()
        info.nV, info.closed = 77, 5
        good = SurfaceCap((C.c_uint * 3)(1, 1, 1), (C.c_uint * 3)(9, 9, 9), 0)
        cases = [None, good, SurfaceCap((C.c_uint * 3)(3, 0, 0), (C.c_uint * 3)(3, 9, 9), 0), SurfaceCap((C.c_uint * 3)(0, 0, 0), (C.c_uint * 3)(9, 99, 9), 1)]
        for opt in cases:
            assert not L.MC33_calculate_capped_isosurface(M, lib.real(iso + 1), C.byref(opt) if opt is not None else None, C.byref(info))
            assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
            assert (info.nV, info.closed) == (77, 5)
        assert not L.MC33_calculate_capped_isosurface(M, lib.real(iso + 1), None, None)
        assert (M.contents.iso, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
