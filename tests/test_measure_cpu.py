"""Surface measures (area, volume, components), the part that needs no GPU: the numpy oracle of the definition against the figures
of the unmodified reference's meshes and against the analytic sphere, its labels against an independent formulation, the
invariance of a closed surface's volume under the reference point, the new names in the headers and in every built library, the
new kernels in the code object, and the host-logic build of mc33_capi.c, whose emulated device layer cannot measure."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import measure_oracle as mo
from mc33_c_library_amd.api import Component
from mc33_capi import CMeasure
from mesh_checks import assert_exported, assert_kernels, host_logic, launched, reference_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_measure_surface", "mc33hip_label_components", "mc33hip_measure_components"]
C_NAMES = ["MC33_measure_isosurface", "MC33_measure_isosurfaces", "MC33_measure_components"]
KERNELS = ["k_measure_triangles<float, true>", "k_measure_triangles<float, false>", "k_measure_bbox<float>", "k_measure_finish", "k_cc_init", "k_cc_union",
           "k_cc_flatten", "k_cc_flag", "k_cc_count", "k_cc_table_triangles<float>", "k_cc_table_vertices"] + launched("k_mesh_scan_top", "k_mesh_place<MeshFlag, 0>")

# what the issue's table adds to mo.FIXTURES: total area and signed volume of the reference's mesh, to the digits it quotes
FIGURES = {"sphere": (12.561676, -4.185969), "blobs": (759.193278, 375.618205)}


def mesh(reflibs, name):
    data, r0, d, iso, s = reference_mesh(reflibs, name)
    return data, r0, d, s


@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_oracle_on_the_reference_meshes(reflibs, name):
    data, r0, d, s = mesh(reflibs, name)
    nV, nT, ncomp, unref, edges = mo.FIXTURES[name][2]
    assert (s.nV, s.nT) == (nV, nT)
    lab, gc, gu, rounds = mo.label_components(s.T, s.nV)
    assert (gc, gu, mo.open_edges(s.T)) == (ncomp, unref, edges)
    assert np.unique(lab).size == ncomp + unref
    m = mo.measure(s.V, s.T, r0, d, data.shape)
    tab, ab, wb = mo.component_table(s.V, s.T, lab, m.origin)
    print("%s: area %.6f (bound %.2g) volume %.6f (bound %.2g), %d rounds" % (name, m.area, m.area_bound, m.volume, m.volume_bound, rounds))
    assert tab.shape[0] == ncomp and int(tab["nT"].sum()) == nT and int(tab["nV"].sum()) == nV - unref
    assert np.array_equal(tab["root"], np.unique(lab[s.T[:, 0].astype(np.int64)]))
    assert 1.5e-11 <= min(m.area_bound, m.volume_bound) and max(m.area_bound, m.volume_bound) <= 1e-7  # (2e-11 .. 1e-7, rounded)
    if name in FIGURES:
        assert abs(m.area - FIGURES[name][0]) < 1e-6 and abs(m.volume - FIGURES[name][1]) < 1e-6
    if name == "blobs":
        assert tab["nT"].min() == 1868 and tab["nT"].max() == 1940
        assert round(float(tab["volume"].min()), 4) == 13.9117 and round(float(tab["volume"].max()), 4) == 13.9118
    if name == "quant":
        assert sorted(tab["nT"].tolist())[-1] == 33856 and sorted(tab["nT"].tolist())[0] == 4 and sorted(tab["nT"].tolist())[-2] == 16
    # the double sums a device may form stay far inside the bound; a float accumulator does not
    A = mo.triangle_terms(s.V, s.T, m.origin)["A"]
    for other in (float(np.sum(A)), float(np.add.accumulate(A)[-1]), float(np.add.accumulate(A[::-1])[-1])):
        assert abs(other - m.area) * 100.0 <= m.area_bound
    assert abs(float(np.add.accumulate(A.astype(np.float32))[-1]) - m.area) > 1000.0 * m.area_bound


def test_oracle_against_the_analytic_sphere(reflibs):
    """radius 1: the faceted surface lies inside the sphere - 3.7e-4 of the area, 6.7e-4 of the volume missing, with room for
    nothing else; the volume is NEGATIVE with the reference's winding; the centroid is the centre"""
    data, r0, d, s = mesh(reflibs, "sphere")
    m = mo.measure(s.V, s.T, r0, d, data.shape)
    da, dv = 1.0 - m.area / (4.0 * math.pi), 1.0 - (-m.volume) / (4.0 * math.pi / 3.0)
    print("relative deficits: area %.3g, volume %.3g" % (da, dv))
    assert m.volume < 0.0 and 3.6e-4 < da < 3.8e-4 and 6.6e-4 < dv < 6.8e-4
    assert np.all(np.abs(m.centroid - 2.0) < 1e-6)
    # the centre is a grid point, so the extreme vertices lie on grid lines through it, where the field is (x - 2)^2: linear
    # interpolation of it between two samples errs by at most h^2 / 4, which moves the crossing by at most h^2 / 8 (slope 2)
    h = d[0]
    assert np.all(np.abs(m.bbox_min - 1.0) <= h * h / 8.0) and np.all(np.abs(m.bbox_max - 3.0) <= h * h / 8.0)


@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_labels_against_scipy(reflibs, name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    data, r0, d, s = mesh(reflibs, name)
    lab = mo.label_components(s.T, s.nV)[0]
    T = s.T.astype(np.int64)
    i, j = np.concatenate([T[:, 0], T[:, 0]]), np.concatenate([T[:, 1], T[:, 2]])
    n, which = connected_components(sp.coo_matrix((np.ones(i.size, np.int8), (i, j)), shape=(s.nV, s.nV)), directed=False)
    smallest = np.full(n, s.nV, np.int64)
    np.minimum.at(smallest, which, np.arange(s.nV))
    assert np.array_equal(lab, smallest[which].astype(np.uint32))


@pytest.mark.parametrize("name", ["sphere", "blobs"])
@pytest.mark.parametrize("shift", [(0.37, -1.9, 2.3), (100.0, 50.0, -70.0)])
def test_volume_of_a_closed_surface_ignores_the_reference_point(reflibs, name, shift):
    """within the SUM of the two runs' bounds: the far point's terms are larger, and so is its bound"""
    data, r0, d, s = mesh(reflibs, name)
    assert mo.open_edges(s.T) == 0
    a = mo.measure(s.V, s.T, r0, d, data.shape)
    b = mo.measure(s.V, s.T, r0, d, data.shape, c=a.origin + np.array(shift))
    print("%s moved by %s: volume differs by %.3g, bounds %.3g + %.3g" % (name, shift, abs(a.volume - b.volume), a.volume_bound, b.volume_bound))
    assert abs(a.volume - b.volume) <= a.volume_bound + b.volume_bound
    assert abs(a.area - b.area) <= a.area_bound + b.area_bound


def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    for n in HIP_NAMES:
        assert re.search(r"\bint %s\(mc33hip_ctx \*" % n, hip), n
    for n in C_NAMES:
        assert re.search(r"\b(int|unsigned) %s\(MC33 \*" % n, pub), n
    for t in ("mc33hip_measures", "mc33hip_component"):
        assert re.search(r"\} %s;" % t, hip), t
    for t in ("mc33_measure", "mc33_component"):
        assert re.search(r"\} %s;" % t, pub), t
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


def test_measure_kernels_are_in_the_code_object():
    assert_kernels("f32", KERNELS, max_vgprs=128)  # (two blocks of 256 per SIMD at least)


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_measure(dtype):
    """mc33_capi.c linked with the emulated device layer, which has none of the measuring entry points: the library still loads
    (they are weak references), the three functions return -1 / 0 surfaces, and the object extracts as before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        m, many, rows, n, u = CMeasure(), (CMeasure * 3)(), (Component * 4)(), C.c_uint(7), C.c_uint(7)
        many[1].nT = 5
        assert L.MC33_measure_isosurface(M, lib.real(iso), C.byref(m)) == -1
        assert L.MC33_measure_isosurfaces(M, (lib.real * 3)(iso, iso, iso), 3, many) == 0 and many[1].nT == 0
        assert L.MC33_measure_components(M, lib.real(iso), rows, 4, C.byref(n), C.byref(u)) == -1 and (n.value, u.value) == (0, 0)
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
