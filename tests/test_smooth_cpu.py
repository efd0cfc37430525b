"""Smoothing extracted surfaces, the part that needs no GPU: the numpy oracle of the Taubin passes and of the
recomputed normals on the unmodified reference's meshes against figures computed once from them, its invariants, the new names
in the headers, the libraries and the code objects, and the host-logic build of mc33_capi.c, whose emulated device layer
cannot smooth.

test_oracle_on_the_reference_meshes and the invariant tests test the oracle and the fixtures, not the product: they pin
tests/smooth_oracle.py and pass without the feature.  The product is held to that oracle by the name, struct, export,
code-object and host-logic tests below and, on the device, by tests/test_gpu_smooth.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import measure_oracle as mo
import smooth_oracle as so
from mc33_c_library_amd.api import SurfaceSmoothing
from mesh_checks import assert_exported, assert_kernels, host_logic, launched
from smooth_cases import TABLE, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_smooth_surface", "mc33hip_vertex_normals"]
C_NAMES = ["MC33_calculate_smoothed_isosurface"]
KERNELS = ["k_sm_count<0>", "k_sm_count<1>", "k_sm_fill<0>", "k_sm_fill<1>", "k_sm_rows"] + launched("k_mesh_tile_sum<MeshCount>", "k_mesh_scan_top", "k_mesh_place<MeshCount, 2>")

@pytest.mark.parametrize("name", list(TABLE))
def test_oracle_on_the_reference_meshes(reflibs, name):
    data, r0, d, iso, s, A, P = mesh(reflibs, name)
    maxdeg, lone, nbnd, a0, a_pin, a_free = TABLE[name]
    area = [mo.measure(v, s.T, r0, d, data.shape).area for v in (s.V, P[True], P[False])]
    print("%s: max degree %d, isolated %d, boundary %d, area %.4f -> %.4f pinned, %.4f not" % (name, A.max_degree, A.isolated_vertices, A.boundary_vertices, *area))
    assert (A.max_degree, A.isolated_vertices, A.boundary_vertices, A.invalid_triangles) == (maxdeg, lone, nbnd, 0)
    for got, want in zip(area, (a0, a_pin, a_free)):
        print("   %.6f against %.4f: relative difference %.2e" % (got, want, abs(got - want) / want))
        # The table gives four decimals, so a figure is known to half a unit of the last one - 4e-6 of the sphere's area, more
        # than the 1e-6 relative the areas are otherwise compared to.  Asked here: the area printed to four decimals IS the
        # figure, which is the most its format can tell, and never less than 1e-6 relative beyond that half unit.
        assert "%.4f" % got == "%.4f" % want and abs(got - want) <= 1e-6 * want + 0.5e-4, (got, want)


@pytest.mark.parametrize("name", list(TABLE))
def test_oracle_invariants(reflibs, name):
    data, r0, d, iso, s, A, P = mesh(reflibs, name)
    still = A.boundary | (A.deg == 0)
    assert np.array_equal(P[True][still].view(np.uint32), s.V[still].view(np.uint32))  # pinned and isolated rows: V's bits
    lone = A.deg == 0
    assert np.array_equal(P[False][lone].view(np.uint32), s.V[lone].view(np.uint32))
    if A.boundary_vertices:
        assert np.any(P[False][A.boundary] != s.V[A.boundary])
    f0, f1 = so.face_normals(s.V, s.T), so.face_normals(P[True], s.T)
    flips = int(np.count_nonzero((f0 * f1).sum(1) < 0))
    print("%s: %d of %d triangles flip" % (name, flips, s.nT))
    if name == "noise":
        assert flips <= 1e-3 * s.nT
    else:
        assert flips == 0
    if name == "sphere":
        v0, v1 = (mo.measure(v, s.T, r0, d, data.shape).volume for v in (s.V, P[True]))
        print("sphere: volume %.4f -> %.4f" % (v0, v1))
        assert v0 < 0 and abs(v1 - v0) < 1e-3 * abs(v0)
    if name == "quant":
        a0, a1 = (mo.measure(v, s.T, r0, d, data.shape).area for v in (s.V, P[True]))
        assert a1 < 0.9 * a0
    # iterations == 0 and skipped passes leave the bits; a skipped mu pass is pass(lambda) alone
    assert np.array_equal(so.smooth(s.V, s.T, 0, A=A)[0].view(np.uint32), s.V.view(np.uint32))
    fixed = still
    one = so.one_pass(s.V, A, fixed, 0.5)
    assert np.array_equal(so.smooth(s.V, s.T, 1, 0.5, 0.0, True, A=A)[0].view(np.uint32), one.view(np.uint32))


@pytest.mark.parametrize("name", ["sphere", "blobs", "sheet"])
def test_recomputed_normals_agree_with_the_reference(reflibs, name):
    data, r0, d, iso, s, A, P = mesh(reflibs, name)
    n = so.vertex_normals(s.V, s.T)
    dots = (n.astype(np.float64) * s.N).sum(1)
    print("%s: smallest dot product with the reference's N %.4f" % (name, dots.min()))
    assert dots.min() >= 0.99


def test_oracle_definitions_on_a_tiny_mesh():
    # two triangles that share the edge {1, 2}, a degenerate one, an invalid one, vertex 5 isolated
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 2, 2], [9, 9, 9]], np.float32)
    T = np.array([[0, 1, 2], [2, 1, 3], [4, 4, 3], [0, 1, 6]], np.uint32)
    A = so.adjacency(T, 6)
    assert A.deg.tolist() == [2, 3, 3, 3, 1, 0] and A.invalid_triangles == 1 and A.isolated_vertices == 1 and A.max_degree == 3
    assert A.nbr[A.start[3]:A.start[4]].tolist() == [1, 2, 4]
    assert A.boundary.tolist() == [True, True, True, True, False, False]  # {1, 2} and {3, 4} (4 -> 3, 3 -> 4) have two uses
    P, _ = so.smooth(V, T, 3, 0.5, -0.53, True)
    assert np.array_equal(P[[0, 1, 2, 3, 5]].view(np.uint32), V[[0, 1, 2, 3, 5]].view(np.uint32)) and np.all(P[4] != V[4])
    P, _ = so.smooth(V, T, 1, 1.0, 0.0, False)
    assert np.array_equal(P[0], ((V[1].astype(np.float64) + V[2]) / 2.0).astype(np.float32)) and np.array_equal(P[5], V[5])
    n = so.vertex_normals(V, T)
    assert n[0].tolist() == [0.0, 0.0, 1.0] and n[5].tolist() == [0.0, 0.0, 0.0] and n[4].tolist() == [0.0, 0.0, 0.0]
    neg = np.array([[-0.0, 1.0, 2.0]], np.float32)
    assert np.signbit(so.smooth(neg, np.zeros((0, 3), np.uint32), 2)[0][0, 0])


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_smooth_surface\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_smoothing;", hip)
    assert re.search(r"\bint mc33hip_vertex_normals\(mc33hip_ctx \*", hip)
    assert re.search(r"\bsurface \*MC33_calculate_smoothed_isosurface\(MC33 \*", pub) and re.search(r"\} mc33_smoothing;", pub)
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype,real", [("f32", "float"), ("f64", "double")])
def test_smoothing_kernels_are_in_the_code_object(dtype, real):
    assert_kernels(dtype, KERNELS + ["k_sm_pass<%s>" % real, "k_sm_normals<%s>" % real])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_smooth(dtype):
    """mc33_capi.c linked with the emulated device layer, which cannot smooth: the library still loads (a weak reference),
    MC33_calculate_smoothed_isosurface returns NULL and leaves the object alone, and the object extracts as before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        sm = SurfaceSmoothing(10, 0.5, -0.53, 1)
        assert not L.MC33_calculate_smoothed_isosurface(M, lib.real(iso), C.byref(sm)) and M.contents.memoryfault == 0
        assert not L.MC33_calculate_smoothed_isosurface(M, lib.real(iso), None)
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
