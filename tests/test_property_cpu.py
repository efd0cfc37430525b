"""Property grid (colours from a second scalar field), the part that needs no GPU: the numpy oracle of the definition against an
analytic field, the new names in the headers and in every built library, and the host-logic build of mc33_capi.c, whose
emulated device layer cannot sample and must say so."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fixtures as fx
import property_oracle as po
from mesh_checks import assert_exported, assert_kernels, host_logic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AWKWARD_R0, AWKWARD_D = (-1.3, 0.7, 2.9), (0.1, 0.07, 0.13)

HIP_NAMES = ["mc33hip_property_upload_rows", "mc33hip_property_upload_contiguous", "mc33hip_property_adopt_device", "mc33hip_property_drop",
             "mc33hip_sample_property", "mc33hip_color_vertices", "mc33hip_download_enqueue"]
C_NAMES = ["MC33_set_property_grid", "MC33_set_color_map"]


def linear_property(shape, dtype):
    """P[k][j][i] = 3i - 2j + 5k + 7: exact in every sample type (the callers keep it within the type's range)."""
    k, j, i = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    return (3 * i - 2 * j + 5 * k + 7).astype(dtype)


def test_oracle_reproduces_a_linear_property(reflibs):
    """Trilinear interpolation is exact on a linear field: |oracle - (3 g_x - 2 g_y + 5 g_z + 7)| <= 2^-23 max|P| with g clamped
    to [0, N] - the double sum of exactly representable samples errs by a few 2^-53, the rounding to float by 2^-24 relative."""
    data, _, _ = fx.cos_field(48)
    V = reflibs["f32"].isosurface(data, 0.0, AWKWARD_R0, AWKWARD_D).V
    assert V.shape[0] == 8424
    P = linear_property(data.shape, np.float32)
    got = po.sample_property(V, AWKWARD_R0, AWKWARD_D, P)
    g, _, _ = po.grid_coordinates(V, AWKWARD_R0, AWKWARD_D, data.shape)
    g = np.clip(g, 0.0, 47.0)
    want = 3.0 * g[:, 0] - 2.0 * g[:, 1] + 5.0 * g[:, 2] + 7.0
    err = np.abs(got.astype(np.float64) - want).max()
    bound = 2.0 ** -23 * np.abs(P.astype(np.float64)).max()
    print("largest error %.3g, bound %.3g, %d vertices" % (err, bound, V.shape[0]))
    assert err <= bound


def test_oracle_clamps_and_colours():
    """the corners of the definition on a 2 x 2 x 2-cell grid, by hand"""
    P = linear_property((3, 3, 3), np.float32)
    V = np.array([[0, 0, 0], [2, 2, 2], [-0.25, 1, 1], [2.5, 0.5, 0], [1, 1, 1.5]], np.float32)
    got = po.sample_property(V, (0, 0, 0), (1, 1, 1), P)
    assert got.tolist() == [7.0, 19.0, 10.0, 12.0, 15.5]  # (below the grid: clamped to x = 0; beyond it: i = N, f = 0)
    pal = [0x11, 0x22, 0x33]
    c = po.color_values(np.array([7.0, 9.0, 12.9, 15.9, 16.0, 100.0, -5.0, np.nan], np.float32), pal, 7.0, 19.0)
    assert c.tolist() == [0x11, 0x11, 0x22, 0x22, 0x33, 0x33, 0x11, int(po.DEFAULT_COLOR)]
    P2 = P.copy()
    P2[0, 0, 1] = np.nan  # a neighbour that f == 0 must not read
    assert po.sample_property(V[:1], (0, 0, 0), (1, 1, 1), P2)[0] == 7.0


def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    for n in HIP_NAMES:
        assert re.search(r"\bint %s\(mc33hip_ctx \*" % n, hip), n
    for n in C_NAMES:
        assert re.search(r"\bint %s\(MC33 \*" % n, pub), n
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


def test_property_kernel_is_in_the_code_object():
    assert_kernels("f32", ("k_property<float, true>", "k_property<float, false>"))


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_a_property_grid(dtype):
    """mc33_capi.c linked with the emulated device layer, which has none of the property entry points: the library still loads
    (they are weak references), MC33_set_property_grid returns -1, a colour map alone changes nothing."""
    with host_logic(dtype, prop=linear_property) as h:
        lib, L, M, iso, Pg = h.lib, h.L, h.M, h.iso, h.Pg
        assert L.MC33_set_property_grid(M, Pg) == -1
        assert L.MC33_set_property_grid(M, None) == -1
        pal = (C.c_int * 3)(1, 2, 3)
        assert L.MC33_set_color_map(M, pal, 3, 0.0, 1.0) == 0
        assert L.MC33_set_color_map(M, pal, 1, 0.0, 1.0) == -1 and L.MC33_set_color_map(M, pal, 257, 0.0, 1.0) == -1
        assert L.MC33_set_color_map(M, pal, 3, 1.0, 1.0) == -1 and L.MC33_set_color_map(M, pal, 3, float("nan"), 1.0) == -1
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        s = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert s.nV > 0 and np.all(s.color == po.DEFAULT_COLOR)
        assert L.MC33_set_color_map(M, None, 0, 0.0, 0.0) == 0
