"""Curvature from the grid's second differences, the part that needs no GPU.

The oracle facts pin tests/curvature_oracle.py itself - against analytic spheres and a hand case - and pass without the feature.
The product is held to that oracle by the tests behind them, which fail without the feature: the names, exports and struct
layouts, k_curvature in the code objects, the kernel's own text - curv_vertex of mc33_curvature.hip.h - compiled for the host into a
stand-alone program (tests/curvature_host.cpp) and held to the oracle bit for bit, once more under ASan and UBSan, and the host-logic
build of mc33_capi.c, whose emulated device layer has no curvature pass."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import curvature_cases as cc
import curvature_oracle as co
from mc33_c_library_amd.api import IsosurfaceCurvature
from mesh_checks import assert_exported, assert_kernels, host_logic, reference_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_curvature.hip.h")

HIP_NAMES = ["mc33hip_curvature_vertices", "mc33hip_color_values"]
C_NAMES = ["MC33_set_color_source", "MC33_isosurface_curvature"]
TYPES = ("f32", "f64", "u8", "u16", "u32")
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


# ---- the oracle against closed forms ------------------------------------------------------------------------------------------------

# (cells, radius, centre) -> the deviation of mean from 1 / r and of gauss from 1 / r^2 that the float64 prototype of the
# definition gave: the bounds are twice these
SPHERES = {
    "centre": ((32, 10, (16, 16, 16)), 2.5e-4, 5.0e-5),
    "corner": ((16, 12, (0, 0, 0)), 9.9e-4, 1.65e-4),   # (a sphere about a corner of the grid: the face rules)
}


@pytest.mark.parametrize("name", list(SPHERES))
def test_oracle_on_an_analytic_sphere(name):
    (cells, r, centre), dev_mean, dev_gauss = SPHERES[name]
    F, V = cc.sphere_case(cells, r, centre)
    assert F.dtype == np.float32 and V.shape[0] > 300
    mean, gauss, k1, k2 = (x.astype(np.float64) for x in co.curvature(V, *UNIT, F))
    em, eg = float(np.abs(mean - 1.0 / r).max()), float(np.abs(gauss - 1.0 / r ** 2).max())
    print("%s: %d vertices, |mean - 1/r| <= %.3g, |gauss - 1/r^2| <= %.3g" % (name, V.shape[0], em, eg))
    assert em <= 2 * dev_mean and eg <= 2 * dev_gauss
    assert (k1 >= k2).all() and np.abs(k1 - 1.0 / r).max() <= 4 * dev_mean + math.sqrt(2 * dev_gauss)   # (|k - mean| = sqrt(mean^2 - gauss))
    s = co.summary(co.curvature(V, *UNIT, F))
    assert s.finite == V.shape[0] and s.undefined == 0 and s.lo[0] > 0
    # the other sign: the negated mean, the same gauss, k1 and k2 exchanged and negated
    m2, g2, k12, k22 = co.curvature(V, *UNIT, F, sign=-1)
    m1, g1, k11, k21 = co.curvature(V, *UNIT, F)
    assert np.array_equal(m2, -m1) and np.array_equal(g2, g1) and np.array_equal(k12, -k21) and np.array_equal(k22, -k11)


def hand_field():
    """x^2 + 2 y^2 + 3 z^2 + x y on 3 x 3 x 3 points in index units: every second difference is exact"""
    z, y, x = np.meshgrid(*(np.arange(3, dtype=np.float64),) * 3, indexing="ij")
    return (x * x + 2 * y * y + 3 * z * z + x * y).astype(np.float32)


def closed_form(g, H, sign=1):
    """steps 3 - 8 in plain Python floats from a gradient and a symmetric matrix"""
    gx, gy, gz = g
    (hxx, hxy, hxz), (_, hyy, hyz), (_, _, hzz) = H
    g2 = (gx * gx + gy * gy) + gz * gz
    gHg = (((gx * gx) * hxx + (gy * gy) * hyy) + (gz * gz) * hzz) + 2.0 * ((((gx * gy) * hxy) + ((gx * gz) * hxz)) + ((gy * gz) * hyz))
    mean = sign * ((gHg - g2 * ((hxx + hyy) + hzz)) / ((2.0 * g2) * math.sqrt(g2)))
    A = (hyy * hzz - hyz * hyz, hxx * hzz - hxz * hxz, hxx * hyy - hxy * hxy, hxz * hyz - hxy * hzz, hxy * hyz - hxz * hyy, hxy * hxz - hxx * hyz)
    gAg = (((gx * gx) * A[0] + (gy * gy) * A[1]) + (gz * gz) * A[2]) + 2.0 * ((((gx * gy) * A[3]) + ((gx * gz) * A[4])) + ((gy * gz) * A[5]))
    gauss = gAg / (g2 * g2)
    r = math.sqrt(max(mean * mean - gauss, 0.0))
    return np.array([mean, gauss, mean + r, mean - r]).astype(np.float32)


HAND_H = ((2.0, 1.0, 0.0), (1.0, 4.0, 0.0), (0.0, 0.0, 6.0))
# vertex -> the interpolated gradient: central differences inside, one-sided on the faces (g_x = S(1) - S(0) = 1 + y at x = 0)
HAND = [
    ((1.0, 1.0, 1.0), (3.0, 5.0, 6.0)),      # on a node
    ((0.0, 1.0, 1.0), (2.0, 4.0, 6.0)),      # on a node of face x = 0: 2, not the true derivative 1
    ((0.5, 1.0, 1.0), (2.5, 4.5, 6.0)),      # on an edge
    ((0.5, 0.5, 0.5), (2.0, 3.5, 4.5)),      # inside a cell: eight nodes, all on faces
    ((-0.7, 1.0, 5.0), (2.0, 4.0, 9.0)),     # below and beyond the grid: clamped to the node (0, 1, 2), g_z = S(2) - S(1) = 9
]


def test_oracle_on_the_hand_case():
    F = hand_field()
    V = np.array([v for v, _ in HAND], np.float32)
    q = co.interpolated(V, *UNIT, F)
    for k, (v, g) in enumerate(HAND):
        assert tuple(float(q[a][k]) for a in range(3)) == g, (v, [float(q[a][k]) for a in range(3)])
        assert tuple(float(q[a][k]) for a in range(3, 9)) == (2.0, 4.0, 6.0, 1.0, 0.0, 0.0), v
    got = np.stack(co.curvature(V, *UNIT, F), axis=1)
    want = np.stack([closed_form(g, HAND_H) for _, g in HAND])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the clamped vertex is the node it is clamped to
    assert np.array_equal(np.stack(co.curvature(np.array([[0.0, 1.0, 2.0]], np.float32), *UNIT, F), axis=1).view(np.uint32), got[4:5].view(np.uint32))


def planted():
    """the hand field with NaNs in samples that the vertex (0.5, 0, 0) must not read: f_y = f_z = 0, so the nodes at y = 1 and
    z = 1 are not formed, and the stencils of (0, 0, 0) and (1, 0, 0) reach neither (1, 2, 1) nor (2, 2, 2) nor (2, 1, 1)"""
    F = hand_field()
    G = F.copy()
    G[1, 2, 1] = G[2, 2, 2] = G[1, 1, 2] = np.nan   # [z, y, x]
    return F, G, np.array([[0.5, 0.0, 0.0]], np.float32)


def test_oracle_reads_nothing_where_f_is_zero():
    F, G, V = planted()
    a, b = np.stack(co.curvature(V, *UNIT, F)), np.stack(co.curvature(V, *UNIT, G))
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and a vertex with f_y != 0 does read one of them
    assert np.isnan(np.stack(co.curvature(np.array([[0.5, 0.5, 0.0]], np.float32), *UNIT, G))).any()


def symmetric_field():
    z, y, x = np.meshgrid(*(np.arange(3, dtype=np.float64) - 1.0,) * 3, indexing="ij")
    return (x * x + y * y + z * z).astype(np.float32)


def test_oracle_counts_a_vanishing_gradient_as_undefined():
    F = symmetric_field()
    V = np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0]], np.float32)
    val = co.curvature(V, *UNIT, F)
    assert all(np.isnan(x[0]) for x in val) and all(np.isfinite(x[1]) for x in val)
    s = co.summary(val)
    assert (s.finite, s.undefined) == (1, 1) and s.lo[0] == s.hi[0] == float(val[0][1])
    none = co.summary(tuple(x[:1] for x in val))
    assert none.lo == (np.inf,) * 4 and none.hi == (-np.inf,) * 4 and (none.finite, none.undefined) == (0, 1)


# ---- Gauss-Bonnet on the reference's sphere, from the oracles alone ------------------------------------------------------------------------

# |total_gauss - 4 pi| as the curvature oracle and tests/measure_oracle.py give it on the reference's mesh of the sphere fixture
# (21030 vertices): measured once; the bound is twice that, rounded up to one significant digit
GAUSS_BONNET_MEASURED, GAUSS_BONNET_BOUND = 2.72e-3, 6e-3


def test_gauss_bonnet_on_the_sphere_fixture(reflibs):
    data, r0, d, iso, s = reference_mesh(reflibs, "sphere")
    mean, gauss, _, _ = co.curvature(s.V, r0, d, data)
    assert co.summary((mean, gauss, mean, mean)).undefined == 0
    tg, bound = co.total(s.V, s.T, r0, d, data.shape, gauss)
    tm, _ = co.total(s.V, s.T, r0, d, data.shape, mean)
    dev = abs(tg - 4.0 * math.pi)
    print("total_gauss = %.9g, 4 pi = %.9g, deviation %.3g (sum bound %.3g); total_mean = %.9g" % (tg, 4.0 * math.pi, dev, bound, tm))
    assert dev <= GAUSS_BONNET_BOUND
    assert dev >= 0.5 * GAUSS_BONNET_MEASURED   # (the figure quoted is the one measured)
    assert tm < 0   # (the samples of this sphere grow outwards: concave under sign +1)


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_curvature_vertices\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_curvature;", hip)
    assert re.search(r"\bint mc33hip_color_values\(mc33hip_ctx \*", hip)
    assert re.search(r"\bint MC33_set_color_source\(MC33 \*", pub) and re.search(r"\bint MC33_isosurface_curvature\(MC33 \*", pub) and re.search(r"\} mc33_curvature;", pub)
    for k, name in enumerate(("PROPERTY", "MEAN", "GAUSS", "K1", "K2")):
        assert re.search(r"#define MC33_COLOR_%s %d\b" % (name, k), pub)
    import mc33_c_library_amd as pkg
    assert set(HIP_NAMES) <= set(pkg.HIP_API) and set(C_NAMES) <= set(pkg.REFERENCE_API)
    assert callable(pkg.DeviceGrid.curvature) and callable(pkg.DeviceGrid.color_values) and pkg.VertexCurvature
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert '#include "mc33_resample.hip.h"\n#include "mc33_curvature.hip.h"\n#include "mc33_spectrum.hip.h"' in kernels and "k_curvature" in kernels
    from mc33_c_library_amd import build
    assert "mc33_curvature.hip.h" in build.HIP_HEADERS
    assert "mc33_curvature.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("dtype", TYPES)
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", TYPES)
def test_curvature_kernels_are_in_the_code_object(dtype):
    """at most 128 registers - four waves to a SIMD -, no scratch, no spill, and no LDS: the summary leaves a wave through shuffles"""
    ks = assert_kernels(dtype, ["k_curvature<%s>" % ("double" if dtype == "f64" else "float")], max_vgprs=128)
    assert_kernels(dtype, ["k_curv_init", "k_color_values"], max_vgprs=64)
    mine = sorted(n for n in ks if n.startswith("k_curv"))
    assert mine == sorted(["k_curv_init", "k_curvature<%s>" % ("double" if dtype == "f64" else "float")]), mine
    assert ks[mine[1]]["group_segment_fixed_size"] == 0 and ks["k_color_values"]["group_segment_fixed_size"] == 1024


# ---- the host-logic build: mc33_capi.c on a device layer without the curvature pass ------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_a_curvature(dtype):
    with host_logic(dtype, n=12) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
        for source in (1, 2, 3, 4, 5, -1):
            assert L.MC33_set_color_source(M, source) == -1
        assert L.MC33_set_color_source(M, 0) == 0 and L.MC33_set_color_source(None, 0) == -1
        out = IsosurfaceCurvature(7, 8)
        assert L.MC33_isosurface_curvature(M, lib.real(iso), C.byref(out)) == -1 and L.MC33_isosurface_curvature(M, lib.real(iso), None) == -1
        assert (out.nV, out.nT) == (7, 8)
        assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        # a map alone paints nothing: DefaultColorMC, as before
        assert L.MC33_set_color_map(M, (C.c_int * 2)(1, 2), 2, 0.0, 1.0) == 0
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        try:
            s = lib.copy_surface(S)
        finally:
            L.free_surface_memory(S)
        assert s.nV > 0 and np.all(s.color == np.uint32(0xff5c5c5c).view(np.int32))


# ---- the kernel's text compiled for the host ---------------------------------------------------------------------------------------------

HOST_FLAGS = ["-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra"]
# (the sanitizers' runtimes linked statically: the programs stand alone, whatever else the environment loads into a process)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("curvature_host") / "curvature_host")
    subprocess.check_call(["g++"] + HOST_FLAGS + [os.path.join(HERE, "curvature_host.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def host_program_sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: stand-alone, with its own main"""
    out = str(tmp_path_factory.mktemp("curvature_host_san") / "curvature_host_san")
    subprocess.check_call(["g++"] + HOST_FLAGS + SANITIZE + [os.path.join(HERE, "curvature_host.cpp"), "-o", out])
    return out


def run_host_case(program, tmp, F, r0, d, V, sign=1, lay_name="dense"):
    """F in the named layout, cut to the bytes from its first to its last grid point, through the host program: the four float
    arrays and the summary"""
    dtype = {v: k for k, v in cc.NP_DTYPES.items()}[F.dtype.type]
    flat, (pitch, slc, off) = cc.padded(F, lay_name)
    npz, npy, npx = F.shape
    flat = flat[off:off + (npz - 1) * slc + (npy - 1) * pitch + npx].copy()
    V = np.ascontiguousarray(V, cc.real_of(dtype))
    cf, of = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(cf, "wb") as f:
        f.write(np.array([cc.TYPE_CODE[dtype], npx, npy, npz, pitch, slc, V.shape[0], sign], np.int64).tobytes())
        f.write(np.array(list(r0) + list(d), np.float64).tobytes())
        f.write(np.array([flat.size], np.int64).tobytes())
        f.write(flat.tobytes())
        f.write(V.tobytes())
    r = subprocess.run([program, cf, of], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(of, "rb").read()
    n = V.shape[0]
    assert len(raw) == 16 * n + 36
    val = np.frombuffer(raw, np.float32, 4 * n).reshape(n, 4)
    words = struct.unpack_from("9I", raw, 16 * n)

    def unkey(k):
        return float(np.array([k & 0x7FFFFFFF if k >> 31 else ~k & 0xFFFFFFFF], np.uint32).view(np.float32)[0])
    return val, co.Summary(tuple(unkey(k) for k in words[:4]), tuple(unkey(k) for k in words[4:8]), n - words[8], words[8])


def check_host(program, tmp, F, r0, d, V, sign=1, lay_name="all"):
    got, summ = run_host_case(program, tmp, F, r0, d, V, sign, lay_name)
    want = co.curvature(V, r0, d, F, sign)
    for q, name in enumerate(co.NAMES):
        bad = np.count_nonzero(got[:, q].view(np.uint32) != want[q].view(np.uint32))
        assert bad == 0, "%s: %d of %d values differ" % (name, bad, V.shape[0])
    assert summ == co.summary(want), (summ, co.summary(want))
    return got


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("grid", list(cc.SHAPES))
def test_host_build_of_the_kernel_text_equals_the_oracle(host_program, tmp_path, grid, dtype):
    """made-up vertices with 1, 2, 4 and 8 nodes, clamped and NaN rows, on every sample type at a padded pitch and slice"""
    shape = cc.SHAPES[grid]
    F = cc.field(dtype, shape)
    V = cc.made_up_vertices(shape, cc.AWKWARD_R0, cc.AWKWARD_D, cc.real_of(dtype))
    got = check_host(host_program, str(tmp_path), F, cc.AWKWARD_R0, cc.AWKWARD_D, V)
    assert np.isnan(got).any() and np.isfinite(got).any()
    check_host(host_program, str(tmp_path), F, cc.AWKWARD_R0, cc.AWKWARD_D, V, sign=-1, lay_name="dense")


def test_host_build_on_the_hand_cases(host_program, tmp_path):
    F = hand_field()
    V = np.array([v for v, _ in HAND], np.float32)
    got = check_host(host_program, str(tmp_path), F, *UNIT, V)
    assert np.array_equal(got.view(np.uint32), np.stack([closed_form(g, HAND_H) for _, g in HAND]).view(np.uint32))
    F, G, V = planted()
    a, b = check_host(host_program, str(tmp_path), F, *UNIT, V), check_host(host_program, str(tmp_path), G, *UNIT, V)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    _, summ = run_host_case(host_program, str(tmp_path), symmetric_field(), *UNIT, np.array([[1.0, 1.0, 1.0], [1.5, 1.0, 1.0]], np.float32))
    assert (summ.finite, summ.undefined) == (1, 1)


def test_host_build_refuses_what_the_call_refuses(host_program, tmp_path):
    F = cc.field("f32", (3, 3, 3))
    V = np.zeros((1, 3), np.float32)
    for bad_shape, sign in (((2, 3, 3), 1), ((3, 2, 3), 1), ((3, 3, 2), 1), ((3, 3, 3), 0), ((3, 3, 3), 2)):
        with pytest.raises(AssertionError, match="refused"):
            run_host_case(host_program, str(tmp_path), cc.field("f32", bad_shape) if bad_shape != (3, 3, 3) else F, *UNIT, V, sign)


@pytest.mark.parametrize("dtype", TYPES)
def test_host_build_under_the_sanitizers(host_program_sanitized, tmp_path, dtype):
    """ASan and UBSan on the stand-alone program: the source buffer begins with the first grid point and ends with the last, so a
    sample read outside the grid stops the program"""
    for grid in cc.SHAPES:
        shape = cc.SHAPES[grid]
        F = cc.field(dtype, shape, seed=1)
        V = cc.made_up_vertices(shape, cc.AWKWARD_R0, cc.AWKWARD_D, cc.real_of(dtype), seed=1)
        for lay in ("dense", "all"):
            check_host(host_program_sanitized, str(tmp_path), F, cc.AWKWARD_R0, cc.AWKWARD_D, V, lay_name=lay)
    V = cc.divergent_vertices(cc.SHAPES["9x8x7"], cc.AWKWARD_R0, cc.AWKWARD_D, cc.real_of(dtype))
    check_host(host_program_sanitized, str(tmp_path), cc.field(dtype, cc.SHAPES["9x8x7"]), cc.AWKWARD_R0, cc.AWKWARD_D, V, lay_name="dense")
