"""Resampling the grid on the device before extraction, the part that needs no GPU.

The oracle facts pin tests/resample_oracle.py itself and pass without the feature.  The product is held to that oracle by the
tests behind them, which fail without the feature: MC33_gaussian_taps (host C in every library), the names, exports and struct
layouts, the k_rs_* kernels in the code objects, the host-logic build of mc33_capi.c (its emulated device layer cannot resample),
and the kernel's own text - the __host__ __device__ functions of mc33_resample.hip.h - compiled for the host into a stand-alone
program (tests/resample_host.cpp) that runs the case table of tests/test_gpu_resample.py bit for bit; and the host layer's own
handling of contexts and of the grid it owns, on a stub device layer (tests/resample_capi_stub.c)."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import layouts
import resample_cases as rc
import resample_oracle as ro
from mc33_capi import MC33Lib, product_path
from mc33_c_library_amd.api import GridResampling
from mesh_checks import assert_exported, assert_kernels, host_logic, kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_resample.hip.h")

HIP_NAMES = ["mc33hip_resampled_size", "mc33hip_resample_grid", "mc33hip_context_device"]
C_NAMES = ["MC33_gaussian_taps", "MC33_create_resampled", "MC33_resampled_grid"]
TYPES = ["f32", "u16", "u8", "u32", "f64"]
MAX_VGPRS = 64   # with identity taps eight blocks of four waves share a CU, eight waves on every SIMD - 64 registers per lane


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES)
def test_oracle_identity_returns_the_bytes(dtype):
    F = rc.finite_field(dtype, (9, 7, 5), seed=3)
    if dtype == "f32":
        F[0, 0, :4] = [-0.0, np.inf, -np.inf, 0.0]
    assert ro.same_bits(ro.resample(F), F)
    assert ro.same_bits(ro.resample(F, ([1.0], None, [1.0])), F)
    for s in ((2, 1, 1), (3, 2, 2), (4, 3, 2)):
        assert ro.same_bits(ro.resample(F, stride=s), F[::s[2], ::s[1], ::s[0]])


def test_oracle_is_a_correlation():
    F = rc.finite_field("f32", (9, 4, 3), seed=4)
    got = ro.resample(F, ([0.0, 0.0, 1.0], None, None))   # tap 2 multiplies the sample at offset +1
    want = np.concatenate([F[:, :, 1:], F[:, :, -1:]], axis=2)
    assert np.array_equal(got, want)
    got = ro.resample(F, (None, None, [1.0, 0.0, 0.0]))   # ... tap 0 the one at offset -1, along z
    assert np.array_equal(got, np.concatenate([F[:1], F[:-1]], axis=0))


@pytest.mark.parametrize("dtype", ["u8", "u16", "u32"])
def test_oracle_integer_clamps_and_nan(dtype):
    dt = rc.NP_DTYPES[dtype]
    top = int(np.iinfo(dt).max)
    z, y, x = np.indices((4, 4, 6))
    F = (((x + y + z) & 1) * top).astype(dt)
    got = ro.resample(F, (rc.CLAMPING, None, None))
    # inside a row: -0.5 MAX + 0 - 0.5 MAX < 0 -> 0 on the zeros, 2.5 MAX -> MAX on the others: the checkerboard again
    assert np.array_equal(got[:, :, 1:-1], F[:, :, 1:-1]) and set(np.unique(got)) == {0, top}
    assert ro.convert(np.array([np.nan, -1.0, 0.49, 0.5, 1.5, top - 0.5, top + 0.0, np.inf]), dt).tolist() == [0, 0, 0, 1, 2, top, top, top]
    Ff = np.ones((2, 2, 3), np.float32)
    Ff[0, 0, 1] = np.nan
    assert np.isnan(ro.resample(Ff, ([0.25, 0.5, 0.25], None, None))[0, 0]).all()


def test_oracle_sizes_and_geometry():
    assert [ro.out_points(n, s) for n, s in ((11, 3), (10, 3), (2, 1), (3, 2), (3, 3))] == [4, 4, 2, 2, 1]
    assert ro.geometry((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (2, 3, 1)) == ((1.0, 2.0, 3.0), (1.0, 0.75, 2.0))
    assert ro.resample(np.zeros((11, 10, 9), np.uint8), stride=(3, 3, 3)).shape == (4, 4, 3)


# ---- MC33_gaussian_taps of the product: host C, no device ------------------------------------------------------------------------------

def _taps_fn(dtype="f32"):
    path = product_path(dtype)
    assert os.path.exists(path), "build the HIP libraries first (python -m mc33_c_library_amd.build)"
    lib = MC33Lib(path, dtype).lib
    return lib.MC33_gaussian_taps


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_gaussian_taps_of_the_library_equal_the_oracle(dtype):
    fn = _taps_fn(dtype)
    for sigma in (0.0, 0.5, 1.0, 2.0, 8.0 / 3.0):
        for radius in (0, 1, 4, 8):
            buf = (C.c_double * 17)(*([-7.0] * 17))
            r = fn(sigma, radius, buf)
            want = ro.gaussian_taps(sigma, radius)
            assert want is not None and r == (len(want) - 1) // 2, (sigma, radius, r)
            got = [buf[k] for k in range(2 * r + 1)]
            assert struct.pack("%dd" % len(got), *got) == struct.pack("%dd" % len(want), *want), (sigma, radius, got, want)
            assert all(buf[k] == -7.0 for k in range(2 * r + 1, 17))
            if sigma:
                assert abs(sum(got) - 1.0) < 1e-15 * len(got) and got == got[::-1]
    assert [len(ro.gaussian_taps(s)) for s in (0.0, 0.5, 1.0, 2.0, 8.0 / 3.0)] == [1, 5, 7, 13, 17]
    buf = (C.c_double * 17)()
    for sigma, radius in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (3.0, 0), (1.0, 9), (float("inf"), 2), (-0.5, 3)):
        assert fn(sigma, radius, buf) == -1 and ro.gaussian_taps(sigma, radius) is None, (sigma, radius)
    assert fn(1.0, 0, None) == -1
    from mc33_c_library_amd import gaussian_taps
    assert gaussian_taps(1.0) == ro.gaussian_taps(1.0) and gaussian_taps(2.0, 3) == ro.gaussian_taps(2.0, 3) and gaussian_taps(0) == [1.0]
    with pytest.raises(ValueError):
        gaussian_taps(3.0)


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_resample_grid\(mc33hip_ctx \*", hip) and re.search(r"\bint mc33hip_resampled_size\(mc33hip_ctx \*", hip) and re.search(r"\bint mc33hip_context_device\(mc33hip_ctx \*", hip)
    assert re.search(r"\} mc33hip_resampling;", hip) and re.search(r"\} mc33_resampling;", pub)
    assert re.search(r"\bint MC33_gaussian_taps\(double ", pub) and re.search(r"\bMC33 \*MC33_create_resampled\(MC33 \*", pub)
    assert re.search(r"\b_GRD \*MC33_resampled_grid\(MC33 \*", pub)
    import mc33_c_library_amd as pkg
    assert set(HIP_NAMES) <= set(pkg.HIP_API) and set(C_NAMES) <= set(pkg.REFERENCE_API)
    assert callable(pkg.DeviceGrid.resampled) and callable(pkg.gaussian_taps) and pkg.Resampling and pkg.GridResampling
    # the constants tests/resample_cases.py restates are the header's
    text = open(HEADER).read()
    assert re.search(r"constexpr int RS_ZCHUNK = %d;" % rc.RS_ZCHUNK, text)
    assert re.search(r"constexpr int RS_TILE_X = %d, RS_TILE_Y = %d;" % (rc.RS_TILE_X, rc.RS_TILE_Y), text)


@pytest.mark.parametrize("dtype", TYPES)
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", TYPES)
def test_resampling_kernel_is_in_the_code_object(dtype):
    ctype = {"f32": "float", "f64": "double", "u8": "unsigned char", "u16": "unsigned short", "u32": "unsigned int"}[dtype]
    ks = kernels_of(dtype)
    mine = [n for n in ks if n.startswith("k_rs_")]
    assert mine == ["k_rs_resample<%s>" % ctype], (mine, sorted(ks))
    assert_kernels(dtype, mine, MAX_VGPRS)
    for name in mine:
        assert ks[name]["group_segment_fixed_size"] == 0, (name, ks[name])   # (all of its LDS is sized by the plan at launch)


# ---- the host-logic build: mc33_capi.c on a device layer that cannot resample ------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_resample(dtype):
    """MC33_create_resampled returns NULL for good and for refused structs, the source object is unchanged and extracts as before,
    and MC33_resampled_grid of an ordinary object is NULL."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        first = lib.copy_surface(S)
        L.free_surface_memory(S)
        before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
        d3, u3 = C.c_double * 3, C.c_uint * 3
        nan, inf = float("nan"), float("inf")
        cases = [GridResampling(d3(1, 1, 1), u3(0, 0, 0), u3(1, 1, 1)), GridResampling(d3(0, 0, 0), u3(0, 0, 0), u3(2, 2, 2)),
                 GridResampling(d3(-1, 1, 1), u3(0, 0, 0), u3(1, 1, 1)), GridResampling(d3(1, nan, 1), u3(0, 0, 0), u3(1, 1, 1)),
                 GridResampling(d3(1, 1, inf), u3(0, 0, 0), u3(1, 1, 1)), GridResampling(d3(3, 1, 1), u3(0, 0, 0), u3(1, 1, 1)),
                 GridResampling(d3(1, 1, 1), u3(0, 9, 0), u3(1, 1, 1)), GridResampling(d3(1, 1, 1), u3(0, 0, 0), u3(1, 0, 1)),
                 GridResampling(d3(0, 0, 0), u3(0, 0, 0), u3(1, 1, 19))]
        for r in cases:
            assert not L.MC33_create_resampled(M, C.byref(r))
            assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        assert not L.MC33_create_resampled(M, None) and not L.MC33_create_resampled(None, C.byref(cases[0]))
        assert not L.MC33_resampled_grid(M) and not L.MC33_resampled_grid(None)
        assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        again = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert np.array_equal(again.T, first.T) and ro.same_bits(again.V, first.V) and ro.same_bits(again.N, first.N)


# ---- the kernel's text compiled for the host ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resample_host") / "resample_host")
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "resample_host.cpp"), "-o", out])
    return out


def write_case(path, dtype, F, taps, stride, src_flat, src_lay, dst_flat, dst_lay):
    npz, npy, npx = F.shape
    w = np.zeros((3, 17))
    nt = []
    for a in range(3):
        t = [1.0] if taps[a] is None else taps[a]
        w[a, :len(t)] = t
        nt.append(len(t))
    head = [rc.TYPE_CODE[dtype], npx, npy, npz] + nt + [int(s) for s in stride] + [src_lay[0], src_lay[1], src_lay[2], dst_lay[0], dst_lay[1], dst_lay[2]]
    with open(path, "wb") as f:
        f.write(np.array(head, np.int64).tobytes())
        f.write(w.tobytes())
        for flat in (src_flat, dst_flat):
            f.write(np.array([flat.size], np.int64).tobytes())
            f.write(flat.tobytes())


SEEN_TILES = {}   # case -> the tile the program reported


def run_host_case(program, tmp, name, dtype, src_layout="dense", dst_layout="all"):
    """the case through the host program: the source in a poisoned buffer that ends with its last grid point, the output inside
    a canary that ends with ITS last grid point; returns (output grid, every other sample of the output buffer, the canary)"""
    F, taps, stride, want = rc.case(name, dtype)
    it = F.dtype.itemsize
    sl = layouts.layout(src_layout, F.shape, it)
    src = layouts.place(F, sl, [0.0])
    src = src[:sl[2] + (F.shape[0] - 1) * sl[1] + (F.shape[1] - 1) * sl[0] + F.shape[2]].copy()   # nothing behind the last grid point
    dl = layouts.layout(dst_layout, want.shape, it)
    n = dl[2] + (want.shape[0] - 1) * dl[1] + (want.shape[1] - 1) * dl[0] + want.shape[2]
    canary = np.array([0xA5] * it, np.uint8).view(F.dtype)[0]
    dst = np.full(n, canary, F.dtype)
    cf, of = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    write_case(cf, dtype, F, taps, stride, src, sl, dst, dl)
    said = subprocess.check_output([program, cf, of], text=True)
    m = re.match(r"tile (\d+) x (\d+),", said)
    SEEN_TILES[name] = (int(m.group(1)), int(m.group(2)))
    out = np.fromfile(of, F.dtype)
    assert out.size == n
    got = np.array(layouts.host_view(out, want.shape, dl))
    mask = np.ones(n, bool)
    np.lib.stride_tricks.as_strided(mask[dl[2]:], want.shape, (dl[1], dl[0], 1))[...] = False
    return got, out[mask], canary, want


@pytest.mark.parametrize("name", list(rc.CASES))
def test_host_build_of_the_kernel_text_equals_the_oracle(host_program, tmp_path, name):
    got, rest, canary, want = run_host_case(host_program, str(tmp_path), name, "f32")
    assert ro.same_bits(got, want), "%s: %d of %d samples differ" % (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()), want.size)
    assert np.all(rest.view(np.uint8) == 0xA5), "a sample that is no output grid point was written"
    if name in rc.TILES:   # the case reaches the tile - and with it the branch of rs_cols / rs_emit - its name promises
        assert SEEN_TILES[name] == rc.TILES[name], (name, SEEN_TILES[name])


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", list(rc.ALL_TYPE_CASES))
def test_host_build_on_every_sample_type(host_program, tmp_path, name, dtype):
    got, rest, canary, want = run_host_case(host_program, str(tmp_path), name, dtype, src_layout="padx_odd", dst_layout="padx16")
    assert ro.same_bits(got, want)
    assert np.all(rest.view(np.uint8) == 0xA5)
    if want.dtype.kind == "u":
        top = np.iinfo(want.dtype).max
        assert (want == 0).any() and (want == top).any()   # both clamps are hit
    else:
        assert np.isnan(want).any() and np.isinf(want).any()


# ---- the host layer's handling of contexts and of the grid it owns, on a stub device layer -----------------------------------------------

@pytest.mark.parametrize("flavour", ["f32", "u16_ortho"])
def test_host_layer_creates_resamples_and_frees_on_a_stub_device_layer(tmp_path, flavour):
    """tests/resample_capi_stub.c: mc33_capi.c as it ships with a device layer on the heap that refuses a dead context, a context
    destroyed with the resampled grid still allocated through it, and anything left allocated at the end - MC33_create_resampled
    (on the device the source's context resolved), the source freed first, MC33_resampled_grid, a second resampling, free_MC33."""
    csrc = os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_capi.c")
    cdef = ["-DINTEGER_GRD", "-DGRD_TYPE_SIZE=2", "-DGRD_ORTHOGONAL"] if flavour == "u16_ortho" else []
    out = str(tmp_path / "capi_stub")
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-std=c11", "-Wall", "-Wextra"] + cdef +
                          [csrc, os.path.join(ROOT, "tests", "resample_capi_stub.c"), "-o", out, "-lm", "-lpthread"])
    assert subprocess.check_output([out], text=True).strip() == "ok"
