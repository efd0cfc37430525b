"""The contour spectrum of the grid, the part that needs no GPU.

The oracle facts pin tests/spectrum_oracle.py itself and pass without the feature.  The product is held to that oracle by the
tests behind them, which fail without the feature: MC33_isovalue_ladder (host C in every library), the names, exports and struct
layouts, the k_sp_* kernels in the code objects, the host-logic build of mc33_capi.c (its emulated device layer has no spectrum),
the kernel's own text - the __host__ __device__ functions of mc33_spectrum.hip.h - compiled for the host into a stand-alone
program (tests/spectrum_host.cpp) that runs the case table of tests/test_gpu_spectrum.py, once more under ASan and UBSan; the host
layer's slabs on a stub device layer (tests/spectrum_capi_stub.c); and slabs.reduce_spectrum on gloo."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import layouts
import spectrum_cases as sc
import spectrum_oracle as so
from mc33_capi import MC33Lib, product_path
from mc33_c_library_amd.api import SpectrumInfo
from mesh_checks import assert_exported, assert_kernels, host_logic, kernels_of
from spectrum_cases import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_spectrum.hip.h")

HIP_NAMES = ["mc33hip_grid_spectrum"]
C_NAMES = ["MC33_grid_spectrum", "MC33_isovalue_ladder"]
TYPES = sc.TYPES


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------

def _nan_field():
    """6 x 7 x 9 floats with NaNs of both signs, both infinities and both zeros"""
    return sc.field("special", "f32", (6, 7, 9), seed=1)


def test_oracle_equals_the_corner_test_at_every_isovalue():
    F = _nan_field()
    assert np.isnan(F).any() and np.signbit(F[np.isnan(F)]).any() and not np.signbit(F[np.isnan(F)]).all()
    isos = [-0.75, -0.25, 0.0, 0.125, 0.5, 0.99]
    got = so.spectrum(F, isos)
    assert [int(x) for x in got.cut_cells] == [so.brute_cut_cells(F, v) for v in isos]
    assert got.cells == 5 * 6 * 8 and got.points == F.size and int(got.histogram.sum()) == F.size
    assert got.nan_samples == int(np.isnan(F).sum()) and got.sample_min == -np.inf and got.sample_max == np.inf
    for dtype in ("u8", "u16", "u32", "f64"):   # integer isovalues that equal samples; double isovalues two floats cannot tell apart
        G = sc.field("plateau", dtype, (5, 4, 6))
        isos = [1.0, 2.0, 2.0 + 2.0 ** -30, 3.0] if dtype == "f64" else [1.0, 2.0, 3.0]
        assert [int(x) for x in so.spectrum(G, isos).cut_cells] == [so.brute_cut_cells(G, v) for v in isos]


def test_oracle_ranks():
    v = so.convert_isovalues([-1.0, 0.0, 2.0], np.float32)
    nan = np.float32(np.nan)
    F = np.array([-np.inf, -1.0, -0.5, -0.0, 0.0, 1e-45, 2.0, 2.5, np.inf, np.copysign(nan, 1), np.copysign(nan, -1)], np.float32)
    assert so.ranks(F, v).tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 3, 0, 3]
    assert so.convert_isovalues([0.0, 1.0, np.nan], np.float32) is None and so.convert_isovalues([1.0, 1.0], np.float32) is None
    assert so.convert_isovalues([1.0, 1.0 + 2.0 ** -40], np.float32) is None and so.convert_isovalues([1.0, 1.0 + 2.0 ** -40], np.float64) is not None
    assert so.convert_isovalues(list(range(256)), np.float32) is None and so.convert_isovalues([-np.inf, np.inf], np.uint8) is not None


@pytest.mark.parametrize("parts", [1, 3, 8])
def test_oracle_ranges_add_up_to_the_whole_grid(parts):
    F = _nan_field()
    isos = [-0.5, 0.0, 0.5]
    whole = so.spectrum(F, isos)
    ranges = sc.split(F.shape[0] - 1, parts)
    assert ranges[0][0] == 0 and ranges[-1][1] == F.shape[0] - 1 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert so.same(so.add(so.spectrum(F, isos, a, b) for a, b in ranges), whole)
    assert so.spectrum(F, isos, 0, 2).points == 2 * 6 * 7   # (the plane above a range that stops short belongs to the next)


def test_oracle_without_isovalues_and_on_nothing_but_nans():
    F = _nan_field()
    got = so.spectrum(F, [])
    assert got.cut_cells.size == 0 and got.histogram.tolist() == [F.size] and got.sample_max == np.inf
    got = so.spectrum(np.full((2, 2, 2), np.nan, np.float32), [0.0])
    assert got.histogram.tolist() == [8, 0] and (got.sample_min, got.sample_max, got.nan_samples) == (np.inf, -np.inf, 8) and got.cut_cells.tolist() == [0]


def test_case_table_reaches_what_it_names():
    assert sc.SHAPES["one_point_beyond"] == (66, 18, 34) and sc.SHAPES["tile_minus_1_beyond"] == (128, 32, 64)
    assert sorted(sc.SHAPES[k][0] % 4 for k in ("dword_plus_1", "dword_plus_2", "dword_plus_3")) == [1, 2, 3]
    assert all(np.prod(s) <= 2_000_000 and max(s) <= 1100 for s in sc.SHAPES.values())
    for dtype in TYPES:
        for name in sc.cases_of(dtype):
            F, isos, want = sc.case(name, dtype)
            assert int(want.histogram.sum()) == want.points == F.size
    F, isos, want = sc.case("plateau_isovalues_equal_samples", "u8")
    assert set(isos) <= set(float(x) for x in np.unique(F))
    assert sc.case("constant", "f32")[2].cut_cells.tolist() == [0, 0, 0] and sc.case("constant", "f32")[2].histogram.tolist() == [0, 60, 0, 0]
    assert (sc.case("n_255_noise", "f32")[2].histogram > 0).all() and (sc.case("one_point_beyond_noise", "u16")[2].cut_cells > 0).all()
    F = sc.case("special_values", "f64")[0]
    assert np.isinf(F).any() and (F == 0).any() and np.signbit(F[F == 0]).any() and not np.signbit(F[F == 0]).all()


# ---- MC33_isovalue_ladder of the product: host C, no device --------------------------------------------------------------------------

def _ladder_fn(dtype):
    path = product_path(dtype)
    assert os.path.exists(path), "build the HIP libraries first (python -m mc33_c_library_amd.build)"
    lib = MC33Lib(path, dtype)
    fn = lib.lib.MC33_isovalue_ladder
    return lib, fn


@pytest.mark.parametrize("dtype", ["f32", "u8", "f64"])
def test_isovalue_ladder_of_the_library_equals_its_formula(dtype):
    lib, fn = _ladder_fn(dtype)
    for lo, hi, n in ((0.0, 1.0, 3), (-3.0, 3.0, 64), (0.0, 255.0, 255), (-1e30, 1e30, 8), (1.0, 1.0 + 2.0 ** -20, 7), (5.0, 6.0, 0), (0.1, 0.7, 1)):
        buf = (lib.real * 256)(*([-7.0] * 256))
        want = so.ladder(lo, hi, n, lib.np_dtype)
        assert want is not None and fn(lo, hi, n, buf) == n, (lo, hi, n)
        got = np.array([buf[k] for k in range(n)], lib.np_real)
        assert got.tobytes() == want.tobytes(), (lo, hi, n)
        assert all(buf[k] == -7.0 for k in range(n, 256))
        assert n == 0 or (lo < got[0] and got[-1] < hi)
    buf = (lib.real * 256)()
    inf, nan = float("inf"), float("nan")
    for lo, hi, n in ((0.0, inf, 3), (-inf, 0.0, 3), (nan, 1.0, 3), (0.0, nan, 3), (1.0, 1.0, 3), (2.0, 1.0, 3), (0.0, 1.0, 256), (0.0, 1.0, 0xFFFFFFFF)):
        assert fn(lo, hi, n, buf) == -1 and so.ladder(lo, hi, n, lib.np_dtype) is None, (lo, hi, n)
    assert fn(0.0, 1.0, 3, None) == -1
    if dtype != "f64":   # steps closer than a float resolves
        assert fn(1.0, 1.0 + 2.0 ** -20, 255, buf) == -1 and so.ladder(1.0, 1.0 + 2.0 ** -20, 255, np.float32) is None
    from mc33_c_library_amd import isovalue_ladder
    assert isovalue_ladder(-3.0, 3.0, 9, dtype) == [float(x) for x in so.ladder(-3.0, 3.0, 9, lib.np_dtype)]
    with pytest.raises(ValueError):
        isovalue_ladder(1.0, 1.0, 3, dtype)
    with pytest.raises(ValueError):
        isovalue_ladder(0.0, 1.0, 256, dtype)


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_grid_spectrum\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_spectrum;", hip)
    assert re.search(r"\bint MC33_grid_spectrum\(MC33 \*", pub) and re.search(r"\bint MC33_isovalue_ladder\(double ", pub) and re.search(r"\} mc33_spectrum_info;", pub)
    import mc33_c_library_amd as pkg
    from mc33_c_library_amd import slabs
    assert set(HIP_NAMES) <= set(pkg.HIP_API) and set(C_NAMES) <= set(pkg.REFERENCE_API)
    assert callable(pkg.DeviceGrid.spectrum) and callable(pkg.DeviceGrid.spectrum_ladder) and callable(pkg.isovalue_ladder) and pkg.GridSpectrum
    assert callable(slabs.reduce_spectrum)
    # the constants tests/spectrum_cases.py restates are the header's
    text = open(HEADER).read()
    assert re.search(r"constexpr int SP_TILE_X = %d, SP_TILE_Y = %d;" % (sc.SP_TILE_X, sc.SP_TILE_Y), text)
    assert re.search(r"constexpr int SP_ZCHUNK = %d;" % sc.SP_ZCHUNK, text) and re.search(r"constexpr int SP_THREADS = %d;" % sc.SP_THREADS, text)
    assert re.search(r"constexpr int SP_MAX_ISOS = %d;" % so.MAX_ISOS, text)
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert kernels.rstrip().endswith('#include "mc33_spectrum.hip.h"') and "k_sp_spectrum" in kernels


@pytest.mark.parametrize("dtype", TYPES)
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", TYPES)
def test_spectrum_kernels_are_in_the_code_object(dtype):
    ctype = {"f32": "float", "f64": "double", "u8": "unsigned char", "u16": "unsigned short", "u32": "unsigned int"}[dtype]
    pack = {"u8": 4, "u16": 2}.get(dtype)
    ks = kernels_of(dtype)
    mine = sorted(n for n in ks if n.startswith("k_sp_"))
    want = ["k_sp_init", "k_sp_spectrum<%s, 1>" % ctype] + (["k_sp_spectrum<%s, %d>" % (ctype, pack)] if pack else [])
    assert mine == sorted(want), (mine, sorted(ks))
    assert_kernels(dtype, mine, max_vgprs=96)
    for name in mine:  # every counter, the isovalues and both rank planes in LDS: eight blocks and more to a CU
        assert ks[name]["group_segment_fixed_size"] <= 8192, (name, ks[name])


# ---- the host-logic build: mc33_capi.c on a device layer without a spectrum ------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_the_spectrum(dtype):
    """MC33_grid_spectrum returns -1 whatever it is given, writes nothing, and leaves the object byte for byte as it was; the
    ladder is host C and works."""
    with host_logic(dtype, n=12) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        nV, nT = C.c_uint(), C.c_uint()
        L.size_of_isosurface(M, lib.real(iso), C.byref(nV), C.byref(nT))
        assert nV.value > 0
        before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
        isos = (lib.real * 3)(iso - 1, iso, iso + 1)
        cut = (C.c_ulonglong * 3)(*[0xA5A5] * 3)
        hist = (C.c_ulonglong * 4)(*[0xA5A5] * 4)
        info = SpectrumInfo(1, 2, 3, 4.0, 5.0)
        for n in (3, 1, 0):
            assert L.MC33_grid_spectrum(M, isos, n, cut, hist, C.byref(info)) == -1
        assert L.MC33_grid_spectrum(M, isos, 3, cut, hist, None) == -1 and L.MC33_grid_spectrum(None, isos, 3, cut, hist, C.byref(info)) == -1
        assert list(cut) == [0xA5A5] * 3 and list(hist) == [0xA5A5] * 4 and (info.points, info.cells, info.nan_samples, info.sample_min, info.sample_max) == (1, 2, 3, 4.0, 5.0)
        assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        n2, t2 = C.c_uint(), C.c_uint()
        L.size_of_isosurface(M, lib.real(iso), C.byref(n2), C.byref(t2))
        assert (n2.value, t2.value) == (nV.value, nT.value)
        buf = (lib.real * 8)()
        assert L.MC33_isovalue_ladder(0.0, 1.0, 3, buf) == 3 and [buf[k] for k in range(3)] == [0.25, 0.5, 0.75]


# ---- the kernel's text compiled for the host ---------------------------------------------------------------------------------------------

HOST_FLAGS = ["-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra"]
# (the sanitizers' runtimes linked statically: the programs stand alone, whatever else the environment loads into a process)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spectrum_host") / "spectrum_host")
    subprocess.check_call(["g++"] + HOST_FLAGS + [os.path.join(HERE, "spectrum_host.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def host_program_sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: stand-alone, with its own main"""
    out = str(tmp_path_factory.mktemp("spectrum_host_san") / "spectrum_host_san")
    subprocess.check_call(["g++"] + HOST_FLAGS + SANITIZE + [os.path.join(HERE, "spectrum_host.cpp"), "-o", out])
    return out


def packed_allowed(itemsize, lay):
    """the predicate of the device layer: base, pitch and slice multiples of 4 bytes (the buffer itself is 16-byte aligned)"""
    return itemsize < 4 and all(v * itemsize % 4 == 0 for v in lay)


def run_host_case(program, tmp, F, isos, lay_name="dense", pack=1, rng=None):
    """the grid through the host program, in a poisoned buffer that ends with the last byte the call may read: the last grid
    point, or - packed form - the end of the dword that holds it"""
    it = F.dtype.itemsize
    npz, npy, npx = F.shape
    lay = layouts.layout(lay_name, F.shape, it)
    if pack > 1:
        assert packed_allowed(it, lay), (lay_name, lay)
    flat = layouts.place(F, lay, isos)
    last_row = lay[2] + (npz - 1) * lay[1] + (npy - 1) * lay[0]
    end = last_row + (-(-npx // pack) * pack if pack > 1 else npx)
    assert end <= last_row + lay[0]
    flat = flat[:end].copy()
    zb, ze = rng or (0, npz - 1)
    head = [sc.TYPE_CODE[{v: k for k, v in sc.NP_DTYPES.items()}[F.dtype.type]], npx, npy, npz, lay[0], lay[1], lay[2], pack, zb, ze, int(ze == npz - 1), len(isos)]
    cf, of = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    with open(cf, "wb") as f:
        f.write(np.array(head, np.int64).tobytes())
        f.write(np.array(list(isos) + [0.0] * (255 - len(isos)), np.float64).tobytes())
        f.write(np.array([flat.size], np.int64).tobytes())
        f.write(flat.tobytes())
    r = subprocess.run([program, cf, of], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(of, "rb").read()
    assert len(raw) == 256 * 8 * 2 + 8 + 16
    n = len(isos)
    hist = np.frombuffer(raw, np.uint64, 256)
    diff = np.frombuffer(raw, np.int64, 256, 2048)
    nan, = struct.unpack_from("Q", raw, 4096)
    lo, hi = struct.unpack_from("dd", raw, 4104)
    assert not hist[n + 1:].any() and not diff[n + 1:].any() and int(diff.sum()) == 0
    planes = ze - zb + int(ze == npz - 1)
    return so.Spectrum(np.cumsum(diff)[:n].astype(np.uint64), hist[:n + 1].copy(), npx * npy * planes, (npx - 1) * (npy - 1) * (ze - zb), nan, lo, hi), r.stdout


@pytest.mark.parametrize("name", list(sc.CASES))
def test_host_build_of_the_kernel_text_equals_the_oracle(host_program, tmp_path, name):
    F, isos, want = sc.case(name, "f32")
    got, said = run_host_case(host_program, str(tmp_path), F, isos)
    assert so.same(got, want), report(got, want)
    if "one_point_beyond" in sc.CASES[name][0]:
        assert said.startswith("2 x 2 tiles, 2 chunks, 8 items on 3 blocks"), said


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", ["one_point_beyond_noise", "dword_plus_1_cos", "dword_plus_2_noise", "dword_plus_3_noise", "narrow_dword_plus_1_cos",
                                  "narrow_dword_plus_3_noise", "plateau_isovalues_equal_samples", "n_255_noise", "n_0", "tile_minus_1_beyond_cos"])
def test_host_build_on_every_sample_type_and_form(host_program, tmp_path, name, dtype):
    """all five sample types, in the layout whose pitch is odd (one sample per load) and - 1- and 2-byte samples - in layouts
    that allow the packed form, which is then the one that runs"""
    F, isos, want = sc.case(name, dtype)
    got, _ = run_host_case(host_program, str(tmp_path), F, isos, "padx_odd")
    assert so.same(got, want), report(got, want)
    if F.dtype.itemsize < 4:
        for lay in ("padx16", "padx4", "pady"):
            got, _ = run_host_case(host_program, str(tmp_path), F, isos, lay, pack=4 // F.dtype.itemsize)
            assert so.same(got, want), (lay, report(got, want))


@pytest.mark.parametrize("dtype", TYPES)
def test_host_build_on_ranges(host_program, tmp_path, dtype):
    F, isos, want = sc.case("one_point_beyond_noise", dtype)
    pack = 4 // F.dtype.itemsize if F.dtype.itemsize < 4 else 1
    parts = []
    for a, b in sc.split(F.shape[0] - 1, 3) + [(0, 1), (F.shape[0] - 2, F.shape[0] - 1)]:
        got, _ = run_host_case(host_program, str(tmp_path), F, isos, "padx16", pack=pack, rng=(a, b))
        assert so.same(got, so.spectrum(F, isos, a, b)), (a, b)
        parts.append(got)
    assert so.same(so.add(parts[:3]), want)


@pytest.mark.parametrize("dtype", TYPES)
def test_host_build_under_the_sanitizers(host_program_sanitized, tmp_path, dtype):
    """ASan and UBSan on the stand-alone program: the source buffer ends with the last readable byte, so a load beyond the readable
    extent of include/mc33_hip.h - or a rank byte outside its plane, a counter outside its array - stops the program"""
    names = ["dword_plus_1_cos", "dword_plus_2_noise", "dword_plus_3_noise", "narrow_dword_plus_3_noise", "one_point_beyond_noise", "n_255_noise"]
    names += ["special_values", "infinite_isovalues"] if dtype in ("f32", "f64") else []
    for name in names:
        F, isos, want = sc.case(name, dtype)
        for lay in ("dense", "all"):
            got, _ = run_host_case(host_program_sanitized, str(tmp_path), F, isos, lay)
            assert so.same(got, want), (name, lay, report(got, want))
        if F.dtype.itemsize < 4:
            for lay in ("padx4", "padx16"):
                got, _ = run_host_case(host_program_sanitized, str(tmp_path), F, isos, lay, pack=4 // F.dtype.itemsize)
                assert so.same(got, want), (name, lay, report(got, want))
    F, isos, want = sc.case("one_point_beyond_noise", dtype)
    got, _ = run_host_case(host_program_sanitized, str(tmp_path), F, isos, "dense", rng=(1, 2))
    assert so.same(got, so.spectrum(F, isos, 1, 2))


# ---- the host layer's slabs on a stub device layer -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("flavour", ["f32", "u16_ortho", "f64"])
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_layer_adds_three_slabs_on_a_stub_device_layer(tmp_path, flavour, sanitized):
    """tests/spectrum_capi_stub.c: mc33_capi.c as it ships with MC33_HIP_DEVICES=0,0,0 on a device layer on the heap - the slabs'
    ranges tile the grid, sums and extremes are those of the whole grid on one slab, a changed grid is uploaded first, a failing
    slab gives -1 with nothing written; stand-alone, the second time under ASan (which also reports what was left allocated) and UBSan."""
    csrc = os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_capi.c")
    cdef = {"f32": [], "u16_ortho": ["-DINTEGER_GRD", "-DGRD_TYPE_SIZE=2", "-DGRD_ORTHOGONAL"], "f64": ["-DGRD_TYPE_SIZE=8"]}[flavour]
    san = ["-g"] + SANITIZE if sanitized else []
    out = str(tmp_path / "capi_stub")
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-std=c11", "-Wall", "-Wextra"] + san + cdef +
                          [csrc, os.path.join(HERE, "spectrum_capi_stub.c"), "-o", out, "-lm", "-lpthread"])
    env = {k: v for k, v in os.environ.items() if k not in ("MC33_HIP_DEVICES", "MC33_HIP_REUPLOAD")}
    r = subprocess.run([out], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]


# ---- slabs.reduce_spectrum on gloo, world 2 --------------------------------------------------------------------------------------------------

WORKER = textwrap.dedent('''
    import sys
    import numpy as np
    import torch.distributed as dist
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    from mc33_c_library_amd.api import GridSpectrum
    from mc33_c_library_amd.slabs import reduce_spectrum
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    big = 2 ** 63 + 5   # (beyond int64: the words travel as bit patterns)
    mine = [GridSpectrum([0.5, 1.5], np.array([3, big], np.uint64), np.array([1, 2, 3], np.uint64), 6, 2, 1, -2.5, 7.0),
            GridSpectrum([0.5, 1.5], np.array([4, 1], np.uint64), np.array([10, 0, 2 ** 40], np.uint64), 12, 4, 0, -0.5, float("inf"))][rank]
    got = reduce_spectrum(mine)
    assert got.isovalues == [0.5, 1.5] and got.cut_cells.dtype == np.uint64 and got.histogram.dtype == np.uint64
    assert got.cut_cells.tolist() == [7, big + 1] and got.histogram.tolist() == [11, 2, 2 ** 40 + 3]
    assert (got.points, got.cells, got.nan_samples, got.sample_min, got.sample_max) == (18, 6, 1, -2.5, float("inf"))
    none = reduce_spectrum(GridSpectrum([], np.zeros(0, np.uint64), np.array([rank + 1], np.uint64), rank + 1, 1, rank + 1, float("inf"), float("-inf")))
    assert none.histogram.tolist() == [3] and (none.sample_min, none.sample_max, none.nan_samples) == (float("inf"), float("-inf"), 3)
    if rank == 0:
        print("REDUCE_OK")
    dist.destroy_process_group()
''') % (ROOT, HERE)


def test_reduce_spectrum_on_gloo_world_2(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29537", str(script)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "REDUCE_OK" in out.stdout
