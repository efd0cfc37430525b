"""Rank-filtering the grid on the device, the part that needs no GPU.

The oracle facts pin tests/rank_oracle.py itself - against windows written out by hand, and against two properties of rank filters
- and pass without the feature.  The product is held to that oracle by the tests behind them, which fail without the feature: the
names, exports and constants, the k_rk_* kernels in the code objects, the host-logic build of mc33_capi.c (its emulated device
layer cannot rank), and the kernels' own text - the __host__ __device__ functions of mc33_rank.hip.h - compiled for the host
into a stand-alone program (tests/rank_host.cpp) that runs the case table of tests/test_gpu_rank.py bit for bit, every phase in
both lane orders, with the buffers cut behind their last grid point and the output inside a canary."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import layouts
import rank_cases as kc
import rank_oracle as ko
from mc33_c_library_amd import api
from mesh_checks import assert_exported, assert_kernels, host_logic, kernels_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_rank.hip.h")

HIP_NAMES = ["mc33hip_rank_grid"]
C_NAMES = ["MC33_create_ranked", "MC33_create_resampled", "MC33_resampled_grid"]
TYPES = ["f32", "u16", "u8", "u32", "f64"]
CTYPE = {"f32": "float", "f64": "double", "u8": "unsigned char", "u16": "unsigned short", "u32": "unsigned int"}
MEDIANS = [(1, 1), (3, 1), (9, 1), (1, 3), (3, 3), (9, 3)]   # (window points in a plane, planes) of the k_rk_median instances
# the 27-point selection holds 15 keys and the fetch 10 more; 128 registers keep four waves - a block - on every SIMD.
# The 64-bit keys of a double grid take two registers each: 168 keep three waves there.
MAX_VGPRS = {"f32": 128, "u16": 128, "u8": 128, "u32": 128, "f64": 168}


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------

def f32(*bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_oracle_key_order_is_the_definitions():
    """NaN with the sign bit, -inf, ..., -0, +0, ..., +inf, NaN without the sign bit; and keys turn back into the same bytes"""
    order = f32(0xFFC00123, 0xFF800001, 0xFF800000, 0xC0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x40000000, 0x7F800000, 0x7F800001, 0x7FC00001)
    k = ko.keys(order)
    assert k.dtype == np.uint32 and np.all(k[1:] > k[:-1])
    assert ko.same_bits(ko.samples(k, np.float32), order)
    d = np.array([0xFFF8000000000123, 0xFFF0000000000000, 0xBFF0000000000000, 0x8000000000000000, 0, 0x3FF0000000000000, 0x7FF0000000000000, 0x7FF8000000000001], np.uint64).view(np.float64)
    kd = ko.keys(d)
    assert kd.dtype == np.uint64 and np.all(kd[1:] > kd[:-1]) and ko.same_bits(ko.samples(kd, np.float64), d)
    for dt in (np.uint8, np.uint16, np.uint32):
        u = np.array([0, 1, np.iinfo(dt).max], dt)
        assert ko.keys(u).dtype == dt and np.array_equal(ko.keys(u), u) and ko.same_bits(ko.samples(ko.keys(u), dt), u)


def test_oracle_against_windows_written_out_by_hand():
    pz, nz, pn, nn = 0x00000000, 0x80000000, 0x7FC00001, 0xFFC00123   # +0, -0, NaN without and with the sign bit
    one, two, minf = 0x3F800000, 0x40000000, 0xFF800000
    row = f32(pz, nz, pn, one, nn, two).reshape(1, 1, 6)
    # along x, radius 1, edges replicated: the windows are (+0 +0 -0) (+0 -0 NaN) (-0 NaN 1) (NaN 1 -NaN) (1 -NaN 2) (-NaN 2 2)
    assert ko.same_bits(ko.rank_filter(row, "median", (1, 0, 0)), f32(pz, pz, one, one, one, two).reshape(1, 1, 6))
    assert ko.same_bits(ko.rank_filter(row, "min", (1, 0, 0)), f32(nz, nz, nz, nn, nn, nn).reshape(1, 1, 6))
    assert ko.same_bits(ko.rank_filter(row, "max", (1, 0, 0)), f32(pz, pn, pn, pn, two, two).reshape(1, 1, 6))
    # the same samples along y and along z
    for shape, radius in (((1, 6, 1), (0, 1, 0)), ((6, 1, 1), (0, 0, 1))):
        assert ko.same_bits(ko.rank_filter(row.reshape(shape), "median", radius), f32(pz, pz, one, one, one, two).reshape(shape))
    # a 2 x 2 plane, 3 x 3 windows: a replicated sample counts once for every offset that lands on it.  At (0, 0) the window
    # holds a four times, b and c twice, d once; with a < c < b < d the sorted window is a a a a c c b b d: the median is c
    a, b, c, d = minf, two, one, pn
    plane = f32(a, b, c, d).reshape(1, 2, 2)
    got = ko.rank_filter(plane, "median", (1, 1, 0))
    assert ko.same_bits(got, f32(c, b, c, b).reshape(1, 2, 2))   # (0,1): b x4, a x2, d x2, c: a a c b b b b d d -> b; (1,0): c x4: a a b c c c c d d -> c; (1,1): d x4, b x2, c x2, a: a c c b b d d d d -> b
    assert ko.same_bits(ko.rank_filter(plane, "min", (1, 1, 1)), f32(a, a, a, a).reshape(1, 2, 2))
    assert ko.same_bits(ko.rank_filter(plane, "max", (8, 8, 8)), f32(d, d, d, d).reshape(1, 2, 2))
    # radius 0: the bytes, payloads included
    assert ko.same_bits(ko.rank_filter(row, "median", (0, 0, 0)), row) and ko.same_bits(ko.rank_filter(row, "max", (0, 0, 0)), row)
    assert not ko.accepts(ko.MEDIAN, (2, 0, 0)) and not ko.accepts(ko.MIN, (0, 9, 0)) and not ko.accepts(3, (0, 0, 0)) and ko.accepts(ko.MAX, (8, 8, 8))


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_oracle_median_removes_isolated_spikes(dtype):
    """one constant apart from single-sample spikes, no two within Chebyshev distance 3: every 27-point window holds at most one
    spike, and its median is the constant - exactly, everywhere"""
    dt = kc.NP_DTYPES[dtype]
    F = np.full((17, 18, 19), 7, dt)
    spikes = [(z, y, x) for z in range(0, 17, 4) for y in range(1, 18, 4) for x in range(2, 19, 4)]
    for n, (z, y, x) in enumerate(spikes):
        F[z, y, x] = (np.inf, -np.inf, 1000.0, -5.0)[n % 4] if dt == np.float32 else (0, 65535)[n % 2]
    if dt == np.float32:
        assert (16, 17, 18) in spikes
        F.view(np.uint32)[16, 17, 18] = 0x7FC00001   # a NaN spike in a corner, where it is replicated 8 times in its own window
    got = ko.rank_filter(F, "median", (1, 1, 1))
    assert ko.same_bits(got, np.full(F.shape, 7, dt))


@pytest.mark.parametrize("dtype", TYPES)
def test_oracle_opening_never_exceeds_the_source(dtype):
    F = kc.field(dtype, (13, 11, 9), seed=5)
    opened = ko.rank_filter(ko.rank_filter(F, "min", (1, 2, 1)), "max", (1, 2, 1))
    closed = ko.rank_filter(ko.rank_filter(F, "max", (1, 2, 1)), "min", (1, 2, 1))
    assert np.all(ko.keys(opened) <= ko.keys(F)) and np.all(ko.keys(closed) >= ko.keys(F))
    assert not ko.same_bits(opened, F) and not ko.same_bits(closed, F)


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_rank_grid\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_ranking;", hip)
    assert re.search(r"\bMC33 \*MC33_create_ranked\(MC33 \*", pub) and re.search(r"\} mc33_ranking;", pub)
    for text, prefix in ((hip, "MC33HIP_RANK_"), (pub, "MC33_RANK_")):
        for word, value in (("MIN", ko.MIN), ("MEDIAN", ko.MEDIAN), ("MAX", ko.MAX)):
            assert re.search(r"#define %s%s +%d\b" % (prefix, word, value), text), prefix + word
    import mc33_c_library_amd as pkg
    assert "mc33hip_rank_grid" in pkg.HIP_API and "MC33_create_ranked" in pkg.REFERENCE_API
    assert callable(pkg.DeviceGrid.ranked) and callable(pkg.DeviceGrid.rank_into) and pkg.Ranking is api.Ranking
    # the struct and the signature are in the tables tests/test_bindings_cpu.py holds to the headers
    assert api.STRUCTS["mc33hip_ranking"] is api.Ranking and api.STRUCTS["mc33_ranking"] is api.Ranking
    assert api.SIGNATURES["mc33hip_rank_grid"][2] is False
    # the constants tests/rank_cases.py restates are the header's
    text = open(HEADER).read()
    assert re.search(r"constexpr int RK_ZCHUNK = %d;" % kc.RK_ZCHUNK, text)
    assert re.search(r"constexpr int RK_TILE_X = %d, RK_TILE_Y = %d;" % (kc.RK_TILE_X, kc.RK_TILE_Y), text)
    assert re.search(r"constexpr int RK_MINMAX_RADIUS = %d, RK_MEDIAN_RADIUS = %d;" % (ko.LIMIT[ko.MAX], ko.LIMIT[ko.MEDIAN]), text)
    from mc33_c_library_amd import build
    assert "mc33_rank.hip.h" in build.HIP_HEADERS
    assert "mc33_rank.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("dtype", TYPES)
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", TYPES)
def test_rank_kernels_are_in_the_code_object(dtype):
    ks = kernels_of(dtype)
    mine = sorted(n for n in ks if n.startswith("k_rk_"))
    want = sorted(["k_rk_minmax<%s>" % CTYPE[dtype]] + ["k_rk_median<%s, %d, %d>" % ((CTYPE[dtype],) + m) for m in MEDIANS])
    assert mine == want, (mine, sorted(ks))
    assert_kernels(dtype, mine, MAX_VGPRS[dtype])   # no private segment, no spilled register
    for name in mine:
        assert ks[name]["group_segment_fixed_size"] == 0, (name, ks[name])   # (all of its LDS is sized by the plan at launch)


# ---- the host-logic build: mc33_capi.c on a device layer that cannot rank ---------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_rank(dtype):
    """MC33_create_ranked returns NULL for good and for refused structs, the source object is unchanged and extracts as before"""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        L.MC33_create_ranked.restype, L.MC33_create_ranked.argtypes = C.POINTER(lib.MC33), [C.POINTER(lib.MC33), C.POINTER(api.Ranking)]
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        first = lib.copy_surface(S)
        L.free_surface_memory(S)
        before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
        u3 = C.c_uint * 3
        for r in (api.Ranking(u3(1, 1, 1), ko.MEDIAN), api.Ranking(u3(8, 8, 8), ko.MIN), api.Ranking(u3(2, 0, 0), ko.MEDIAN), api.Ranking(u3(0, 0, 9), ko.MAX),
                  api.Ranking(u3(0, 0, 0), 3), api.Ranking(u3(0, 0, 0), -1)):
            assert not L.MC33_create_ranked(M, C.byref(r))
            assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
        assert not L.MC33_create_ranked(M, None) and not L.MC33_create_ranked(None, C.byref(api.Ranking(u3(1, 1, 1), ko.MEDIAN)))
        assert not L.MC33_resampled_grid(M)
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        again = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert np.array_equal(again.T, first.T) and ko.same_bits(again.V, first.V) and ko.same_bits(again.N, first.N)


# ---- the kernels' text compiled for the host ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rank_host") / "rank_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "rank_host.cpp"), "-o", out])
    return out


def write_case(path, dtype, F, rank, radius, src_flat, src_lay, dst_flat, dst_lay):
    npz, npy, npx = F.shape
    head = [kc.TYPE_CODE[dtype], npx, npy, npz] + [int(r) for r in radius] + [int(rank)] + list(src_lay) + list(dst_lay) + [0, 0]
    assert len(head) == 16
    with open(path, "wb") as f:
        f.write(np.array(head, np.int64).tobytes())
        for flat in (src_flat, dst_flat):
            f.write(np.array([flat.size], np.int64).tobytes())
            f.write(flat.tobytes())


SEEN_TILES = {}   # case -> the tile the program reported


def run_host_case(program, tmp, name, dtype, src_layout="dense", dst_layout="all"):
    """the case through the host program, once per lane order: the source in a buffer of winning poison that ends with its last
    grid point, the output inside a canary that ends with ITS last grid point; returns [(output grid, every other sample of the
    output buffer)] and the oracle's grid"""
    F, rank, radius, want = kc.case(name, dtype)
    it = F.dtype.itemsize
    sl = layouts.layout(src_layout, F.shape, it)
    src = kc.place(F, sl, kc.poison(dtype, rank))   # (cut behind the last grid point)
    dl = layouts.layout(dst_layout, want.shape, it)
    canary = np.array([0xA5] * it, np.uint8).view(F.dtype)[0]
    dst = kc.place(np.full(F.shape, canary, F.dtype), dl, canary)
    n = dst.size
    cf, of = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
    write_case(cf, dtype, F, rank, radius, src, sl, dst, dl)
    outs = []
    for order in ("0", "1"):
        said = subprocess.check_output([program, cf, of, order], text=True)
        m = re.match(r"tile (\d+) x (\d+),", said)
        SEEN_TILES[name] = (int(m.group(1)), int(m.group(2)))
        out = np.fromfile(of, F.dtype)
        assert out.size == n
        got = np.array(layouts.host_view(out, want.shape, dl))
        mask = np.ones(n, bool)
        np.lib.stride_tricks.as_strided(mask[dl[2]:], want.shape, (dl[1], dl[0], 1))[...] = False
        outs.append((got, out[mask]))
    return outs, want


@pytest.mark.parametrize("name", list(kc.CASES))
def test_host_build_of_the_kernel_text_equals_the_oracle(host_program, tmp_path, name):
    outs, want = run_host_case(host_program, str(tmp_path), name, "f32", src_layout="padx_odd")
    for order, (got, rest) in enumerate(outs):
        assert ko.same_bits(got, want), "%s, lane order %d: %d of %d samples differ" % (name, order, int((got.view(np.uint32) != want.view(np.uint32)).sum()), want.size)
        assert np.all(rest.view(np.uint8) == 0xA5), "a sample that is no output grid point was written"
    if name in kc.TILES:   # the case reaches the tile its name promises
        assert SEEN_TILES[name] == kc.TILES[name], (name, SEEN_TILES[name])


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("name", list(kc.ALL_TYPE_CASES))
def test_host_build_on_every_sample_type(host_program, tmp_path, name, dtype):
    outs, want = run_host_case(host_program, str(tmp_path), name, dtype, src_layout="all", dst_layout="padx16")
    for got, rest in outs:
        assert ko.same_bits(got, want)
        assert np.all(rest.view(np.uint8) == 0xA5)
    F = kc.case(name, dtype)[0]
    if F.dtype.kind == "u":
        assert (F == 0).any() and (F == np.iinfo(F.dtype).max).any()
    else:
        bits = F.view(kc.SPECIAL_BITS[F.dtype].dtype)
        assert all((bits == b).any() for b in kc.SPECIAL_BITS[F.dtype])   # both infinities, both zeros, NaN of both signs
        assert np.isnan(want).any() or kc.case(name, dtype)[1] == kc.MEDIAN
