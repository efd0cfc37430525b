"""GPU tests of the component compaction (include/mc33_hip.h: mc33hip_compact_components; include/marching_cubes_33.h:
MC33_calculate_filtered_isosurface; DeviceGrid.compact_components / select_components / extract_filtered).

V, N, T come from the reference twin (oracle/_ref) or are synthetic; the expected arrays come from tests/filter_oracle.py, the
definition in numpy.  Everything is compared bit for bit - oV, oN, oT, both attributes, oMap and the three counts; nothing here has
a tolerance.  Every output of every call is canaried (tests/mesh_harness.py: CanariedCall)."""
import ctypes as C
import re

import numpy as np
import pytest

from capi_slab_refusals import refusal
import filter_oracle as fo
import fixtures as fx
import measure_oracle as mo
import property_oracle as po
from filter_cases import ROWS, SIZED, mesh
from mc33_c_library_amd.api import ComponentFilter
from mc33_capi import MC33Lib, ref_path
from mesh_harness import CompactCall as Call, bits, capi, check_python, c_palette, ctx, device_grid, palette, to_device  # noqa: F401 (ctx: the module's fixture)

pytestmark = pytest.mark.gpu

# the rows of the issue's table that a filter struct expresses (the others name their roots)
CRITERIA = {"noise-min16": {"min_triangles": 16}, "noise-closed": {"closed_only": True}, "quant-min8": {"min_triangles": 8}, "quant-all": {},
            "quant-closed": {"closed_only": True}}


# ---- the eight rows of the table that give sizes, float, two attributes ----------------------------------------------------------

@pytest.mark.parametrize("row", SIZED)
def test_table_rows_f32(reflibs, row):
    name, choose, invert, kept, nV_out, nT_out = ROWS[row]
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, name)
    roots = np.asarray(choose(tab, topo), np.uint32)
    P = fx.noise_f32(0, 77, shape=data.shape) * np.float32(1000.0)
    words = np.random.default_rng(11).integers(0, 1 << 32, s.nV, dtype=np.uint64).astype(np.uint32)
    Pv = po.sample_property(s.V, r0, d, P)
    want = fo.compact(s.V, s.N, s.T, lab, roots, invert, attrs=(words, Pv))
    assert (want.components_kept, want.nV_out, want.nT_out) == (kept, nV_out, nT_out)
    g = device_grid(data, r0, d, P)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    labels = g.label_components(T, s.nV)[0]
    assert np.array_equal(labels.cpu().numpy().view(np.uint32), lab)
    dP = g.sample_property(V)
    assert np.array_equal(bits(dP.cpu().numpy()), bits(Pv))
    first = Call(g, V, N, T, labels, roots, invert, attrs=(to_device(words), dP))
    assert first.rc == 0, first.message
    first.check(want)
    again = Call(g, V, N, T, labels, roots[::-1], invert, attrs=(to_device(words), dP))  # (the roots in another order)
    assert again.rc == 0 and again.all_bytes() == first.all_bytes(), "two calls on the same inputs differ"
    check_python(g.compact_components(V, N, T, labels, roots, invert, attrs=(to_device(words), dP)), want)
    # the product's own extraction: its V, N, T are the reference's bit for bit
    if row in CRITERIA:
        crit = CRITERIA[row]
        table = g.measure_components(V, T, labels)
        ttab = g.component_topology(T, s.nV, labels) if crit.get("closed_only") else None
        assert np.array_equal(g.select_components(table, ttab, **crit), roots)
        V2, N2, T2, k2, d2, P2 = g.extract_filtered(iso, with_property=True, **crit)
        assert (k2, d2) == (kept, tab.shape[0] - kept)
        V3, N3, T3, k3, d3 = g.extract_filtered(iso, **crit)
        assert (k3, d3) == (k2, d2) and np.array_equal(bits(V3.cpu().numpy()), bits(want.V)) and np.array_equal(T3.cpu().numpy().view(np.uint32), want.T)
    else:
        oV, oN, oT, cnt, oP = g.extract(iso, with_property=True)
        V2, N2, T2, (P2,), _, k2 = g.compact_components(oV, oN, oT, g.label_components(oT, oV.shape[0])[0], roots, invert, attrs=(oP,))
        assert k2 == kept
    assert np.array_equal(bits(V2.cpu().numpy()), bits(want.V)) and np.array_equal(bits(N2.cpu().numpy()), bits(want.N))
    assert np.array_equal(T2.cpu().numpy().view(np.uint32), want.T) and np.array_equal(bits(P2.cpu().numpy()), bits(want.attrs[1]))


# ---- scan boundaries: synthetic meshes, no grid --------------------------------------------------------------------------------

def synthetic(nV, seed):
    """vertices 3k, 3k+1, 3k+2 form triangle k; a seeded third of the triangles is joined into pairs through a shared vertex (the
    second of a pair names the first one's last vertex instead of its own first, which nothing names any more); the labels follow"""
    rng = np.random.default_rng(seed)
    nT = nV // 3
    T = np.arange(3 * nT, dtype=np.int64).reshape(nT, 3)
    lab = np.arange(nV, dtype=np.int64)
    lab[:3 * nT] = np.repeat(np.arange(nT, dtype=np.int64) * 3, 3)
    joined = rng.permutation(nT)[:(nT // 3) // 2 * 2].reshape(-1, 2)
    a, b = joined.min(axis=1), joined.max(axis=1)
    T[b, 0] = T[a, 2]
    lab[3 * b] = 3 * b          # unreferenced now: its own root
    lab[3 * b + 1] = lab[3 * b + 2] = 3 * a
    V = rng.integers(0, 1 << 32, (nV, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    N = rng.integers(0, 1 << 32, (nV, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    A = [rng.integers(0, 1 << 32, nV, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    comp_roots = np.unique(lab[T[:, 0]]) if nT else np.zeros(0, np.int64)
    roots = comp_roots[rng.random(comp_roots.size) < 0.5]
    return V, N, T.astype(np.uint32), lab.astype(np.uint32), A, roots.astype(np.uint32)


# around a wave, a block, a tile of 4 per lane, and one and four rounds of a 256-tile top-level scan
SIZES = [0, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 262143, 262144, 262145, 1048577]


@pytest.mark.parametrize("nV", SIZES)
def test_scan_boundaries(ctx, nV):
    V, N, T, lab, A, roots = synthetic(nV, 1000 + nV)
    dV, dN, dT, dA = to_device(V), to_device(N), to_device(T.reshape(-1, 3)), [to_device(x) for x in A]
    labels, nc, nu = ctx.label_components(dT, nV)
    assert np.array_equal(labels.cpu().numpy().view(np.uint32), lab)
    for inv in (False, True):
        want = fo.compact(V, N, T, lab, roots, inv, attrs=A)
        assert want.left_out == 0
        call = Call(ctx, dV, dN, dT, labels, roots, inv, attrs=dA)
        assert call.rc == 0, call.message
        call.check(want)


def test_keep_nothing_and_keep_all(reflibs):
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, "quant")
    g = device_grid(data, r0, d)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    labels = g.label_components(T, s.nV)[0]
    none = Call(g, V, N, T, labels, [])
    assert none.rc == 0 and none.counts == (0, 0, 0)
    none.check(fo.compact(s.V, s.N, s.T, lab, []))
    assert np.all(none.host(none.oMap[:s.nV]).view(np.uint32) == fo.NONE)
    every = Call(g, V, N, T, labels, [], invert=True)
    assert every.rc == 0 and every.counts == (15775, 33948, 14)  # only the 25 unreferenced vertices go
    every.check(fo.compact(s.V, s.N, s.T, lab, [], invert=True))
    # a root that owns no triangle (an unreferenced vertex) selects nothing and is no error; duplicates are allowed
    lone = int(np.nonzero(~fo.compact(s.V, s.N, s.T, lab, [], invert=True).keep)[0][0])
    r = [int(tab["root"][1]), lone, int(tab["root"][1])]
    dup = Call(g, V, N, T, labels, r)
    assert dup.rc == 0 and dup.counts[2] == 1
    dup.check(fo.compact(s.V, s.N, s.T, lab, r))
    # nT == 0: 0, 0 and success
    import torch
    empty = Call(g, V, N, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), labels, [], invert=True)
    assert empty.rc == 0 and empty.counts == (0, 0, 0)
    empty.spare_intact()


# ---- the other builds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["u8", "f64", "f64-blobs"])
def test_other_sample_types(reflibs, case):
    """The cos_field_int / cos_field cases of tests/test_gpu_measure.py's test of the same name - one component each, so every
    second row from row 0 keeps everything (24-byte rows of V in the double build) and from row 1 nothing - and, because one
    component says little about the scan, 27 blobs in double as well."""
    dtype, n = case.split("-")[0], 40
    r0, d = mo.AWKWARD_R0, mo.AWKWARD_D
    if case == "f64":
        data, iso = fx.cos_field(n, dtype=np.float64)[0], 0.0
    elif case == "u8":
        data, iso = fx.cos_field_int(n, np.uint8, 40.0, 128.0), 128.5
    else:
        (data, r0, d), iso = fx.cos_field(48, -10.0, 10.0, dtype=np.float64), 2.0
    s = reflibs[dtype].isosurface(data, iso, r0, d)
    assert s.V.dtype == (np.float64 if dtype == "f64" else np.float32) and s.V.strides[0] == (24 if dtype == "f64" else 12) and s.nV > 1000
    lab = mo.label_components(s.T, s.nV)[0]
    tab = mo.component_table(s.V, s.T, lab, mo.reference_point(r0, d, data.shape))[0]
    assert tab.shape[0] == (27 if case == "f64-blobs" else 1)
    words = np.random.default_rng(5).integers(0, 1 << 32, s.nV, dtype=np.uint64).astype(np.uint32)
    g = device_grid(data, r0, d)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    labels = g.label_components(T, s.nV)[0]
    for start in (0, 1):
        roots = tab["root"][start::2]
        want = fo.compact(s.V, s.N, s.T, lab, roots, attrs=(words,))
        assert want.components_kept == roots.size
        call = Call(g, V, N, T, labels, roots, attrs=(to_device(words),))
        assert call.rc == 0, call.message
        call.check(want)
        check_python(g.compact_components(V, N, T, labels, roots, attrs=(to_device(words),)), want)
    table = g.measure_components(V, T, labels)
    V2, N2, T2, k2, d2 = g.extract_filtered(iso, largest=2)
    big = fo.compact(s.V, s.N, s.T, lab, fo.select(tab, largest=2))
    assert (k2, d2) == (big.components_kept, table.shape[0] - big.components_kept)
    assert np.array_equal(bits(V2.cpu().numpy()), bits(big.V)) and np.array_equal(T2.cpu().numpy().view(np.uint32), big.T)


# ---- capacities -------------------------------------------------------------------------------------------------------------------

def test_capacity(reflibs):
    from mc33_c_library_amd.api import Compaction, ECAPACITY
    name, choose, invert, kept, nV_out, nT_out = ROWS["blobs-every-second"]
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, name)
    roots = np.ascontiguousarray(choose(tab, topo), dtype=np.uint32)  # (a column of the table is strided; the call reads n_roots words)
    g = device_grid(data, r0, d)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    labels = g.label_components(T, s.nV)[0]
    # the size query: null outputs, capacity 0
    a = Compaction()
    a.V, a.N, a.T, a.label, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), labels.data_ptr(), s.nV, s.nT
    a.roots, a.n_roots = roots.ctypes.data, roots.size
    assert g.lib.mc33hip_compact_components(g.ctx, C.byref(a)) == ECAPACITY
    assert (a.nV_out, a.nT_out, a.components_kept) == (nV_out, nT_out, kept)
    for capV, capT in ((nV_out - 1, nT_out), (nV_out, nT_out - 1)):
        short = Call(g, V, N, T, labels, roots, attrs=(labels,), capV=capV, capT=capT)
        assert short.rc == ECAPACITY and short.counts == (nV_out, nT_out, kept), (short.rc, short.message)
        short.spare_intact(written=False)  # every output still at its fill
    exact = Call(g, V, N, T, labels, roots, attrs=(labels,), capV=nV_out, capT=nT_out)
    assert exact.rc == 0
    exact.check(fo.compact(s.V, s.N, s.T, lab, roots, attrs=(lab,)))


# ---- invalid input ---------------------------------------------------------------------------------------------------------------

def test_a_triangle_outside_v_is_counted_not_read(reflibs):
    """One index set to nV: tested before anything is gathered through it.  V is the first nV rows of a tensor with 16 spare
    rows behind them, so that not even a wrong kernel could touch memory this test does not own."""
    import torch
    from mc33_c_library_amd.api import ERUNTIME
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, "blobs")
    g = device_grid(data, r0, d)
    room = torch.zeros((s.nV + 16, 3), dtype=torch.float32, device="cuda")
    room[:s.nV] = to_device(s.V)
    V, N = room[:s.nV], to_device(s.N)
    badT = s.T.copy()
    badT[777, 1] = s.nV
    T, Tbad = to_device(s.T), to_device(badT)
    labels = g.label_components(T, s.nV)[0]
    roots = tab["root"][::2]
    want = fo.compact(s.V, s.N, badT, lab, roots)
    assert want.left_out == 1 and want.nT_out == fo.compact(s.V, s.N, s.T, lab, roots).nT_out - 1
    bad = Call(g, V, N, Tbad, labels, roots)
    assert bad.rc == ERUNTIME and "1 triangle " in bad.message, (bad.rc, bad.message)
    bad.check(want)  # the outputs are the oracle's without that triangle
    good = Call(g, V, N, T, labels, roots)  # the next call on the context succeeds
    assert good.rc == 0, good.message
    good.check(fo.compact(s.V, s.N, s.T, lab, roots))


def test_labels_of_another_mesh(reflibs):
    """The labels of the first half of the triangles, a few of them outside the array: kept triangles name vertices that are not
    kept.  ERUNTIME with the count, the outputs as the definition has them, nothing outside them written."""
    from mc33_c_library_amd.api import ERUNTIME
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, "noise")
    other = mo.label_components(s.T[:s.nT // 2], s.nV)[0].copy()
    other[5::997] = 0xFFFFFFFF
    other[6::997] = s.nV
    cand = np.unique(other[other < s.nV])
    roots = cand[::2]
    want = fo.compact(s.V, s.N, s.T, other, roots)
    assert want.left_out > 0 and want.nT_out > 0
    g = device_grid(data, r0, d)
    call = Call(g, to_device(s.V), to_device(s.N), to_device(s.T), to_device(other), roots)
    assert call.rc == ERUNTIME and re.search(r"\b%d triangles " % want.left_out, call.message), (call.rc, call.message, want.left_out)
    call.check(want)


def test_invalid_arguments(reflibs):
    from mc33_c_library_amd.api import Compaction, EINVAL
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, "blobs")
    g = device_grid(data, r0, d)
    V, N, T = to_device(s.V), to_device(s.N), to_device(s.T)
    labels = g.label_components(T, s.nV)[0]
    roots = np.ascontiguousarray(tab["root"][::2], dtype=np.uint32)
    import torch
    oV, oN, oT = torch.empty_like(V), torch.empty_like(N), torch.empty_like(T)
    oA = [torch.empty_like(labels) for _ in range(2)]
    spare = torch.empty_like(labels)

    def call(**change):
        a = Compaction()
        a.V, a.N, a.T, a.label, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), labels.data_ptr(), s.nV, s.nT
        a.roots, a.n_roots = roots.ctypes.data, roots.size
        a.oV, a.oN, a.oT, a.capV, a.capT = oV.data_ptr(), oN.data_ptr(), oT.data_ptr(), s.nV, s.nT
        for k, v in change.items():
            if k in ("attr", "oAttr"):
                for j, x in enumerate(v):
                    getattr(a, k)[j] = x
            else:
                setattr(a, k, v)
        return g.lib.mc33hip_compact_components(g.ctx, C.byref(a))
    assert call() == 0
    # null pointers where sizes are not zero
    for name in ("V", "N", "T", "label", "roots", "oV", "oN", "oT"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n_attr=1, oAttr=[oA[0].data_ptr()]) == EINVAL and call(n_attr=1, attr=[labels.data_ptr()]) == EINVAL
    assert g.lib.mc33hip_compact_components(g.ctx, None) == EINVAL and g.lib.mc33hip_compact_components(None, C.byref(Compaction())) == EINVAL
    # sizes above 2^32-1, three attributes, a root >= nV
    assert call(nV=1 << 32) == EINVAL and call(nT=1 << 32) == EINVAL
    assert call(n_attr=3, attr=[labels.data_ptr(), labels.data_ptr()], oAttr=[oA[0].data_ptr(), oA[1].data_ptr()]) == EINVAL
    big = np.array([roots[0], s.nV], np.uint32)
    assert call(roots=big.ctypes.data, n_roots=2) == EINVAL
    # an output that meets an input: oV == V, oT inside T, oMap over the labels, an attribute onto itself
    assert call(oV=V.data_ptr()) == EINVAL
    assert call(oT=T.data_ptr() + 12 * 100, capT=s.nT - 100) == EINVAL
    assert call(oMap=labels.data_ptr()) == EINVAL
    assert call(n_attr=1, attr=[spare.data_ptr()], oAttr=[spare.data_ptr() + 4 * (s.nV - 1)]) == EINVAL
    assert call(n_attr=2, attr=[labels.data_ptr(), spare.data_ptr()], oAttr=[oA[0].data_ptr(), oA[1].data_ptr()]) == 0


# ---- the C API -------------------------------------------------------------------------------------------------------------------

def filtered(lib, M, iso, f):
    k, dr = C.c_uint(77), C.c_uint(77)
    S = lib.lib.MC33_calculate_filtered_isosurface(M, lib.real(iso), C.byref(f) if f is not None else None, C.byref(k), C.byref(dr))
    if not S:
        return None, k.value, dr.value
    try:
        if S.contents.nV:  # the object's public prefix mirrors the returned surface, as calculate_isosurface leaves it
            m, r = M.contents, S.contents
            assert (m.T, m.V, m.N, m.color, m.nT, m.capt, m.capv) == (r.T, r.V, r.N, r.color, r.nT, r.capt, r.capv)
        return lib.copy_surface(S), k.value, dr.value
    finally:
        lib.lib.free_surface_memory(S)


def check_surface(got, want):
    assert (got.nV, got.nT) == (want.nV_out, want.nT_out)
    assert np.array_equal(bits(got.V), bits(want.V)) and np.array_equal(bits(got.N), bits(want.N)) and np.array_equal(got.T, want.T)


@pytest.mark.parametrize("row", ["noise-min16", "quant-closed"])
def test_c_api(reflibs, row):
    name, choose, invert, kept, nV_out, nT_out = ROWS[row]
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, name)
    want = fo.compact(s.V, s.N, s.T, lab, choose(tab, topo))
    lib = capi()
    L = lib.lib
    G, keep = lib.make_grid(data, r0, d)
    P = fx.noise_f32(0, 79, shape=data.shape) * np.float32(10.0)
    Pg, keep2 = lib.make_grid(P, r0, d)
    M = L.create_MC33(G)
    assert M
    try:
        f = ComponentFilter(**{k: int(v) for k, v in CRITERIA[row].items()})
        got, k, dr = filtered(lib, M, iso, f)
        assert got is not None and (k, dr) == (kept, tab.shape[0] - kept)
        check_surface(got, want)
        assert np.all(got.color == po.DEFAULT_COLOR) and got.color.size == want.nV_out
        assert M.contents.iso == np.float32(iso) and M.contents.memoryfault == 0 and M.contents.nT == want.nT_out
        nV_left = M.contents.nV
        again, _, _ = filtered(lib, M, iso, f)
        check_surface(again, want)
        # colours: those of the unfiltered surface at the kept vertices
        pal, lo, hi = palette(7), -2.5, 3.25
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, c_palette(pal), len(pal), lo, hi) == 0
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        whole = lib.copy_surface(S)
        assert M.contents.nV == nV_left and (M.contents.V, M.contents.nT, M.contents.capv) == (S.contents.V, s.nT, S.contents.capv)  # (nV: the same after either call)
        L.free_surface_memory(S)
        assert np.array_equal(whole.color, po.color_vertices(s.V, r0, d, P, pal, lo, hi)) and np.unique(whole.color).size > 2
        painted, k, dr = filtered(lib, M, iso, f)
        check_surface(painted, want)
        assert np.array_equal(painted.color, whole.color[want.keep])
        assert L.MC33_set_property_grid(M, None) == 0
        plain, _, _ = filtered(lib, M, iso, f)
        assert np.all(plain.color == po.DEFAULT_COLOR)
        # a null filter is refused; the object is still good, and its surface is the reference's
        none, k, dr = filtered(lib, M, iso, None)
        assert none is None and (k, dr) == (0, 0)
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        mine = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert np.array_equal(bits(mine.V), bits(s.V)) and np.array_equal(mine.T, s.T) and np.array_equal(bits(mine.N), bits(s.N))
        # keep nothing: an empty surface, not a failure
        nothing, k, dr = filtered(lib, M, iso, ComponentFilter(min_triangles=1 << 30))
        assert nothing is not None and (nothing.nV, nothing.nT, k, dr) == (0, 0, 0, tab.shape[0])
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2


def test_c_api_nneg_flavour():
    """the nneg reference's own surface, filtered by the oracle"""
    field, iso, _ = mo.FIXTURES["noise"]
    data, r0, d = field()
    s = MC33Lib(ref_path("f32", nneg=True), "f32").isosurface(data, iso, r0, d)
    lab = mo.label_components(s.T, s.nV)[0]
    tab = mo.component_table(s.V, s.T, lab, mo.reference_point(r0, d, data.shape))[0]
    want = fo.compact(s.V, s.N, s.T, lab, fo.select(tab, min_triangles=16))
    assert (want.components_kept, want.nV_out, want.nT_out) == (8, 47990, 101970)
    lib = capi(nneg=True)
    L = lib.lib
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    assert M
    try:
        got, k, dr = filtered(lib, M, iso, ComponentFilter(min_triangles=16))
        assert (k, dr) == (8, tab.shape[0] - 8)
        check_surface(got, want)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refuses_an_object_on_several_slabs(launcher):
    """MC33_HIP_DEVICES=0,0 in a fresh process, before the library is loaded: two slabs on one device (tests/capi_slab_refusals_worker.py)."""
    out = refusal(launcher, "filter")
    assert out["rc"] == 0 and "refused: 1 0 0" in out["stdout"], out
