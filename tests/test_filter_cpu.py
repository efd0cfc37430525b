"""Keeping or dropping surface components, the part that needs no GPU: the numpy oracle of the compaction on the
unmodified reference's meshes against figures computed once from them, its invariants, MC33_select_components - host C in the
product library - against the restated rule, the new names in the headers, the libraries and the code objects, and the
host-logic build of mc33_capi.c, whose emulated device layer cannot compact.

test_oracle_on_the_reference_meshes tests the oracle and the fixtures, not the product: it pins tests/filter_oracle.py to the
figures of the table and passes without the feature.  The product is held to that oracle by the select, header, export,
code-object and host-logic tests below and, on the device, by tests/test_gpu_filter.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import filter_oracle as fo
import measure_oracle as mo
import topology_oracle as to
from mc33_capi import product_path
from filter_cases import ROWS, mesh
from mc33_c_library_amd.api import Component, ComponentFilter, ComponentTopology
from mesh_checks import assert_exported, assert_kernels, host_logic, launched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_compact_components"]
C_NAMES = ["MC33_select_components", "MC33_calculate_filtered_isosurface"]
KERNELS = ["k_filt_roots", "k_filt_keep", "k_filt_tri_count", "k_filt_tris"] + launched("k_mesh_ref", "k_mesh_scan_top", "k_mesh_place<MeshFlag, 1>")


@pytest.mark.parametrize("row", list(ROWS))
def test_oracle_on_the_reference_meshes(reflibs, row):
    name, choose, invert, kept, nV_out, nT_out = ROWS[row]
    data, r0, d, iso, s, lab, tab, topo, c = mesh(reflibs, name)
    roots = np.asarray(choose(tab, topo), np.uint32)
    got = fo.compact(s.V, s.N, s.T, lab, roots, invert)
    print("%s: kept %d components, %d vertices, %d triangles" % (row, got.components_kept, got.nV_out, got.nT_out))
    assert got.components_kept == kept and got.left_out == 0
    assert nV_out is None or got.nV_out == nV_out
    assert nT_out is None or got.nT_out == nT_out
    if row == "blobs-every-second":
        assert roots[:4].tolist() == [6, 150, 162, 306]
    if row == "blobs-the-1868-row":
        assert roots.tolist() == [8908]
    if row == "noise-not-the-big-one":
        assert roots.tolist() == [0] and int(np.nonzero(got.keep)[0][0]) == 22
    if row == "noise-min-area":
        a = np.sort(tab["area"])[::-1]
        assert round(float(a[0]), 2) == 327.32 and round(float(a[1]), 4) == 0.0701 and round(float(a[2]), 4) == 0.0492
    if row == "quant-min-volume":
        w = np.sort(np.abs(tab["volume"]))[::-1]
        assert round(float(w[0]), 1) == 461.5 and round(float(w[1]), 2) == 9.69 and round(float(w[2]), 2) == 1.55
    if row == "blobs-largest3":
        assert roots.tolist() == tab["root"][tab["nT"] == 1940][:3].tolist()
    # the invariants
    lab2, nc2, unref2, _ = mo.label_components(got.T, got.nV_out)
    assert unref2 == 0 and nc2 == kept
    selected = np.isin(tab["root"], roots) != invert
    want = tab[selected]
    tab2 = mo.component_table(got.V, got.T, lab2, c)[0]
    assert np.array_equal(tab2["nV"], want["nV"]) and np.array_equal(tab2["nT"], want["nT"])
    assert np.array_equal(tab2["root"], got.vmap[want["root"]])
    assert np.array_equal(tab2["area"].view(np.uint64), want["area"].view(np.uint64))  # (the order of a component's triangles is unchanged)
    topo2 = to.component_table(got.T, got.nV_out, lab2)
    for col in ("nV", "nT") + to.COUNTS + ("euler", "genus"):
        assert np.array_equal(topo2[col], topo[selected][col]), col
    again = fo.compact(got.V, got.N, got.T, lab2, tab2["root"])
    assert np.array_equal(again.T, got.T) and np.array_equal(again.V.view(np.uint32), got.V.view(np.uint32))
    assert np.array_equal(again.N.view(np.uint32), got.N.view(np.uint32)) and np.array_equal(again.vmap, np.arange(got.nV_out, dtype=np.uint32))


# ---- the selection rule: host C in the product library, no GPU -------------------------------------------------------------------

@pytest.fixture(scope="module")
def select_lib():
    path = product_path("f32")
    assert os.path.exists(path), "build the HIP libraries first (python -m mc33_c_library_amd.build)"
    from mc33_c_library_amd import load_library
    return load_library("f32")


def c_select(lib, tab, topo=None, **criteria):
    t = np.ascontiguousarray(tab, dtype=np.dtype(Component))
    p = np.ascontiguousarray(topo, dtype=np.dtype(ComponentTopology)) if topo is not None else None
    roots = np.full(t.shape[0] + 1, 0xDEADBEEF, np.uint32)
    f = ComponentFilter(**{k: (int(v) if k == "closed_only" else v) for k, v in criteria.items()})
    n = lib.MC33_select_components(t.ctypes.data if t.shape[0] else None, p.ctypes.data if p is not None else None, t.shape[0], C.byref(f), roots.ctypes.data)
    assert roots[-1] == 0xDEADBEEF
    return None if n < 0 else roots[:n].copy()


CRITERIA = [{}, {"min_triangles": 16}, {"min_triangles": 8}, {"min_triangles": 1869}, {"min_area": 0.06}, {"min_abs_volume": 5.0}, {"closed_only": True},
            {"largest": 3}, {"largest": 1}, {"largest": 1000}, {"min_triangles": 5, "closed_only": True, "largest": 4}, {"min_area": 1e9}]


@pytest.mark.parametrize("name", ["blobs", "noise", "quant"])
def test_select_components_on_the_reference_tables(reflibs, select_lib, name):
    tab, topo = mesh(reflibs, name)[6:8]
    for crit in CRITERIA:
        got, want = c_select(select_lib, tab, topo, **crit), fo.select(tab, topo, **crit)
        assert np.array_equal(got, want), (name, crit, got, want)
        assert np.all(np.diff(got.astype(np.int64)) > 0)
    assert np.array_equal(c_select(select_lib, tab), tab["root"])  # a zeroed filter keeps every row


def test_select_components_on_synthetic_tables(select_lib):
    tab = np.zeros(9, mo.COMPONENT)
    tab["root"] = [3, 7, 8, 20, 21, 40, 41, 90, 91]
    tab["nT"] = [10, 50, 50, 50, 4, 50, 7, 10, 50]
    tab["area"] = [1.0, 2.0, 0.5, 2.0, 0.1, 3.0, 0.2, 1.0, 0.3]
    tab["volume"] = [-1.0, 2.0, -0.5, -2.0, 0.0, 3.0, 0.2, -1.0, 1.0]
    topo = np.zeros(9, to.COMPONENT)
    topo["root"] = tab["root"]
    topo["boundary_edges"] = [0, 4, 0, 0, 1, 0, 0, 2, 0]
    for crit in CRITERIA + [{"largest": 2}, {"largest": 4}, {"largest": 5}, {"largest": 9}, {"largest": 10}, {"min_triangles": 50, "largest": 3},
                            {"min_abs_volume": 1.0}, {"min_abs_volume": 1.0, "closed_only": True, "largest": 2}, {"min_area": 0.0}]:
        got, want = c_select(select_lib, tab, topo, **crit), fo.select(tab, topo, **crit)
        assert np.array_equal(got, want), (crit, got, want)
    assert c_select(select_lib, tab, topo, largest=2).tolist() == [7, 8]  # ties among the 50s: the smaller roots
    assert c_select(select_lib, tab, topo, largest=20).tolist() == tab["root"].tolist()
    assert c_select(select_lib, tab[:0]).tolist() == []  # n == 0
    # -1: closed_only without topology rows, null arguments
    assert c_select(select_lib, tab, None, closed_only=True) is None and fo.select(tab, None, closed_only=True) is None
    t = np.ascontiguousarray(tab, dtype=np.dtype(Component))
    roots = np.zeros(9, np.uint32)
    f = ComponentFilter()
    assert select_lib.MC33_select_components(t.ctypes.data, None, 9, None, roots.ctypes.data) == -1
    assert select_lib.MC33_select_components(None, None, 9, C.byref(f), roots.ctypes.data) == -1
    assert select_lib.MC33_select_components(t.ctypes.data, None, 9, C.byref(f), None) == -1
    assert select_lib.MC33_select_components(None, None, 0, C.byref(f), None) == 0


# ---- names, kernels, structs ------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_compact_components\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_compaction;", hip)
    assert re.search(r"\bint MC33_select_components\(const mc33_component \*", pub)
    assert re.search(r"\bsurface \*MC33_calculate_filtered_isosurface\(MC33 \*", pub) and re.search(r"\} mc33_component_filter;", pub)
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype,real", [("f32", "float"), ("f64", "double")])
def test_filter_kernels_are_in_the_code_object(dtype, real):
    assert_kernels(dtype, KERNELS + ["k_filt_rows<%s>" % real])


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_filter(dtype):
    """mc33_capi.c linked with the emulated device layer, which cannot compact: the library still loads (a weak reference),
    MC33_calculate_filtered_isosurface returns NULL, the selection rule - plain host C - works, and the object extracts as before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        f, k, dr = ComponentFilter(), C.c_uint(7), C.c_uint(7)
        assert not L.MC33_calculate_filtered_isosurface(M, lib.real(iso), C.byref(f), C.byref(k), C.byref(dr)) and (k.value, dr.value) == (0, 0)
        tab = np.zeros(2, mo.COMPONENT)
        tab["root"], tab["nT"] = [0, 5], [3, 9]
        assert c_select(L, tab, min_triangles=4).tolist() == [5]
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
