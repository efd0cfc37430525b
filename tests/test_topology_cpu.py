"""Surface topology (edges, boundary, Euler number, genus), the part that needs no GPU: the numpy oracle of the definition on the
unmodified reference's five fixture meshes against the figures computed from them once and written down here, the new names in
the headers and in every built library, the new kernels in the code object, and the host-logic build of mc33_capi.c, whose
emulated device layer has no edge table."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import measure_oracle as mo
import topology_oracle as to
from mc33_c_library_amd.api import ComponentTopology
from mc33_capi import CTopology
from mesh_checks import assert_exported, assert_kernels, host_logic, launched, reference_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_surface_topology", "mc33hip_component_topology"]
C_NAMES = ["MC33_isosurface_topology", "MC33_component_topology"]
KERNELS = ["k_topo_insert", "k_topo_classify", "k_topo_rows_triangles", "k_topo_rows_vertices", "k_topo_finish"] + launched("k_mesh_clear", "k_mesh_scan_top", "k_mesh_place<MeshFlag, 0>")

# fixture -> unique edges, used once, used more than twice, most uses of one edge, used twice in the same direction, degenerate
# triangles, Euler number nV_ref - E + nT, boundary loops, boundary vertices that do not end exactly two boundary edges
FIGURES = {
    "sphere": (63084, 0, 0, 2, 0, 0, 2, 0, 0),
    "blobs": (78246, 0, 0, 2, 0, 0, 54, 0, 0),
    "sheet": (44508, 720, 0, 2, 0, 0, -4, 6, 0),
    "noise": (157201, 5778, 14, 4, 0, 0, -5508, 314, 0),
    "quant": (51777, 2603, 430, 8, 0, 0, -2054, 91, 72),
}
# fixture -> {(closed, Euler number of the component): how many}
CHI = {
    "sphere": {(True, 2): 1},
    "blobs": {(True, 2): 27},
    "sheet": {(False, -4): 1},
    "noise": {(True, 2): 86, (False, 1): 65, (False, -5745): 1},
    "quant": {(True, 2): 7, (False, 1): 6, (False, -2074): 1},
}

_cache = {}


def figures(reflibs, name):
    """(surface dict, component table, edge table) of the oracle on the reference's mesh of a fixture, made once"""
    if name not in _cache:
        s = reference_mesh(reflibs, name)[4]
        lab = mo.label_components(s.T, s.nV)[0]
        e = to.EdgeTable(s.T, s.nV)
        surf, tab = to.surface(s.T, s.nV, lab, e)
        _cache[name] = (surf, tab, e, s.T)
    return _cache[name]


@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_oracle_reproduces_the_table(reflibs, name):
    surf, tab, e, T = figures(reflibs, name)
    ends = np.bincount(np.concatenate([e.lo[e.boundary], e.hi[e.boundary]]))
    got = (surf["edges"], surf["boundary_edges"], surf["nonmanifold_edges"], int(e.uses.max()), surf["misoriented_edges"], surf["degenerate_triangles"],
           surf["euler"], surf["boundary_loops"], int(np.count_nonzero((ends != 0) & (ends != 2))))
    print(name, got)
    assert got == FIGURES[name]
    assert surf["boundary_edges"] == mo.open_edges(T) == mo.FIXTURES[name][2][4]
    nV, nT, ncomp, unref, _ = mo.FIXTURES[name][2]
    assert (surf["nV"], surf["nT"], surf["components"], surf["referenced_vertices"]) == (nV, nT, ncomp, nV - unref)
    assert (surf["closed"], surf["manifold"], surf["oriented"]) == (int(FIGURES[name][1] == 0), int(FIGURES[name][2] == 0), 1)


@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_oracle_per_component(reflibs, name):
    surf, tab, e, T = figures(reflibs, name)
    hist = collections.Counter((bool(r["boundary_edges"] == 0), int(r["euler"])) for r in tab)
    assert dict(hist) == CHI[name]
    # the columns add up to the surface's figures
    for col in to.COUNTS:
        assert int(tab[col].sum()) == surf[col], col
    assert int(tab["nV"].sum()) == surf["referenced_vertices"] and int(tab["nT"].sum()) == surf["nT"]
    assert int(tab["euler"].sum()) == surf["euler"]
    assert surf["closed_components"] == sum(n for (closed, _), n in CHI[name].items() if closed)
    assert np.all(np.diff(tab["root"].astype(np.int64)) > 0)
    if name in ("sphere", "blobs", "sheet"):  # genus 0 everywhere: the sheet's (2 + 4 - 6) / 2
        assert np.all(tab["genus"] == 0) and surf["genus_sum"] == 0 and surf["genus_defined"] == 1
    else:  # the large component has non-manifold edges; every other one is a sphere or a disc
        assert sorted(tab["genus"].tolist())[:2] == [-1, 0] and surf["genus_sum"] == 0 and surf["genus_defined"] == 0


def test_oracle_on_small_meshes():
    """a tetrahedron, the same with one triangle turned over, a torus of 3 x 3 quads, a strip with a degenerate triangle"""
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    s, tab = to.surface(tet, 4, np.zeros(4, np.uint32))
    assert (s["edges"], s["euler"], s["closed"], s["oriented"], s["genus_sum"], tab["genus"].tolist()) == (6, 2, 1, 1, 0, [0])
    flipped = tet.copy()
    flipped[1] = flipped[1, [1, 0, 2]]
    s, tab = to.surface(flipped, 4, np.zeros(4, np.uint32))
    assert (s["misoriented_edges"], s["oriented"], s["genus_defined"], tab["genus"].tolist()) == (3, 0, 0, [-1])
    n, tris = 3, []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * n + j, ((i + 1) % n) * n + j, ((i + 1) % n) * n + (j + 1) % n, i * n + (j + 1) % n
            tris += [[a, b, c], [a, c, d]]
    s, tab = to.surface(np.array(tris), 9, np.zeros(9, np.uint32))
    assert (s["edges"], s["euler"], s["closed"], s["manifold"], s["oriented"], s["genus_sum"]) == (27, 0, 1, 1, 1, 1)
    strip = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 3], [7, 1, 2]])  # vertex 5 unreferenced, the last triangle invalid for nV = 6
    s, tab = to.surface(strip, 6, np.array([0, 0, 0, 0, 0, 5], np.uint32))
    assert (s["degenerate_triangles"], s["manifold"], s["referenced_vertices"], s["edges"], s["boundary_edges"], s["boundary_loops"]) == (1, 0, 5, 6, 4, 1)  # ({3, 4} is used twice: 3 -> 4 forward, 4 -> 3 backward, and 3 -> 3 is skipped)
    assert s["euler"] == 5 - 6 + 3 and tab["genus"].tolist() == [-1] and tab["nT"].tolist() == [3]
    s, tab = to.surface(np.zeros((0, 3), np.uint32), 6, np.arange(6))
    assert tab.shape[0] == 0 and [s[k] for k in ("closed", "manifold", "oriented", "genus_defined", "euler", "edges")] == [1, 1, 1, 1, 0, 0]


def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    for n in HIP_NAMES:
        assert re.search(r"\bint %s\(mc33hip_ctx \*" % n, hip), n
    for n in C_NAMES:
        assert re.search(r"\bint %s\(MC33 \*" % n, pub), n
    assert re.search(r"\} mc33hip_topology;", hip) and re.search(r"\bstruct mc33hip_component_topology \{", hip)
    for t in ("mc33_topology", "mc33_component_topology"):
        assert re.search(r"\} %s;" % t, pub), t
    assert "pinched vertex" in hip
    from mc33_c_library_amd import HIP_API, REFERENCE_API
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


def test_topology_kernels_are_in_the_code_object():
    assert_kernels("f32", KERNELS, max_vgprs=128)  # (two blocks of 256 per SIMD at least)


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses(dtype):
    """mc33_capi.c linked with the emulated device layer, which has neither entry point: the library still loads (they are weak
    references), both functions return -1, and the object extracts as before."""
    with host_logic(dtype) as h:
        lib, L, M, iso = h.lib, h.L, h.M, h.iso
        t, rows, n = CTopology(), (ComponentTopology * 4)(), C.c_uint(7)
        assert L.MC33_isosurface_topology(M, lib.real(iso), C.byref(t)) == -1
        assert L.MC33_component_topology(M, lib.real(iso), rows, 4, C.byref(n)) == -1 and n.value == 0
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
