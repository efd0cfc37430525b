"""Started once per session (tests/capi_slab_refusals.py) in a process of its own, with MC33_HIP_DEVICES=0,0 in the environment
before the library is loaded: the extractor has two z-slabs on one device, which every C API call that works on an extracted
surface refuses (a slab's triangles name vertices that live in its neighbour's arrays).  One object, every refused call, and
after each part the object must still extract.  Prints, after the object and the grid are freed, one line per part:
    measure refused: <rc> <count> <rc>          MC33_measure_isosurface, MC33_measure_isosurfaces, MC33_measure_components
    topology refused: <rc> <rc> <components>    MC33_isosurface_topology, MC33_component_topology
    filter refused: <1 if NULL> <kept> <dropped>
    smooth / simplify / clip refused: <1 if NULL> <memoryfault>"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import fixtures as fx  # noqa: E402
from clip_cases import cclip  # noqa: E402
from mc33_c_library_amd.api import Component, ComponentFilter, ComponentTopology, SurfaceSmoothing  # noqa: E402
from mc33_capi import CMeasure, CTopology  # noqa: E402
from mesh_harness import capi  # noqa: E402
from simplify_cases import csimp  # noqa: E402

assert os.environ.get("MC33_HIP_DEVICES") == "0,0"
lib = capi()
L = lib.lib
iso = lib.real(0.0)
data, r0, d = fx.cos_field(32)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
lines = []


def still_extracts():
    S = L.calculate_isosurface(M, iso)
    assert S and S.contents.nV > 0
    L.free_surface_memory(S)


m, many, rows, n = CMeasure(), (CMeasure * 2)(), (Component * 4)(), C.c_uint()
a = L.MC33_measure_isosurface(M, iso, C.byref(m))
b = L.MC33_measure_isosurfaces(M, (lib.real * 2)(0.0, 0.5), 2, many)
c = L.MC33_measure_components(M, iso, rows, 4, C.byref(n), None)
still_extracts()
lines.append("measure refused: %d %d %d" % (a, b, c))

t, trows, n = CTopology(), (ComponentTopology * 4)(), C.c_uint(7)
a = L.MC33_isosurface_topology(M, iso, C.byref(t))
b = L.MC33_component_topology(M, iso, trows, 4, C.byref(n))
still_extracts()
lines.append("topology refused: %d %d %d" % (a, b, n.value))

f, k, dr = ComponentFilter(), C.c_uint(5), C.c_uint(5)
F = L.MC33_calculate_filtered_isosurface(M, iso, C.byref(f), C.byref(k), C.byref(dr))
still_extracts()
lines.append("filter refused: %d %d %d" % (0 if F else 1, k.value, dr.value))

sm = SurfaceSmoothing(10, 0.5, -0.53, 1)
F = L.MC33_calculate_smoothed_isosurface(M, iso, C.byref(sm))
fault = M.contents.memoryfault
still_extracts()
lines.append("smooth refused: %d %d" % (0 if F else 1, fault))

sp = csimp((2.0, 2.0, 2.0), 0, 1)
F = L.MC33_calculate_simplified_isosurface(M, iso, C.byref(sp))
fault = M.contents.memoryfault
still_extracts()
lines.append("simplify refused: %d %d" % (0 if F else 1, fault))

cl = cclip([(0.0, 0.0, 1.0, 0.0)])
F = L.MC33_calculate_clipped_isosurface(M, iso, C.byref(cl))
fault = M.contents.memoryfault
still_extracts()
lines.append("clip refused: %d %d" % (0 if F else 1, fault))

L.free_MC33(M)
L.free_memory_grd(G)
print("\n".join(lines))
