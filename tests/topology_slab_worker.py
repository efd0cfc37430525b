"""Started by tests/test_gpu_topology.py in a process of its own, with MC33_HIP_DEVICES=0,0 in the environment before the library
is loaded: the extractor has two z-slabs on one device, which the topology functions of the C API refuse (a slab's triangles
name vertices that live in its neighbour's arrays).  Prints `refused: <rc> <rc> <components>`; the object must still extract."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import fixtures as fx  # noqa: E402
from mc33_capi import MC33Lib, product_path  # noqa: E402
from test_topology_cpu import CComponentTopology, CTopology, bind_topology_api  # noqa: E402

assert os.environ.get("MC33_HIP_DEVICES") == "0,0"
lib = MC33Lib(product_path("f32"), "f32")
bind_topology_api(lib)
L = lib.lib
data, r0, d = fx.cos_field(32)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
t, rows, n = CTopology(), (CComponentTopology * 4)(), C.c_uint(7)
a = L.MC33_isosurface_topology(M, lib.real(0.0), C.byref(t))
b = L.MC33_component_topology(M, lib.real(0.0), rows, 4, C.byref(n))
S = L.calculate_isosurface(M, lib.real(0.0))
assert S and S.contents.nV > 0
L.free_surface_memory(S)
L.free_MC33(M)
L.free_memory_grd(G)
print("refused: %d %d %d" % (a, b, n.value))
