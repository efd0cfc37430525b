"""Started by tests/test_gpu_measure.py in a process of its own, with MC33_HIP_DEVICES=0,0 in the environment before the library is
loaded: the extractor has two z-slabs on one device, which the measuring functions of the C API refuse (a slab's triangles name
vertices that live in its neighbour's arrays).  Prints `refused: <rc> <count> <rc>`; the object must still extract."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import fixtures as fx  # noqa: E402
from test_gpu_measure import CComponent, CMeasure, capi  # noqa: E402

assert os.environ.get("MC33_HIP_DEVICES") == "0,0"
lib = capi()
L = lib.lib
data, r0, d = fx.cos_field(32)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
m, many, rows, n = CMeasure(), (CMeasure * 2)(), (CComponent * 4)(), C.c_uint()
a = L.MC33_measure_isosurface(M, lib.real(0.0), C.byref(m))
b = L.MC33_measure_isosurfaces(M, (lib.real * 2)(0.0, 0.5), 2, many)
c = L.MC33_measure_components(M, lib.real(0.0), rows, 4, C.byref(n), None)
S = L.calculate_isosurface(M, lib.real(0.0))
assert S and S.contents.nV > 0
L.free_surface_memory(S)
L.free_MC33(M)
L.free_memory_grd(G)
print("refused: %d %d %d" % (a, b, c))
