"""Started by tests/test_gpu_clip.py in a process of its own, with MC33_HIP_DEVICES=0,0 in the environment before the library is
loaded: the extractor has two z-slabs on one device, which MC33_calculate_clipped_isosurface refuses (a slab's triangles name
vertices that live in its neighbour's arrays).  Prints `refused: <1 if NULL> <memoryfault>`; the object must still extract."""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import fixtures as fx  # noqa: E402
from test_gpu_clip import capi, cclip  # noqa: E402

assert os.environ.get("MC33_HIP_DEVICES") == "0,0"
lib = capi()
L = lib.lib
data, r0, d = fx.cos_field(32)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
cl = cclip([(0.0, 0.0, 1.0, 0.0)])
F = L.MC33_calculate_clipped_isosurface(M, lib.real(0.0), C.byref(cl))
fault = M.contents.memoryfault
S = L.calculate_isosurface(M, lib.real(0.0))
assert S and S.contents.nV > 0
L.free_surface_memory(S)
L.free_MC33(M)
L.free_memory_grd(G)
print("refused: %d %d" % (0 if F else 1, fault))
