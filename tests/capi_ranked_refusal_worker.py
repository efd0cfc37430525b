"""Started by tests/test_gpu_rank.py in a process of its own, with MC33_HIP_DEVICES=0,0 in the environment before the library is
loaded: the extractor has two z-slabs on one device, which MC33_create_ranked refuses (it filters whole grids on one device).  The
object must still extract afterwards.  Prints, after the object and the grid are freed:
    ranked refused: <1 if NULL> <memoryfault>"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import fixtures as fx  # noqa: E402
from mc33_c_library_amd.api import RANK_MEDIAN, Ranking  # noqa: E402
from mesh_harness import capi  # noqa: E402

assert os.environ.get("MC33_HIP_DEVICES") == "0,0"
lib = capi()
L = lib.lib
L.MC33_create_ranked.restype, L.MC33_create_ranked.argtypes = C.POINTER(lib.MC33), [C.POINTER(lib.MC33), C.POINTER(Ranking)]
iso = lib.real(0.0)
data, r0, d = fx.cos_field(32)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
R = L.MC33_create_ranked(M, C.byref(Ranking((C.c_uint * 3)(1, 1, 1), RANK_MEDIAN)))
fault = M.contents.memoryfault
S = L.calculate_isosurface(M, iso)
assert S and S.contents.nV > 0
L.free_surface_memory(S)
if R:
    L.free_MC33(R)
L.free_MC33(M)
L.free_memory_grd(G)
print("ranked refused: %d %d" % (0 if R else 1, fault))
