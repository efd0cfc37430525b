"""Started by tests/test_gpu_section.py in a process of its own, with MC33_HIP_DEVICES=0,0 in the environment before the library
is loaded: the extractor has two z-slabs on one device, which the section calls refuse as every C API call that works on an
extracted surface does (the pattern of tests/capi_slab_refusals_worker.py).  After them the object must be untouched and still
extract.  Prints, after the object and the grid are freed:
    section refused: <1 if NULL> <rc of MC33_section_contours> <rc of MC33_section_profile> <1 if the object is untouched>"""
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import fixtures as fx  # noqa: E402
from mc33_capi import MC33Lib, product_path  # noqa: E402
from mc33_c_library_amd.api import Contour, SectionLevel  # noqa: E402

assert os.environ.get("MC33_HIP_DEVICES") == "0,0"
lib = MC33Lib(product_path("f32"), "f32")
L = lib.lib
iso = lib.real(0.0)
data, r0, d = fx.cos_field(32)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
S = L.calculate_isosurface(M, iso)
assert S and S.contents.nV > 0
L.free_surface_memory(S)
before = (M.contents.iso, M.contents.nT, M.contents.nV, M.contents.memoryfault, M.contents.T, M.contents.V)
plane = (C.c_double * 4)(0.0, 0.0, 1.0, 0.0)
table, n = (Contour * 4)(), C.c_uint(7)
levels = (SectionLevel * 2)()
F = L.MC33_section_isosurface(M, lib.real(0.5), C.byref(plane))
a = L.MC33_section_contours(M, lib.real(0.5), C.byref(plane), table, 4, C.byref(n))
b = L.MC33_section_profile(M, lib.real(0.5), C.byref((C.c_double * 3)(0.0, 0.0, 1.0)), (C.c_double * 2)(-0.5, 0.5), 2, levels)
same = (M.contents.iso, M.contents.nT, M.contents.nV, M.contents.memoryfault, M.contents.T, M.contents.V) == before and n.value == 0
S = L.calculate_isosurface(M, iso)
assert S and S.contents.nV > 0
L.free_surface_memory(S)
L.free_MC33(M)
L.free_memory_grd(G)
del keep
print("section refused: %d %d %d %d" % (0 if F else 1, a, b, 1 if same else 0))
