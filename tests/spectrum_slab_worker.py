"""Process of tests/test_gpu_spectrum.py: MC33_grid_spectrum of the product libraries with the grid spread over three slabs on ONE
GPU (MC33_HIP_DEVICES=0,0,0 is read when the extractor is created, so it needs a process of its own).  Every slab counts its own
cell slices; the sums and extremes must be the oracle's for the whole grid, and the MC33 struct must stay as it was."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import spectrum_cases as sc  # noqa: E402
import spectrum_oracle as so  # noqa: E402
from mc33_capi import MC33Lib, product_path  # noqa: E402
from spectrum_cases import c_spectrum, report  # noqa: E402


def main():
    assert os.environ.get("MC33_HIP_DEVICES") == "0,0,0"
    done = 0
    for dtype, name in (("f32", "special_values"), ("u8", "one_point_beyond_noise"), ("u16", "tile_minus_1_beyond_cos"), ("f64", "narrow_dword_plus_3_noise")):
        lib = MC33Lib(product_path(dtype), dtype)
        L = lib.lib
        F, isos, want = sc.case(name, dtype)
        G, keep = lib.make_grid(np.array(F))
        M = L.create_MC33(G)
        assert M
        try:
            before = bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33)))
            got = c_spectrum(lib, L, M, isos)
            assert got != -1 and so.same(got, want), "%s %s\n%s" % (dtype, name, report(got, want))
            assert so.same(c_spectrum(lib, L, M, []), so.spectrum(F, []))
            assert c_spectrum(lib, L, M, [2.0, 1.0]) == -1
            assert bytes(C.string_at(C.addressof(M.contents), C.sizeof(lib.MC33))) == before
            # the extractor still extracts over its slabs: the count of one isovalue is the spectrum's
            nV, nT = C.c_uint(), C.c_uint()
            L.size_of_isosurface(M, lib.real(isos[len(isos) // 2]), C.byref(nV), C.byref(nT))
            assert (nV.value > 0) == (int(want.cut_cells[len(isos) // 2]) > 0)
            done += 1
        finally:
            L.free_MC33(M)
            L.free_memory_grd(G)
            del keep
    print("SPECTRUM_SLABS_OK %d" % done)


if __name__ == "__main__":
    main()
