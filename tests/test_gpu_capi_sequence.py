"""The C API's calls that work on an extracted surface, one after another on ONE MC33 object: they share the object's two staging
sets, its label and property words and the host frame around every call, so what one call leaves behind -
rows, capacities, a set without a colour array - is what the next one starts from.  After every step the result must be, bit for
bit, what the same call returns on an object created for that call alone - which is what each part's own test_c_api pins to the
oracles - and the object's public prefix must be as calculate_isosurface leaves it."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
from clip_cases import cbox, cclip
from mc33_c_library_amd.api import ComponentFilter, SurfaceSmoothing
from mc33_capi import SURFACE, CMeasure
from mesh_harness import c_palette, capi, palette
from simplify_cases import csimp

pytestmark = pytest.mark.gpu

PALETTE, MAP_LO, MAP_HI = palette(7), -2.5, 3.25


def rows(s):
    """every count and array of a host copy of a surface, as bytes where the bits matter (capv / capt are the host blocks')"""
    return (s.nV, s.nT, np.float32(s.iso).tobytes(), s.V.tobytes(), s.N.tobytes(), s.T.tobytes(), s.color.tobytes())


class Calls:
    """the f32 product library, every prototype declared (tests/mc33_capi.py)"""

    def __init__(self):
        self.lib = capi()
        self.L = self.filt = self.clip = self.simp = self.smooth = self.lib.lib

    def surface(self, M, iso, S):
        """a derived surface copied and freed, after the checks of clipped_surface() in tests/test_gpu_clip.py"""
        assert S
        try:
            m, r = M.contents, S.contents
            assert (m.nV, m.nT, m.memoryfault, m.iso) == (0, r.nT, 0, np.float32(iso))  # as calculate_isosurface leaves them
            if r.nV:  # the object's public prefix mirrors the returned surface
                assert (m.T, m.V, m.N, m.color, m.capt, m.capv) == (r.T, r.V, r.N, r.color, r.capt, r.capv)
            return rows(self.lib.copy_surface(S))
        finally:
            self.L.free_surface_memory(S)

    def filtered(self, M, iso):
        f, k, dr = ComponentFilter(largest=1), C.c_uint(77), C.c_uint(77)
        S = self.filt.MC33_calculate_filtered_isosurface(M, C.c_float(iso), C.byref(f), C.byref(k), C.byref(dr))
        return self.surface(M, iso, S) + (k.value, dr.value)

    def clipped(self, M, iso, cl):
        return self.surface(M, iso, self.clip.MC33_calculate_clipped_isosurface(M, C.c_float(iso), C.byref(cl)))

    def simplified(self, M, iso):
        sp = csimp((2.0, 2.0, 2.0), 0, 1)
        return self.surface(M, iso, self.simp.MC33_calculate_simplified_isosurface(M, C.c_float(iso), C.byref(sp)))

    def smoothed(self, M, iso):
        sm = SurfaceSmoothing(3, 0.5, -0.53, 1)
        return self.surface(M, iso, self.smooth.MC33_calculate_smoothed_isosurface(M, C.c_float(iso), C.byref(sm)))

    def measured(self, M, iso):
        m = CMeasure()
        assert self.L.MC33_measure_isosurface(M, C.c_float(iso), C.byref(m)) == 0
        assert M.contents.iso == np.float32(iso) and M.contents.memoryfault == 0
        return (bytes(m),)

    def several(self, M, isos):
        out = (C.POINTER(SURFACE) * len(isos))()
        assert self.L.calculate_isosurfaces(M, (C.c_float * len(isos))(*isos), len(isos), out) == len(isos)
        assert M.contents.iso == np.float32(isos[-1]) and M.contents.memoryfault == 0
        got = ()
        for S in out:
            got += rows(self.lib.copy_surface(S))
            self.L.free_surface_memory(S)
        return got


def test_one_object_through_every_derived_call():
    c = Calls()
    lib, L = c.lib, c.L
    data, r0, d = fx.cos_field(64)  # the "sheet" of tests/measure_oracle.py: 15072 vertices at 0, far fewer at 2.5
    G, keep = lib.make_grid(data, r0, d)
    Pg, keep2 = lib.make_grid(fx.noise_f32(0, 79, shape=data.shape) * np.float32(10.0), r0, d)
    box, _ = cbox(lib, (-2.0, -2.0, -2.0), (1.6, 1.6, 1.6))
    one = cclip([(1.0, 0.5, 0.25, 0.125)])

    def colour_map(M):
        assert c.filt.MC33_set_color_map(M, c_palette(PALETTE), len(PALETTE), MAP_LO, MAP_HI) == 0

    def property_grid(M):
        assert c.filt.MC33_set_property_grid(M, Pg) == 0

    # (what the shared object goes through before the call, the call): the former is also how a fresh object is made ready
    steps = [
        ("filtered", (), lambda M: c.filtered(M, 0.0)),
        ("clipped by a box", (), lambda M: c.clipped(M, 0.0, box)),
        ("simplified, much smaller", (), lambda M: c.simplified(M, 2.5)),
        ("filtered with colours: set 1 has rows but no colour array", (property_grid, colour_map), lambda M: c.filtered(M, 0.0)),
        ("smoothed", (), lambda M: c.smoothed(M, 0.0)),
        ("measured", (), lambda M: c.measured(M, 0.0)),
        ("three isovalues", (), lambda M: c.several(M, (0.0, 1.0, 2.5))),
        ("clipped by one plane", (), lambda M: c.clipped(M, 0.0, one)),
        ("clipped without the property grid", (lambda M: c.filt.MC33_set_property_grid(M, None),), lambda M: c.clipped(M, 0.0, one)),
    ]
    M = L.create_MC33(G)
    assert M
    try:
        state = []  # the settings the shared object has by now
        results = {}
        for name, settings, call in steps:
            for s in settings:
                s(M)
            state += settings
            got = call(M)
            F = L.create_MC33(G)
            assert F
            try:
                for s in state:
                    s(F)
                want = call(F)
            finally:
                L.free_MC33(F)
            assert len(got) == len(want)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a == b, "%s: element %d differs from a fresh object's" % (name, k)
            results[name] = got
        # the steps did what the sequence is for
        assert results["filtered"][:2] == (15072, 29432) and results["filtered"][-2:] == (1, 0)
        assert 0 < results["clipped by a box"][0] < 15072 and 0 < results["simplified, much smaller"][0] < 15072 // 4
        painted = np.frombuffer(results["filtered with colours: set 1 has rows but no colour array"][6], np.int32)
        assert painted.size == 15072 and np.unique(painted).size > 2
        assert np.unique(np.frombuffer(results["clipped by one plane"][6], np.int32)).size > 2
        assert np.unique(np.frombuffer(results["clipped without the property grid"][6], np.int32)).size == 1
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2
