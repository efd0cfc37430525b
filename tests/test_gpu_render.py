"""GPU tests of the pictures (include/mc33_hip.h: mc33hip_render_surface; include/marching_cubes_33.h: MC33_render_isosurface;
DeviceGrid.render / extract_rendered).

Every grid case of tests/render_cases.py is extracted on the device and drawn there; the expected images come from
tests/render_oracle.py run on the very mesh that was downloaded.  Everything is compared bit for bit - the colour image, the depth
image, the id image and all counts; nothing here has a tolerance.  The three images sit in canaried tensors (tests/mesh_harness.py:
CanariedCall)."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import render_cases as rc
import render_oracle as ro
from mc33_c_library_amd.api import Image, View
from mesh_harness import CanariedCall, capi, device_grid, tiny_grid, to_device

pytestmark = pytest.mark.gpu

EINVAL, ERUNTIME = -1, -5
RGBA, DEPTH, IDS = 1, 2, 4
_grids, _meshes, _ctx = {}, {}, {}


def grid(name):
    """the case and a context on its grid, made once per case and module"""
    if name not in _grids:
        c = rc.case(name)
        _grids[name] = (c, device_grid(c.data, r0=c.r0, d=c.d))
    return _grids[name]


def extracted(name):
    """the case's surface as the device extracts it, on the host, with colour words: a mesh like render_cases' made-up ones"""
    if name not in _meshes:
        c, g = grid(name)
        V, N, T, cnt = g.extract(c.iso)
        m = rc.mesh(V.cpu().numpy(), T.cpu().numpy().view(np.uint32), dtype=np.float64 if c.dtype == "f64" else np.float32)
        m.N = N.cpu().numpy()
        for a in (m.V, m.N, m.T, m.C):
            a.setflags(write=False)
        _meshes[name] = m
    return _meshes[name]


def plain():
    """a context for meshes that come from no grid, one per module"""
    if "plain" not in _ctx:
        _ctx["plain"] = tiny_grid()
    return _ctx["plain"]


def variant(vw, **kw):
    d = dict(vars(vw))
    d.update(kw)
    return ro.view(d["m"], d["width"], d["height"], d["cull"], d["two_sided"], d["light"], d["ambient"], d["diffuse"], d["background"])


class Call(CanariedCall):
    """one mc33hip_render_surface call: the mesh uploaded, the images `want` names in canaried tensors of width x height words"""

    def __init__(self, g, m, vw, want=RGBA | DEPTH | IDS, colours=True, base_color=0xFF5C5C5C, change=None, fill_from=None):
        import torch
        from mc33_c_library_amd.api import Rendering
        super().__init__(g)
        self.pixels, self.want = vw.width * vw.height, want
        nV, nT = m.V.shape[0], m.T.shape[0]
        self.dV = to_device(m.V) if nV else torch.empty((0, 3), dtype=torch.float32, device="cuda")
        self.dN = to_device(m.N) if nV else torch.empty((0, 3), dtype=torch.float32, device="cuda")
        self.dT = to_device(m.T) if nT else torch.empty((0, 3), dtype=torch.int32, device="cuda")
        self.dC = to_device(m.C) if colours and nV else None
        self.img = [self.room(self.pixels, 0, dt) if want >> b & 1 else None for b, dt in enumerate((torch.int32, torch.float32, torch.int32))]
        self.before = self.all_bytes()
        a = Rendering()
        a.V, a.N, a.T, a.nV, a.nT = (self.dV.data_ptr() if nV else None), (self.dN.data_ptr() if nV else None), (self.dT.data_ptr() if nT else None), nV, nT
        a.C = self.dC.data_ptr() if self.dC is not None else None
        a.m, a.light = (C.c_double * 16)(*vw.m), (C.c_double * 3)(*vw.light)
        a.width, a.height, a.cull, a.two_sided = vw.width, vw.height, vw.cull, vw.two_sided
        a.ambient, a.diffuse, a.background, a.base_color = vw.ambient, vw.diffuse, vw.background, base_color
        a.oRGBA, a.oDepth, a.oTri = (x.data_ptr() if x is not None else None for x in self.img)
        self.call(g.lib.mc33hip_render_surface, a, change)
        self.counts = tuple(int(getattr(a, n)) for n in ro.COUNTS)

    def outputs(self):
        return [(x, self.pixels) for x in self.img]

    def check(self, want):
        """bit for bit against the oracle; the canaries behind the images still hold FILL"""
        assert self.counts == want.counts(), (dict(zip(ro.COUNTS, self.counts)), dict(zip(ro.COUNTS, want.counts())))
        for x, ref, label in zip(self.img, (want.rgba, want.depth, want.tri), ("rgba", "depth", "ids")):
            if x is not None:
                self.equal_bits(label, x[:self.pixels], ref.reshape(-1))
        self.spare_intact()

    def untouched(self):
        assert self.all_bytes() == self.before, "a refused call wrote to its images"


# ---- surfaces ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cull", [0, 1, 2])
@pytest.mark.parametrize("two_sided", [1, 0])
def test_sphere_bit_for_bit(cull, two_sided):
    c, g = grid("sphere")
    m = extracted("sphere")
    vw = variant(c.view, cull=cull, two_sided=two_sided)
    want = ro.render(m.V, m.N, m.T, m.C, vw)
    print("    sphere cull %d two_sided %d: %r" % (cull, two_sided, dict(zip(ro.COUNTS, want.counts()))))
    assert want.covered > 800 and (want.culled > 0) == (cull != 0)
    call = Call(g, m, vw)
    assert call.rc == 0, call.message
    call.check(want)
    base = Call(g, m, vw, colours=False, base_color=0xFF4080C0)  # no colour array: base_color for every vertex
    assert base.rc == 0, base.message
    base.check(ro.render(m.V, m.N, m.T, None, vw, base_color=0xFF4080C0))


@pytest.mark.parametrize("name", ["noise16", "inside", "f64"])
def test_grid_cases_bit_for_bit(name):
    c, g = grid(name)
    m = extracted(name)
    want = ro.render(m.V, m.N, m.T, m.C, c.view)
    print("    %s: %r" % (name, dict(zip(ro.COUNTS, want.counts()))))
    assert want.covered > 500 and (name != "inside" or want.rejected > 0) and (name != "f64" or m.V.dtype == np.float64)
    call = Call(g, m, c.view)
    assert call.rc == 0, call.message
    call.check(want)
    culled = variant(c.view, cull=1, two_sided=0)
    call = Call(g, m, culled)
    assert call.rc == 0, call.message
    call.check(ro.render(m.V, m.N, m.T, m.C, culled))


# ---- made-up meshes ------------------------------------------------------------------------------------------------------------

def test_lattice_meshes():
    for seed in range(24):
        m, vw, inside = rc.lattice(seed)
        want = ro.render(m.V, m.N, m.T, m.C, vw)
        call = Call(plain(), m, vw)
        assert call.rc == 0, call.message
        call.check(want)
        assert call.counts[6] == call.counts[7] == inside


def test_a_quad_over_the_whole_viewport():
    m, vw = rc.quad(512, 384)
    want = ro.render(m.V, m.N, m.T, m.C, vw)
    assert want.covered == 512 * 384 == want.fragments and want.drawn == 2
    for cull in (0, 1, 2):
        call = Call(plain(), m, variant(vw, cull=cull))
        assert call.rc == 0, call.message
        call.check(want if cull == 0 else ro.render(m.V, m.N, m.T, m.C, variant(vw, cull=cull)))


def test_the_guard_band_at_4096():
    """a corner on the guard band's limit is drawn, one two steps beyond it rejects its triangle: ids, depth and counts"""
    m, vw = rc.guard()
    want = ro.render(m.V, m.N, m.T, m.C, vw, shade=False)
    assert (want.drawn, want.rejected, want.offscreen, want.covered) == (1, 1, 1, 4096 * 4096)
    call = Call(plain(), m, vw, want=DEPTH | IDS)
    assert call.rc == 0, call.message
    call.check(want)


def test_invalid_indices_are_counted_not_read():
    m0, vw, _ = rc.lattice(3)
    m = rc.with_bad_indices(m0)
    want = ro.render(m.V, m.N, m.T, m.C, vw)
    assert want.invalid_triangles == 3
    call = Call(plain(), m, vw)
    assert call.rc == ERUNTIME and "3 triangles" in call.message
    call.check(want)


def test_nonfinite_vertices_tiny_triangles_and_empty_meshes():
    m0, vw, _ = rc.lattice(7)
    m = rc.with_nonfinite(m0)
    want = ro.render(m.V, m.N, m.T, m.C, vw)
    assert want.rejected >= 3
    call = Call(plain(), m, vw)
    assert call.rc == 0, call.message
    call.check(want)
    t, tv = rc.tiny()
    want = ro.render(t.V, t.N, t.T, t.C, tv)
    assert want.degenerate >= 15
    call = Call(plain(), t, tv)
    assert call.rc == 0, call.message
    call.check(want)
    import types
    for empty in (types.SimpleNamespace(V=t.V, N=t.N, T=t.T[:0], C=t.C), types.SimpleNamespace(V=t.V[:0], N=t.N[:0], T=t.T[:0], C=t.C[:0])):
        want = ro.render(empty.V, empty.N, empty.T, empty.C, tv)
        call = Call(plain(), empty, tv)
        assert call.rc == 0 and call.counts == (0,) * 8, call.message
        call.check(want)
    # triangles over vertices that are not there: all invalid
    none = types.SimpleNamespace(V=t.V[:0], N=t.N[:0], T=t.T, C=t.C[:0])
    call = Call(plain(), none, tv)
    assert call.rc == ERUNTIME and call.counts[5] == t.T.shape[0]
    call.check(ro.render(none.V, none.N, none.T, none.C, tv))


# ---- the two paths, the outputs, repeated calls ---------------------------------------------------------------------------------

def test_the_path_limit_changes_no_byte(monkeypatch):
    """MC33_HIP_RENDER_SMALL is read when a context is created: 0 sends every triangle down the tiled path, a huge value every
    triangle down the path of one lane, and the default splits them"""
    c, _ = grid("sphere")
    ms = extracted("sphere")
    mq, vq = rc.quad(512, 384)
    want_s, want_q = ro.render(ms.V, ms.N, ms.T, ms.C, c.view), ro.render(mq.V, mq.N, mq.T, mq.C, vq)
    seen = []
    for value in ("0", None, "4000000000"):
        if value is None:
            monkeypatch.delenv("MC33_HIP_RENDER_SMALL", raising=False)
        else:
            monkeypatch.setenv("MC33_HIP_RENDER_SMALL", value)
        g = tiny_grid()
        try:
            a, b = Call(g, ms, c.view), Call(g, mq, vq)
            assert a.rc == 0 and b.rc == 0, (value, a.message, b.message)
            a.check(want_s)
            b.check(want_q)
            seen.append((a.all_bytes(), b.all_bytes()))
        finally:
            g.close()
    assert seen[0] == seen[1] == seen[2]


def test_every_output_may_be_null():
    c, g = grid("sphere")
    m = extracted("sphere")
    want = ro.render(m.V, m.N, m.T, m.C, c.view)
    for bits_ in (DEPTH | IDS, RGBA | IDS, RGBA | DEPTH, RGBA, DEPTH, IDS, 0):
        call = Call(g, m, c.view, want=bits_)
        assert call.rc == 0, call.message
        call.check(want)


def test_two_calls_give_the_same_bytes():
    c, g = grid("noise16")
    m = extracted("noise16")
    want = ro.render(m.V, m.N, m.T, m.C, c.view)
    first, second = Call(g, m, c.view), Call(g, m, c.view)
    assert first.rc == 0 and second.rc == 0 and first.all_bytes() == second.all_bytes()
    second.check(want)
    # a larger image first, a smaller one second: nothing of the first is left in the scratch
    mq, vq = rc.quad(512, 384)
    big = Call(g, mq, vq)
    assert big.rc == 0
    g.extract(0.3)
    third = Call(g, m, c.view)
    assert third.rc == 0 and third.all_bytes() == first.all_bytes()
    cs, gs = grid("sphere")
    small = Call(g, extracted("sphere"), cs.view)  # (another mesh on this context, after the larger one)
    small.check(ro.render(extracted("sphere").V, extracted("sphere").N, extracted("sphere").T, extracted("sphere").C, cs.view))


def test_refusals_leave_the_images_alone():
    c, g = grid("sphere")
    m = extracted("sphere")
    nan, inf = float("nan"), float("inf")
    changes = [{"width": 0}, {"height": 0}, {"width": 4097}, {"height": 5000}, {"m5": nan}, {"m9": inf}, {"light1": nan}, {"ambient": inf}, {"diffuse": nan},
               {"light": (0.0, 0.0, 0.0)}, {"cull": 3}, {"cull": -1}, {"nV": 1 << 32}, {"nT": 1 << 32}, {"V": None}, {"N": None}, {"T": None}]
    for change in changes:
        call = Call(g, m, c.view, change=change)
        assert call.rc == EINVAL and call.counts == (0,) * 8, (change, call.rc, call.message)
        call.untouched()
    # an inclined context and a z-slab context are accepted: the call reads only the arrays it is given
    want = ro.render(m.V, m.N, m.T, m.C, c.view)
    gi = device_grid(c.data, r0=c.r0, d=c.d)
    gi.set_inclined([[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[1.0, -0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    call = Call(gi, m, c.view)
    assert call.rc == 0, call.message
    call.check(want)
    gi.close()
    from mc33_c_library_amd import DeviceGrid
    gs = DeviceGrid(to_device(c.data)[2:7].contiguous(), nz_total=c.data.shape[0] - 1, plane0=2)
    call = Call(gs, m, c.view)
    assert call.rc == 0, call.message
    call.check(want)
    gs.close()


# ---- Python and the C API --------------------------------------------------------------------------------------------------------

def as_view(vw):
    v = View()
    v.m, v.light = (C.c_double * 16)(*vw.m), (C.c_double * 3)(*vw.light)
    v.width, v.height, v.cull, v.two_sided, v.ambient, v.diffuse, v.background = vw.width, vw.height, vw.cull, vw.two_sided, vw.ambient, vw.diffuse, vw.background
    return v


def test_python_methods():
    c, g = grid("sphere")
    m = extracted("sphere")
    want = ro.render(m.V, m.N, m.T, None, c.view, base_color=0xFF5C5C5C)
    rgba, depth, ids, info = g.extract_rendered(c.iso, as_view(c.view))
    assert tuple(info[n] for n in ro.COUNTS) == want.counts() and (info["nV"], info["nT"]) == (m.V.shape[0], m.T.shape[0])
    assert np.array_equal(rgba.cpu().numpy().view(np.uint32), want.rgba) and np.array_equal(ids.cpu().numpy().view(np.uint32), want.tri)
    assert np.array_equal(depth.cpu().numpy().view(np.uint32), want.depth.view(np.uint32))
    rgba, depth, ids, info = g.render(to_device(m.V), to_device(m.N), to_device(m.T), to_device(m.C), as_view(c.view), want=RGBA)
    assert depth is None and ids is None and np.array_equal(rgba.cpu().numpy().view(np.uint32), ro.render(m.V, m.N, m.T, m.C, c.view).rgba)
    ms = (C.c_float * 6)()
    assert g.lib.mc33hip_render_timing(g.ctx, C.byref(ms)) == EINVAL  # (the context was made without MC33_HIP_TIMING=2: no events, no times)
    from mc33_c_library_amd import MC33Error
    with pytest.raises(MC33Error):
        g.render(to_device(m.V), to_device(m.N), to_device(m.T), None, as_view(variant(c.view, cull=5)))


def c_view(vw):
    v = View()
    v.m, v.light = (C.c_double * 16)(*vw.m), (C.c_double * 3)(*vw.light)
    v.width, v.height, v.cull, v.two_sided, v.ambient, v.diffuse, v.background = vw.width, vw.height, vw.cull, vw.two_sided, vw.ambient, vw.diffuse, vw.background
    return v


def host_image(img, which, dtype):
    p = getattr(img, which)
    return np.ctypeslib.as_array(p, (img.height, img.width)).view(dtype).copy() if p else None


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_c_api(dtype, monkeypatch, tmp_path):
    """two views of one extraction, colours from a property grid through a colour map: the images are the oracle's rendering of
    what calculate_isosurface returns, colours included; only the arrays asked for come back; the object is left as specified"""
    monkeypatch.delenv("MC33_HIP_DEVICES", raising=False)
    lib = capi(dtype)
    L = lib.lib
    if dtype == "f32":
        data, iso = np.ascontiguousarray(rc.ball((20, 22, 24), (11.3, 10.6, 9.4), 7.7).astype(np.float32)), 0.0
    else:
        data, iso = np.ascontiguousarray(np.clip(np.rint(1000.0 + 10.0 * rc.ball((20, 22, 24), (11.3, 10.6, 9.4), 7.7)), 0, 65535).astype(np.uint16)), 1000.5
    prop = np.ascontiguousarray((np.random.default_rng(4).standard_normal(data.shape) * (10 if dtype == "u16" else 1) + (100 if dtype == "u16" else 0)).astype(lib.np_dtype))
    G, keep = lib.make_grid(data)
    Pg, keep2 = lib.make_grid(prop)
    M = L.create_MC33(G)
    assert M
    try:
        pal = [int((0xff000000 if k % 2 else 0x7f000000) | ((k * 2654435761) & 0xffffff)) for k in range(9)]
        cpal = (C.c_int * len(pal))(*[int(x) for x in np.array(pal, np.uint32).view(np.int32)])
        lo, hi = (80.0, 120.0) if dtype == "u16" else (-1.5, 1.5)
        assert L.MC33_set_property_grid(M, Pg) == 0 and L.MC33_set_color_map(M, cpal, len(pal), lo, hi) == 0
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        s = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert len(np.unique(s.color)) > 3
        before = (M.contents.nV, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        eye, target = (44.0, 36.0, 31.0), (11.3, 10.6, 9.4)
        views = [ro.view(rc.perspective(eye, target, (0, 0, 1), 30.0, 80, 56, 25.0, 75.0), 80, 56, light=(1.0, 0.5, 0.8), background=0xFF102030),
                 ro.view(rc.orthographic(target, (-1.0, 0.3, -0.4), (0, 0, 1), 10.0, 48, 64, -15.0, 15.0), 48, 64, cull=1, two_sided=0, light=(1.0, -0.3, 0.4))]
        cviews = (View * 2)(*[c_view(v) for v in views])
        for want in (RGBA | DEPTH | IDS, RGBA, DEPTH | IDS):
            out = (Image * 2)()
            assert L.MC33_render_isosurface(M, lib.real(iso), cviews, 2, want, out) == 2
            assert (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == (lib.np_real(iso),) + before
            for vw, img in zip(views, out):
                ref = ro.render(s.V, s.N, s.T, s.color.view(np.uint32), vw)
                assert (img.width, img.height, img.nV, img.nT) == (vw.width, vw.height, s.nV, s.nT) and ref.covered > 500
                assert (img.drawn, img.culled, img.degenerate, img.rejected, img.offscreen, img.invalid_triangles, img.fragments, img.covered) == ref.counts()
                got = [host_image(img, "rgba", np.uint32), host_image(img, "depth", np.uint32), host_image(img, "triangle", np.uint32)]
                for b, (x, r) in enumerate(zip(got, (ref.rgba, ref.depth.view(np.uint32), ref.tri))):
                    assert (x is not None) == bool(want >> b & 1)
                    assert x is None or np.array_equal(x, r), ("rgba", "depth", "ids")[b]
                if want & RGBA:
                    path = str(tmp_path / "view.ppm")
                    assert L.MC33_write_image_ppm(C.byref(img), path.encode()) == 0
                    raw = open(path, "rb").read()
                    assert raw[-3:] == bytes([int(ref.rgba[-1, -1]) & 255, int(ref.rgba[-1, -1]) >> 8 & 255, int(ref.rgba[-1, -1]) >> 16 & 255])
                L.MC33_free_image(C.byref(img))
                assert not img.rgba and not img.depth and not img.triangle
        # without the map: DefaultColorMC for every vertex
        assert L.MC33_set_color_map(M, None, 0, 0.0, 0.0) == 0
        out = (Image * 1)()
        assert L.MC33_render_isosurface(M, lib.real(iso), cviews, 1, RGBA, out) == 1
        ref = ro.render(s.V, s.N, s.T, None, views[0], base_color=0xFF5C5C5C)
        assert np.array_equal(host_image(out[0], "rgba", np.uint32), ref.rgba)
        L.MC33_free_image(C.byref(out[0]))
        # a refused view: the object and out are left alone
        out[0].width, out[0].covered = 77, 9
        state = (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault)
        bad = (View * 2)(c_view(views[0]), c_view(variant(views[1], cull=7)))
        assert L.MC33_render_isosurface(M, lib.real(iso + 1), bad, 2, 7, out) == -1 and L.MC33_render_isosurface(M, lib.real(iso + 1), cviews, 2, 8, out) == -1
        assert (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault) == state and (out[0].width, out[0].covered) == (77, 9) and not out[0].rgba
        # MC33_view_fit frames the grid: most of the ball is in the picture
        v = View()
        D3 = C.c_double * 3
        assert L.MC33_view_fit(M, C.byref(D3(-1.0, -0.8, -0.5)), C.byref(D3(0, 0, 1)), 35.0, 64, 64, C.byref(v)) == 0
        one = (Image * 1)()
        assert L.MC33_render_isosurface(M, lib.real(iso), C.pointer(v), 1, IDS, one) == 1
        assert one[0].rejected == 0 and one[0].offscreen + one[0].drawn + one[0].degenerate == s.nT and one[0].covered > 300
        L.MC33_free_image(C.byref(one[0]))
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        L.free_memory_grd(Pg)
        del keep, keep2


def test_c_api_refuses_several_slabs(monkeypatch):
    """MC33_HIP_DEVICES is read by create_MC33: an object on three slabs refuses to render, is left alone, and still extracts"""
    lib = capi("f32")
    L = lib.lib
    c = rc.case("sphere")
    monkeypatch.delenv("MC33_HIP_DEVICES", raising=False)
    G, keep = lib.make_grid(c.data)
    M = L.create_MC33(G)
    S = L.calculate_isosurface(M, lib.real(c.iso))
    one = lib.copy_surface(S)
    L.free_surface_memory(S)
    L.free_MC33(M)
    monkeypatch.setenv("MC33_HIP_DEVICES", "0,0,0")
    M = L.create_MC33(G)
    assert M
    try:
        out = (Image * 1)()
        out[0].width = 77
        state = (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault)
        assert L.MC33_render_isosurface(M, lib.real(c.iso), C.pointer(c_view(c.view)), 1, 7, out) == -1
        assert (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault) == state and out[0].width == 77 and not out[0].rgba
        v = View()
        D3 = C.c_double * 3
        assert L.MC33_view_fit(M, C.byref(D3(1, 0, 0)), C.byref(D3(0, 0, 1)), 0.0, 32, 32, C.byref(v)) == 0  # (host only: no slab is asked)
        S = L.calculate_isosurface(M, lib.real(c.iso))
        assert S
        s = lib.copy_surface(S)
        L.free_surface_memory(S)
        assert s.V.tobytes() == one.V.tobytes() and s.T.tobytes() == one.T.tobytes()
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
