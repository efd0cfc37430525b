"""Pictures of an isosurface, the part that needs no GPU: the numpy oracle (tests/render_oracle.py) on made-up meshes
and on surfaces of the CPU extractor held to facts it does not compute itself - pixel centres of a lattice counted by hand, points
unprojected back onto their triangles, the side the stored normals point to -, MC33_view_fit through the host-logic build of
mc33_capi.c (it needs no device), the new names in the headers, the libraries and the code objects, the struct layouts, the
host-logic build's refusal to render, and the PPM writer.

The tests over render_cases pin the oracle and pass without the feature; the name, export, code-object, layout, host-logic and PPM
tests fail without it.  On the device the product is held to the oracle bit for bit by tests/test_gpu_render.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_cases as rc
import render_oracle as ro
from mc33_c_library_amd.api import Image, View
from mesh_checks import assert_exported, assert_kernels, host_logic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HIP_NAMES = ["mc33hip_render_surface", "mc33hip_render_timing"]
C_NAMES = ["MC33_render_isosurface", "MC33_free_image", "MC33_view_fit", "MC33_write_image_ppm"]
KERNELS = ["k_render_clear", "k_render_tiles"]
WIDE_KERNELS = ["k_render_triangles", "k_render_resolve"]  # three corners in doubles and int64 edge functions: 80 registers, six waves per SIMD

_surfaces, _renders = {}, {}


def surface(oracles, name):
    """(case, V, N, T, colour words) of a grid case as the CPU extractor makes it, once"""
    if name not in _surfaces:
        c = rc.case(name)
        s = oracles[c.dtype].isosurface(c.data, c.iso, c.r0, c.d)
        for a in (s.V, s.N, s.T):
            a.setflags(write=False)
        _surfaces[name] = (c, s.V, s.N, s.T, rc.colour_words(s.nV))
    return _surfaces[name]


def rendered(oracles, name, cull=0, two_sided=1):
    key = (name, cull, two_sided)
    if key not in _renders:
        c, V, N, T, words = surface(oracles, name)
        vw = ro.view(c.view.m, c.view.width, c.view.height, cull, two_sided, c.view.light, c.view.ambient, c.view.diffuse, c.view.background)
        _renders[key] = ro.render(V, N, T, words, vw)
    return _renders[key]


# ---- the oracle against independent facts -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", range(6))
def test_lattice_meshes_cover_every_pixel_centre_once(block):
    """300 lattice meshes: every pixel centre inside the outline gets exactly one fragment, whatever the diagonals and windings"""
    for seed in range(block * 50, block * 50 + 50):
        m, vw, inside = rc.lattice(seed)
        o = ro.render(m.V, m.N, m.T, m.C, vw)
        assert o.fragments == o.covered == inside, (seed, o.counts(), inside)
        assert int((o.tri != ro.NOTRI).sum()) == inside and o.invalid_triangles == 0 and o.rejected == 0 and o.culled == 0
        assert o.drawn + o.offscreen + o.degenerate == m.T.shape[0]
        assert np.all(o.depth[o.tri != ro.NOTRI] == np.float32(0.5)) and np.all(np.isposinf(o.depth[o.tri == ro.NOTRI]))
        assert np.all(o.rgba[o.tri == ro.NOTRI] == vw.background) and np.all(o.rgba[o.tri != ro.NOTRI] >> 24 == 255)


def unproject(m, width, height, sx, sy, depth):
    """the points whose clip coordinates divide to the screen position (sx, sy) in pixels and to `depth`"""
    inv = np.linalg.inv(np.asarray(m, np.float64).reshape(4, 4))
    ndc = np.stack([2.0 * sx / width - 1.0, 1.0 - 2.0 * sy / height, depth, np.ones_like(depth)], axis=1)
    q = ndc @ inv.T
    return q[:, :3] / q[:, 3:4]


def test_unprojected_pixels_lie_on_their_triangles(oracles):
    """Every covered pixel of the sphere, unprojected from (its centre, oDepth), lies in the plane of triangle oTri and inside it.
    The bound is derived.  (1) The rasteriser works on corners snapped to 1/256 pixel: S_i = s_i + e_i with |e_i| <= 1/512 pixel per
    axis.  The depth it interpolates at the centre P with the barycentrics b of the snapped triangle is the TRUE plane's depth at
    P* = sum b_i s_i = P - sum b_i e_i, a point of the true triangle (b_i >= 0, sum 1) at most 1/512 pixel from P per axis: the
    unprojected point is within |unproject(P, d) - unproject(P +- (1/512, 1/512), d)| of a point of the triangle.  (2) oDepth is
    the depth rounded to float: d (1 +- 2^-24), which moves the point by |unproject(P, d (1 + 2^-24)) - unproject(P, d)|.  (3) The
    float64 arithmetic of this test and of the oracle: 1e-9 of the largest coordinate, far above it.  On the sphere the bound comes
    to 7.0e-4 .. 8.4e-4 grid units (the snapping, almost all of it; a pixel is 0.2 units wide there) and the largest distance to 4.7e-4."""
    c, V, N, T, _ = surface(oracles, "sphere")
    o = rendered(oracles, "sphere")
    W, H = c.view.width, c.view.height
    ys, xs = np.nonzero(o.tri != ro.NOTRI)
    assert ys.size > 800
    cx, cy, d = xs + 0.5, ys + 0.5, o.depth[ys, xs].astype(np.float64)
    Q = unproject(c.view.m, W, H, cx, cy, d)
    bound = np.zeros(ys.size)
    for ox, oy in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
        bound = np.maximum(bound, np.sqrt(((unproject(c.view.m, W, H, cx + ox / 512.0, cy + oy / 512.0, d) - Q) ** 2).sum(axis=1)))
    bound += np.sqrt(((unproject(c.view.m, W, H, cx, cy, d * (1.0 + 2.0 ** -24)) - Q) ** 2).sum(axis=1)) + 1e-9 * np.abs(V).max()
    P = V.astype(np.float64)[T[o.tri[ys, xs]].astype(np.int64)]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    off = np.abs(((Q - P[:, 0]) * n).sum(axis=1))
    worst = off.copy()
    for e in range(3):  # the signed distance from every edge, in the plane, positive inside
        a, b = P[:, e], P[:, (e + 1) % 3]
        inward = np.cross(n, b - a)
        inward /= np.sqrt((inward * inward).sum(axis=1))[:, None]
        worst = np.maximum(worst, -((Q - a) * inward).sum(axis=1))
    print("    sphere: %d pixels, largest distance %.3g, bound %.3g .. %.3g" % (ys.size, worst.max(), bound.min(), bound.max()))
    assert np.all(off <= bound) and np.all(worst <= bound)


def test_the_front_is_the_side_the_normals_point_to(oracles):
    """The sphere's field falls outwards, so its stored normals point outwards; seen from outside, culling the back changes nothing
    and culling the front shows the far side.  That area2 < 0 is the side N points to is held in two steps, because N is a normal
    per VERTEX - the field's gradient - and the facing is decided by the flat triangle: along the silhouette a triangle that faces
    the eye has corners behind the horizon, whose N points away from it however finely the sphere is sampled (46 of the 887 drawn
    triangles here; 70 of 4820 at 64^3 samples).  (1) N lies on the side of the normal by winding g = (P1 - P0) x (P2 - P0): g . N > 0
    at every corner of every triangle with an area.  (2) A triangle that cull 1 draws has g . (eye - P0) > 0 - a projective map with
    cw > 0 keeps the orientation - unless the snapping to 1/256 pixel decided it: |area2 of the unsnapped corners| is then at
    most the sum over the edges of |dx| + |dy| (every corner moves by 1/2 at most per axis, in 1/256 pixel) plus 2."""
    c, V, N, T, _ = surface(oracles, "sphere")
    both, back, front = (rendered(oracles, "sphere", cull) for cull in (0, 1, 2))
    assert np.array_equal(both.tri, back.tri) and np.array_equal(both.depth.view(np.uint32), back.depth.view(np.uint32)) and np.array_equal(both.rgba, back.rgba)
    assert back.culled > 0 and front.culled > 0 and back.culled + front.culled + both.degenerate + both.rejected == T.shape[0]
    for o in (both, back, front):
        assert o.drawn + o.culled + o.degenerate + o.rejected + o.offscreen + o.invalid_triangles == T.shape[0]
    assert both.culled == 0 and both.drawn == back.drawn + front.drawn
    # the triangles cull 1 keeps: the normals of all three corners point to the eye
    vw = ro.view(c.view.m, c.view.width, c.view.height, 1)
    X, Y, _, _, usable = ro.screen(V, vw)
    kept = [i for i in range(T.shape[0]) if usable[T[i]].all() and ro.setup(X, Y, T[i].astype(np.int64), vw)[0] == "drawn"]
    assert len(kept) == back.drawn
    P, Nd = V.astype(np.float64)[T.astype(np.int64)], N.astype(np.float64)[T.astype(np.int64)]
    g = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    area = np.sqrt((g * g).sum(axis=1))
    assert np.all((g[:, None, :] * Nd).sum(axis=2)[area > 0.0] > 0.0)  # (1)
    facing = (g * (np.asarray(c.eye) - P[:, 0])).sum(axis=1)
    m = vw.m.reshape(4, 4)
    clip = np.concatenate([P, np.ones(P.shape[:2] + (1,))], axis=2) @ m.T
    S = np.stack([(clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * vw.width, (0.5 - clip[..., 1] / clip[..., 3] * 0.5) * vw.height], axis=2) * 256.0
    true2 = (S[:, 1, 0] - S[:, 0, 0]) * (S[:, 2, 1] - S[:, 0, 1]) - (S[:, 2, 0] - S[:, 0, 0]) * (S[:, 1, 1] - S[:, 0, 1])
    slack = sum(np.abs(S[:, (e + 1) % 3] - S[:, e]).sum(axis=1) for e in range(3)) + 2.0
    decided = np.abs(true2) > slack
    assert np.all(np.sign(true2[decided]) == -np.sign(facing[decided]))  # the orientation on the screen is the facing
    assert np.all((facing[kept] > 0.0) | ~decided[kept]) and decided[kept].sum() > 0.9 * len(kept)  # (2)
    towards = ((np.asarray(c.eye) - P[kept]) * Nd[kept]).sum(axis=2)
    print("    sphere: %d triangles drawn with cull 1, %d of them with a corner whose N points away from the eye" % (len(kept), (towards <= 0.0).any(axis=1).sum()))
    assert np.all(towards > 0.0, axis=1).sum() > 0.9 * len(kept)
    # the far side: a larger depth wherever both cover, and nothing where the near side covers nothing
    cov = front.tri != ro.NOTRI
    assert cov.sum() > 800 and np.all((both.tri != ro.NOTRI)[cov]) and np.all(front.depth[cov] > both.depth[cov])
    far = front.tri[cov].astype(np.int64)
    assert np.all((facing[far] < 0.0) | ~decided[far])
    # one-sided light leaves the far side at ambient; two-sided light does not
    one = rendered(oracles, "sphere", 2, 0)
    assert np.array_equal(one.tri, front.tri) and not np.array_equal(one.rgba, front.rgba)


def test_equal_depth_goes_to_the_lower_index():
    m, vw = rc.quad(40, 30)
    T = np.concatenate([m.T[::-1], m.T[::-1]])  # triangle 1 at 0 and 2, triangle 0 at 1 and 3
    o = ro.render(m.V, m.N, T, m.C, vw)
    single = ro.render(m.V, m.N, m.T, m.C, vw)
    assert o.fragments == 2 * 40 * 30 and o.covered == 40 * 30 == single.fragments
    assert set(np.unique(o.tri)) == {0, 1}
    assert np.array_equal(o.tri == 0, single.tri == 1) and np.array_equal(o.depth.view(np.uint32), single.depth.view(np.uint32)) and np.array_equal(o.rgba, single.rgba)


def test_cases_show_what_they_are_for(oracles):
    i = rendered(oracles, "inside")
    c, V, N, T, words = surface(oracles, "inside")
    assert i.rejected > 0 and i.covered > 500
    near = ro.render(V, N, T, words, ro.view(rc.perspective(c.eye, (rc.SPHERE_C[0] + 6.0, rc.SPHERE_C[1] + 6.0, rc.SPHERE_C[2] + 1.0), (0.0, 0.0, 1.0), 100.0, 64, 48, 0.01, 30.0), 64, 48))
    assert near.fragments > i.fragments and (near.drawn, near.rejected) == (i.drawn, i.rejected)  # fragments before the near plane were dropped
    n = rendered(oracles, "noise16")
    assert n.degenerate + n.offscreen > 0 and n.fragments > 2 * n.covered and n.covered > 3000
    t, tv = rc.tiny()
    o = ro.render(t.V, t.N, t.T, t.C, tv)
    assert o.degenerate >= 15 and o.offscreen >= 15 and 1 <= o.covered <= o.drawn <= 20
    g, gv = rc.guard()
    X, Y, _, _, usable = ro.screen(g.V, gv)
    assert X[1] == 1 << 23 and Y[2] == 1 << 23 and X[4] == -(1 << 23) and not usable[3] and usable[[0, 1, 2, 4, 5]].all()
    b = rc.with_nonfinite(rc.lattice(7)[0])
    o = ro.render(b.V, b.N, b.T, b.C, rc.lattice(7)[1])
    assert o.rejected >= 3
    e = ro.render(t.V, t.N, t.T[:0], t.C, tv)
    assert e.counts() == (0,) * 8 and np.all(e.rgba == tv.background) and np.all(e.tri == ro.NOTRI)


# ---- MC33_view_fit: host C, through the host-logic build ---------------------------------------------------------------------------

D3 = C.c_double * 3


def fit(L, M, direction, up, fov, width, height, out=None):
    v = out if out is not None else View()
    return L.MC33_view_fit(M, C.byref(D3(*direction)) if direction is not None else None, C.byref(D3(*up)) if up is not None else None, fov, width, height, C.byref(v)), v


INCLINED = [[1.0, 0.3, 0.1], [0.0, 1.0, 0.2], [0.0, 0.0, 1.0]]


@pytest.mark.parametrize("inclined", [False, True])
def test_view_fit_frames_the_box(inclined):
    """the eight corners of the grid's box - of an inclined grid, the sheared box - land inside the viewport with depth in [0, 1]"""
    with host_logic("f32") as h:
        lib = h.lib
        L = lib.lib
        data = np.zeros((7, 10, 13), np.float32)
        r0, d = (1.0, -20.0, 300.0), (0.5, 1.0, 2.0)
        A = np.array(INCLINED) if inclined else np.eye(3)
        G, keep = lib.make_grid(data, r0, d, inclined=(A.tolist(), np.linalg.inv(A).tolist()) if inclined else None)
        M = L.create_MC33(G)
        assert M
        try:
            cells = np.array([12, 9, 6], np.float64)
            corners = np.array([np.asarray(r0) + A @ (np.array([i, j, k]) * cells * np.asarray(d)) for i in (0, 1) for j in (0, 1) for k in (0, 1)])
            for direction, up in (((1, 2, -1), (0, 0, 1)), ((0, 0, -1), (0, 1, 0)), ((-3, 0.5, 0.2), (0.1, 1, 0)), ((1e-30, 0, 0), (0, 0, 1e30))):
                for fov in (0.0, 1.0, 45.0, 170.0):
                    for width, height in ((64, 64), (200, 50), (31, 97), (4096, 1)):
                        rcode, v = fit(L, M, direction, up, fov, width, height)
                        assert rcode == 0, (direction, fov, width, height)
                        X, Y, z, cw, usable = ro.screen(corners, ro.view(list(v.m), width, height))
                        assert usable.all() and np.all((X >= 0) & (X <= 256 * width) & (Y >= 0) & (Y <= 256 * height)), (direction, fov, width, height, X, Y)
                        assert np.all((z >= 0.0) & (z <= 1.0)) and z.min() < 0.01 and z.max() > 0.99, (direction, fov, z)
                        # the box fills the image along one axis at least, up to the margin; orthographic: cw is 1
                        assert max((X.max() - X.min()) / (256.0 * width), (Y.max() - Y.min()) / (256.0 * height)) > (0.9 if fov == 0.0 else 0.5 if fov <= 45.0 else 0.0)
                        assert fov != 0.0 or np.all(cw == 1.0)
                        f = np.asarray(direction, np.float64) / np.linalg.norm(direction)
                        assert np.allclose(list(v.light), -f) and (v.ambient, v.diffuse, v.cull, v.two_sided, v.background) == (0.2, 0.8, 0, 1, 0xFF000000)
                        assert (v.width, v.height) == (width, height)
                        # pixels are square and the image is not mirrored: right x up = -forward on the screen
                        m = np.array(list(v.m)).reshape(4, 4)
                        if fov == 0.0:
                            assert np.isclose(np.linalg.norm(m[0, :3]) * width, np.linalg.norm(m[1, :3]) * height)
                            assert np.dot(np.cross(m[0, :3], m[1, :3]), f) < 0.0
        finally:
            L.free_MC33(M)
            L.free_memory_grd(G)
            del keep


def test_view_fit_refusals():
    with host_logic("f32") as h:
        L = h.lib.lib
        nan, inf = float("nan"), float("inf")
        v = View()
        v.width, v.ambient = 77, 5.0
        bad = [((0, 0, 0), (0, 0, 1), 0.0, 64, 64), ((nan, 0, 1), (0, 0, 1), 0.0, 64, 64), ((1, 0, 0), (0, inf, 1), 0.0, 64, 64), ((1, 0, 0), (0, 0, 0), 0.0, 64, 64),
               ((1, 2, 3), (2, 4, 6), 30.0, 64, 64), ((1, 2, 3), (-1, -2, -3), 30.0, 64, 64), ((1, 0, 0), (0, 0, 1), -1.0, 64, 64), ((1, 0, 0), (0, 0, 1), 170.5, 64, 64),
               ((1, 0, 0), (0, 0, 1), nan, 64, 64), ((1, 0, 0), (0, 0, 1), 30.0, 0, 64), ((1, 0, 0), (0, 0, 1), 30.0, 64, 4097), (None, (0, 0, 1), 30.0, 64, 64),
               ((1, 0, 0), None, 30.0, 64, 64)]
        for direction, up, fov, width, height in bad:
            rcode, _ = fit(L, h.M, direction, up, fov, width, height, v)
            assert rcode == -1 and (v.width, v.ambient) == (77, 5.0), (direction, up, fov, width, height)
        assert L.MC33_view_fit(h.M, C.byref(D3(1, 0, 0)), C.byref(D3(0, 0, 1)), 30.0, 64, 64, None) == -1
        assert L.MC33_view_fit(None, C.byref(D3(1, 0, 0)), C.byref(D3(0, 0, 1)), 30.0, 64, 64, C.byref(v)) == -1
        assert fit(L, h.M, (1, 0, 0), (0, 0, 1), 30.0, 64, 64, v)[0] == 0 and v.width == 64


# ---- names, kernels, structs -------------------------------------------------------------------------------------------------------

def test_new_names_are_declared():
    hip = open(os.path.join(ROOT, "include", "mc33_hip.h")).read()
    pub = open(os.path.join(ROOT, "include", "marching_cubes_33.h")).read()
    assert re.search(r"\bint mc33hip_render_surface\(mc33hip_ctx \*", hip) and re.search(r"\} mc33hip_rendering;", hip)
    assert re.search(r"\bint MC33_render_isosurface\(MC33 \*", pub) and re.search(r"\bvoid MC33_free_image\(mc33_image \*", pub)
    assert re.search(r"\bint MC33_view_fit\(MC33 \*", pub) and re.search(r"\bint MC33_write_image_ppm\(const mc33_image \*", pub)
    assert re.search(r"\} mc33_view;", pub) and re.search(r"\} mc33_image;", pub)
    from mc33_c_library_amd import HIP_API, REFERENCE_API, DeviceGrid, Rendering, build  # noqa: F401
    assert set(HIP_NAMES) <= set(HIP_API) and set(C_NAMES) <= set(REFERENCE_API)
    assert callable(DeviceGrid.render) and callable(DeviceGrid.extract_rendered)
    assert "mc33_render.hip.h" in build.HIP_HEADERS
    kernels = open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "mc33_kernels.hip")).read()
    assert '#include "mc33_cap.hip.h"\n#include "mc33_render.hip.h"\n' in kernels and "k_render_triangles" in kernels  # (behind the parts it builds on)
    assert kernels.index('#include "mc33_mesh.hip.h"') < kernels.index('#include "mc33_render.hip.h"')
    assert " mc33_render.hip.h" in open(os.path.join(ROOT, "mc33_c_library_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_every_library_exports_the_new_names(dtype):
    assert_exported(HIP_NAMES + C_NAMES, dtype)


@pytest.mark.parametrize("dtype", ["f32", "u16", "u8", "u32", "f64"])
def test_render_kernels_are_in_the_code_object(dtype):
    real = "double" if dtype == "f64" else "float"
    assert_kernels(dtype, KERNELS + ["k_render_vertices<%s>" % real, "k_mesh_tile_sum<MeshCount>", "k_mesh_place<MeshCount, 2>"])
    assert_kernels(dtype, WIDE_KERNELS, max_vgprs=80)


@pytest.mark.parametrize("dtype", ["f32", "u16"])
def test_host_logic_library_refuses_to_render(dtype):
    """mc33_capi.c linked with the emulated device layer, which cannot render: the library still loads (a weak reference),
    MC33_render_isosurface returns -1 and leaves the object and `out` alone - for good arguments and for refused ones -, and the
    object extracts as before."""
    with host_logic(dtype) as h:
        lib, M, iso = h.lib, h.M, h.iso
        L = lib.lib
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        before = (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V)
        L.free_surface_memory(S)
        good = fit(L, M, (1, 2, -1), (0, 0, 1), 30.0, 48, 32)[1]
        views = (View * 2)(good, good)
        out = (Image * 2)()
        for o in out:
            o.width, o.nT, o.covered = 77, 5, 9
        calls = [(views, 2, 7, out), (views, 1, 1, out), (views, 0, 7, out), (views, 2, 0, out), (views, 2, 8, out), (None, 2, 7, out), (views, 2, 7, None)]
        for change in ({"width": 0}, {"height": 4097}, {"cull": 3}, {"ambient": float("nan")}, {"light": (0.0, 0.0, 0.0)}):
            bad = (View * 2)(good, good)
            for k, x in change.items():
                setattr(bad[1], k, D3(*x) if k == "light" else x)
            calls.append((bad, 2, 7, out))
        bad = (View * 2)(good, good)
        bad[0].m[5] = float("inf")
        calls.append((bad, 2, 7, out))
        for views_, n, want, out_ in calls:
            assert L.MC33_render_isosurface(M, lib.real(iso + 1), views_, n, want, out_) == -1
            assert (M.contents.iso, M.contents.nV, M.contents.nT, M.contents.memoryfault, M.contents.T, M.contents.V) == before
            assert all((o.width, o.nT, o.covered) == (77, 5, 9) and not o.rgba and not o.depth and not o.triangle for o in out)
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)


def test_ppm_round_trip(tmp_path):
    """a made-up image through MC33_write_image_ppm: the header, then R, G, B of every word, the top row first; alpha is not written"""
    from mc33_capi import MC33Lib, product_path
    if True:
        L = MC33Lib(product_path("f32"), "f32").lib  # (mc33_surface_io.c is host C: the product library serves it without a device)
        width, height = 7, 5
        words = np.random.default_rng(3).integers(0, 1 << 32, width * height, dtype=np.uint64).astype(np.uint32)
        img = Image()
        img.width, img.height = width, height
        img.rgba = words.ctypes.data_as(C.POINTER(C.c_uint))
        path = str(tmp_path / "picture.ppm")
        assert L.MC33_write_image_ppm(C.byref(img), path.encode()) == 0
        raw = open(path, "rb").read()
        head = b"P6\n%d %d\n255\n" % (width, height)
        assert raw.startswith(head) and len(raw) == len(head) + 3 * width * height
        body = np.frombuffer(raw[len(head):], np.uint8).reshape(height * width, 3)
        assert np.array_equal(body, np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], axis=1).astype(np.uint8))
        assert L.MC33_write_image_ppm(C.byref(img), str(tmp_path / "no" / "such" / "dir.ppm").encode()) == -1
        img.rgba = None
        assert L.MC33_write_image_ppm(C.byref(img), path.encode()) == -1 and L.MC33_write_image_ppm(None, path.encode()) == -1
        empty = Image()
        L.MC33_free_image(C.byref(empty))
        L.MC33_free_image(None)
