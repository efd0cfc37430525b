#!/usr/bin/env python3
"""Developer timing of the pictures made on the device (results in profiles/render_timing.txt).

On the bench surface - the 1024^3 float cos field at iso 0, extracted on the device - mc33hip_render_surface with all three images,
at 1024 x 1024 and 4096 x 4096, for an orthographic view of the whole box and a perspective close-up from inside it (most triangles
behind the eye or outside the picture, the ones in it many pixels large): the hipEvent time of the whole call (10 calls after a
warm-up, median and range; the call waits once for its counts, so its time holds that host round trip) and, from the library's own
events around its kernels (MC33_HIP_TIMING=2), the median per stage.  Then, through the C API in the same process:
MC33_render_isosurface (one view, colour image only; wall time, extraction and the download of the 4 MB or 64 MB image included)
beside the steady calculate_isosurface of the same build - the download the picture replaces.

usage: tools/time_render.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys
import time

os.environ["MC33_HIP_TIMING"] = "2"  # (read when a context is created)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, Image, Rendering, View, fields  # noqa: E402
from mc33_c_library_amd.api import RENDER_COUNTS  # noqa: E402

REPS = 10
STAGES = ("clear", "vertices", "triangles", "scan", "tiles", "resolve")
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")


def frame(direction, up):
    f = np.asarray(direction, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    return r, np.cross(r, f), f


def orthographic(centre, direction, up, half, near, far):
    r, u, f = frame(direction, up)
    rows, off = [r / half, u / half, f / (far - near), np.zeros(3)], [0.0, 0.0, -near / (far - near), 1.0]
    return [x for k in range(4) for x in list(rows[k]) + [off[k] - float(rows[k] @ np.asarray(centre))]]


def perspective(eye, direction, up, fov, near, far):
    r, u, f = frame(direction, up)
    th, a, b = np.tan(np.radians(fov) / 2.0), far / (far - near), -far * near / (far - near)
    rows, off = [r / th, u / th, a * f, f], [0.0, 0.0, b, 0.0]
    return [x for k in range(4) for x in list(rows[k]) + [off[k] - float(rows[k] @ np.asarray(eye))]]


VIEWS = {"orthographic, the whole box": orthographic((0.0, 0.0, 0.0), (-1.0, -0.7, -0.5), (0.0, 0.0, 1.0), 6.5, -7.0, 7.0),
         "perspective close-up from (0.3, 0.2, 0.1)": perspective((0.3, 0.2, 0.1), (1.0, 0.6, 0.3), (0.0, 0.0, 1.0), 50.0, 0.02, 8.0)}

grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
g = DeviceGrid(grid, r0=r0, d=d)
V, N, T, cnt = g.extract(0.0)
nV, nT = cnt.nV, cnt.nT
print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles, %.1f MB of V, N, T" % (n, nV, nT, (nV * 24 + nT * 12) / 1e6), flush=True)

for size in (1024, 4096):
    out = [torch.empty((size, size), dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32)]
    for name, m in VIEWS.items():
        a = Rendering()
        a.V, a.N, a.T, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), nV, nT
        a.m, a.light = (C.c_double * 16)(*m), (C.c_double * 3)(0.4, 0.5, 0.7)
        a.width, a.height, a.cull, a.two_sided, a.ambient, a.diffuse = size, size, 0, 1, 0.2, 0.8
        a.background, a.base_color = 0xFF000000, 0xFF5C5C5C
        a.oRGBA, a.oDepth, a.oTri = (x.data_ptr() for x in out)
        whole, stages = [], []
        for rep in range(REPS + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = g.lib.mc33hip_render_surface(g.ctx, C.byref(a))
            e1.record()
            e1.synchronize()
            assert rc == 0, g.lib.mc33hip_last_error().decode(errors="replace")
            ms = (C.c_float * 6)()
            assert g.lib.mc33hip_render_timing(g.ctx, C.byref(ms)) == 0
            if rep >= 2:
                whole.append(e0.elapsed_time(e1))
                stages.append(list(ms))
        whole.sort()
        med = np.median(np.array(stages), axis=0)
        print("%d x %d, %s: %s" % (size, size, name, ", ".join("%s %d" % (k, int(getattr(a, k))) for k in RENDER_COUNTS)), flush=True)
        print("    mc33hip_render_surface, %d calls: median %.3f ms, range %.3f .. %.3f | per stage (median): %s" %
              (REPS, whole[len(whole) // 2], whole[0], whole[-1], ", ".join("%s %.3f" % (s, x) for s, x in zip(STAGES, med))), flush=True)
    del out

# ---- the C API: the picture beside the download it replaces ----------------------------------------------------------------------
g.close()
del V, N, T, grid
torch.cuda.empty_cache()
from mc33_capi import MC33Lib, product_path  # noqa: E402
import fixtures as fx  # noqa: E402

lib = MC33Lib(product_path("f32"), "f32")
L = lib.lib
L.MC33_render_isosurface.restype = C.c_int
L.MC33_render_isosurface.argtypes = [C.POINTER(lib.MC33), lib.real, C.POINTER(View), C.c_uint, C.c_uint, C.POINTER(Image)]
L.MC33_free_image.argtypes = [C.POINTER(Image)]
L.MC33_view_fit.restype = C.c_int
L.MC33_view_fit.argtypes = [C.POINTER(lib.MC33), C.POINTER(C.c_double * 3), C.POINTER(C.c_double * 3), C.c_double, C.c_uint, C.c_uint, C.POINTER(View)]
data, r0, d = fx.cos_field(n)
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
wall = []
for rep in range(6):
    t0 = time.perf_counter()
    S = L.calculate_isosurface(M, C.c_float(0.0))
    t1 = time.perf_counter()
    s = S.contents
    mb = (s.nV * 28 + s.nT * 12) / 1e6
    L.free_surface_memory(S)
    wall.append((t1 - t0) * 1e3)
print("calculate_isosurface, 6 calls, wall: %s ms (%.0f MB of surface to the host each)" % (", ".join("%.2f" % x for x in wall), mb), flush=True)
for size in (1024, 4096):
    v = View()
    assert L.MC33_view_fit(M, C.byref((C.c_double * 3)(-1.0, -0.7, -0.5)), C.byref((C.c_double * 3)(0, 0, 1)), 0.0, size, size, C.byref(v)) == 0
    wall = []
    for rep in range(6):
        img = Image()
        t0 = time.perf_counter()
        rc = L.MC33_render_isosurface(M, C.c_float(0.0), C.byref(v), 1, 1, C.byref(img))
        t1 = time.perf_counter()
        assert rc == 1
        covered = img.covered
        L.MC33_free_image(C.byref(img))
        wall.append((t1 - t0) * 1e3)
    print("MC33_render_isosurface, MC33_view_fit's orthographic view, %d x %d, colour image only (%.0f MB to the host), 6 calls, wall: %s ms (%d pixels covered)"
          % (size, size, size * size * 4 / 1e6, ", ".join("%.2f" % x for x in wall), covered), flush=True)
L.free_MC33(M)
