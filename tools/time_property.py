#!/usr/bin/env python3
"""Developer timing of the property pass (results in profiles/r07_property.txt): the bench's 1024^3 float field
with a second 1024^3 field as property grid.

  device ABI : hipEvent time of mc33hip_color_vertices / mc33hip_sample_property (the palette's copy and the 8-byte copy of the
               violation word included), the bytes the kernel must move - 12 nV read, 4 nV written, the property samples it
               touches (counted here with torch, as samples and as 64-byte pieces) - over that time, as a fraction of the 8 TB/s
               peak and of mc33hip_probe_read's ceiling in this process
  C API      : calculate_isosurface wall with and without a colour map

usage: tools/time_property.py [points per axis, default 1024] [--device-only]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402
from mc33_capi import MC33Lib, product_path  # noqa: E402

PEAK = 8000.0  # GB/s, HBM3E spec peak of the MI355X
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")
grid, r0, d = fields.cos_field_cube(n, dev)
h = d[0]
prop = fields.cos_field_slab(n, n, h * 0.37, -1.0, dev)  # another smooth field on the same points: the "potential"
g = DeviceGrid(grid, r0=r0, d=d)
g.attach_property(prop)
V, N, T, cnt = g.extract(0.0)
nV = cnt.nV
print("grid %d^3 float, property %d^3 float, iso 0: %d vertices, %d triangles" % (n, n, nV, cnt.nT), flush=True)

# the property samples the kernel touches (the definition, in torch double on the device)
touched = torch.zeros(n * n * n, dtype=torch.bool, device=dev)
vd = V.to(torch.float64)
idx, frac = [], []
for a in range(3):
    ga = (vd[:, a] - r0[a]) / d[a]
    ia = torch.clamp(torch.floor(ga), 0, n - 1)
    fa = torch.clamp(ga - ia, 0.0, 1.0)
    ia = ia.to(torch.int64)
    fa = torch.where(ia == n - 1, torch.zeros_like(fa), fa)
    idx.append(ia); frac.append(fa != 0)
for dz in (0, 1):
    for dy in (0, 1):
        for dx in (0, 1):
            lin = ((idx[2] + dz * frac[2]) * n + (idx[1] + dy * frac[1])) * n + (idx[0] + dx * frac[0])
            touched[lin] = True
samples = int(touched.sum().item())
pieces = int(touched.view(-1, 16).any(dim=1).sum().item())
del touched, vd, idx, frac
stream_bytes = 16 * nV
print("property samples touched: %d (%.1f MB; %.2f per vertex), in %d 64-byte pieces (%.1f MB)"
      % (samples, samples * 4 / 1e6, samples / nV, pieces, pieces * 64 / 1e6), flush=True)

best, med, nbytes = g.probe_read(10)
ceiling = nbytes / best / 1e6
print("mc33hip_probe_read over the grid: best %.3f ms, median %.3f ms -> %.0f GB/s (%.1f %% of peak)" % (best, med, ceiling, 100 * ceiling / PEAK), flush=True)

pal = (C.c_int * 256)(*[((k * 2654435761) & 0x7fffffff) for k in range(256)])
outc = torch.empty(nV, dtype=torch.int32, device=dev)
outf = torch.empty(nV, dtype=torch.float32, device=dev)
lo, hi = float(prop.min().item()) * 0.5, float(prop.max().item()) * 0.5


def timed(call, reps=12):
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call()
        e1.record()
        assert rc == 0, rc
        assert g.lib.mc33hip_synchronize(g.ctx) == 0
        ms.append(e0.elapsed_time(e1))
    ms = sorted(ms[2:])
    return ms[0], ms[len(ms) // 2]


for name, call in (("mc33hip_color_vertices (256 colours)", lambda: g.lib.mc33hip_color_vertices(g.ctx, C.c_void_p(V.data_ptr()), nV, pal, 256, C.c_double(lo), C.c_double(hi), 0, C.c_void_p(outc.data_ptr()))),
                   ("mc33hip_sample_property", lambda: g.lib.mc33hip_sample_property(g.ctx, C.c_void_p(V.data_ptr()), nV, C.c_void_p(outf.data_ptr())))):
    b, m = timed(call)
    for label, moved in (("V + output + samples", stream_bytes + samples * 4), ("V + output + 64-byte pieces", stream_bytes + pieces * 64)):
        gbs = moved / b / 1e6
        print("%s: best %.4f ms, median %.4f ms; %s = %.1f MB -> %.0f GB/s = %.1f %% of peak, %.1f %% of the read ceiling"
              % (name, b, m, label, moved / 1e6, gbs, 100 * gbs / PEAK, 100 * gbs / ceiling), flush=True)

if "--device-only" in sys.argv:
    sys.exit(0)
# --- the C API: calculate_isosurface with and without a colour map ---------------------------------------------------------
data, pdata = grid.cpu().numpy(), prop.cpu().numpy()
del g, grid, prop, V, N, T, outc, outf
torch.cuda.empty_cache()
lib = MC33Lib(product_path("f32"), "f32")
L = lib.lib
L.MC33_set_property_grid.restype = C.c_int
L.MC33_set_property_grid.argtypes = [C.POINTER(lib.MC33), C.POINTER(lib.GRD)]
L.MC33_set_color_map.restype = C.c_int
L.MC33_set_color_map.argtypes = [C.POINTER(lib.MC33), C.POINTER(C.c_int), C.c_uint, C.c_double, C.c_double]
G, keep = lib.make_grid(data, r0, d)
Pg, keep2 = lib.make_grid(pdata, r0, d)
M = L.create_MC33(G)
assert M


def walls(label, reps=8):
    w = []
    for _ in range(reps):
        t0 = time.perf_counter()
        S = L.calculate_isosurface(M, C.c_float(0.0))
        t1 = time.perf_counter()
        assert S
        first, last = S.contents.nV and C.cast(S.contents.color, C.POINTER(C.c_uint))[0], S.contents.nV and C.cast(S.contents.color, C.POINTER(C.c_uint))[S.contents.nV - 1]
        L.free_surface_memory(S)
        w.append((t1 - t0) * 1e3)
    print("calculate_isosurface %s: walls %s ms; best %.2f, median %.2f (colour of the first / last vertex %08x / %08x)"
          % (label, " ".join("%.2f" % x for x in w), min(w[2:]), sorted(w[2:])[len(w[2:]) // 2], first, last), flush=True)


walls("without a property grid")
t0 = time.perf_counter()
assert L.MC33_set_property_grid(M, Pg) == 0
print("MC33_set_property_grid (upload %.2f GB): %.1f ms" % (pdata.nbytes / 1e9, (time.perf_counter() - t0) * 1e3), flush=True)
walls("with a property grid, no colour map")
assert L.MC33_set_color_map(M, pal, 256, lo, hi) == 0
walls("with property grid and colour map")
assert L.MC33_set_color_map(M, None, 0, 0.0, 0.0) == 0
walls("colour map removed again")
L.free_MC33(M)
