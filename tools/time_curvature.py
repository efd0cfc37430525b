#!/usr/bin/env python3
"""Developer timing of the curvature pass (results in profiles/curvature_timing.txt): the bench's 1024^3 float field,
the surface of isovalue 0 as extract() returns it.

  mc33hip_curvature_vertices : hipEvent best and median of the call (its summary's copy and wait included); how many live axes
               (f != 0) the vertices have - a vertex with L of them walks 2^L nodes; the algorithmic bytes - 12 nV read, 16 nV
               written, 19 samples per node - and their rate against mc33hip_probe_read in this process
  yardsticks : mc33hip_sample_property over the same V (the grid attached to itself as the property grid), and the same
               arithmetic in torch (float64, central differences of the whole grid, then 8 gathers per quantity)

usage: tools/time_curvature.py [points per axis, default 1024] [--no-torch]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402
from mc33_c_library_amd.api import Curvature  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")
grid, r0, d = fields.cos_field_cube(n, dev)
g = DeviceGrid(grid, r0=r0, d=d)
V, N, T, cnt = g.extract(0.0)
nV = cnt.nV
print("grid %d^3 float, iso 0: %d vertices, %d triangles" % (n, nV, cnt.nT), flush=True)

# live axes per vertex (steps 1 - 2 of the definition, in torch double on the device)
vd = V.to(torch.float64)
live = torch.zeros(nV, dtype=torch.int64, device=dev)
for a in range(3):
    ga = (vd[:, a] - r0[a]) / d[a]
    ia = torch.clamp(torch.floor(ga), 0, n - 1)
    fa = torch.clamp(ga - ia, 0.0, 1.0)
    fa = torch.where(ia == n - 1, torch.zeros_like(fa), fa)
    live += (fa != 0).to(torch.int64)
hist = torch.bincount(live, minlength=4).tolist()
nodes = sum(hist[k] << k for k in range(4))
del vd, live
print("live axes per vertex 0 / 1 / 2 / 3: %s -> %d nodes, %.2f per vertex, %d samples gathered" % (hist, nodes, nodes / nV, 19 * nodes), flush=True)

best, med, nbytes = g.probe_read(10)
ceiling = nbytes / best / 1e6
print("mc33hip_probe_read over the grid: best %.3f ms, median %.3f ms -> %.0f GB/s" % (best, med, ceiling), flush=True)


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


out = [torch.empty(nV, dtype=torch.float32, device=dev) for _ in range(4)]
a = Curvature()
a.dV, a.nV, a.sign = V.data_ptr(), nV, 1
a.oMean, a.oGauss, a.oK1, a.oK2 = (t.data_ptr() for t in out)
b, m = timed(lambda: g.lib.mc33hip_curvature_vertices(g.ctx, C.byref(a)))
moved = 28 * nV + 19 * nodes * 4
print("mc33hip_curvature_vertices (four outputs): best %.4f ms, median %.4f ms; V + outputs + 19 samples per node = %.1f MB -> %.0f GB/s = %.1f %% of the read ceiling"
      % (b, m, moved / 1e6, moved / b / 1e6, 100 * moved / b / 1e6 / ceiling), flush=True)
print("summary: mean in [%g, %g], gauss in [%g, %g], finite %d, undefined %d" % (a.lo[0], a.hi[0], a.lo[1], a.hi[1], a.finite, a.undefined), flush=True)
a.oGauss = a.oK1 = a.oK2 = None
b1, m1 = timed(lambda: g.lib.mc33hip_curvature_vertices(g.ctx, C.byref(a)))
print("mc33hip_curvature_vertices (mean alone): best %.4f ms, median %.4f ms" % (b1, m1), flush=True)

g.attach_property(grid)
bp, mp = timed(lambda: g.lib.mc33hip_sample_property(g.ctx, C.c_void_p(V.data_ptr()), nV, C.c_void_p(out[1].data_ptr())))
print("mc33hip_sample_property over the same V: best %.4f ms, median %.4f ms; the curvature pass takes %.1f times that" % (bp, mp, b / bp), flush=True)
g.detach_property()

if "--no-torch" in sys.argv:
    sys.exit(0)


# --- the same arithmetic in torch: differences of the whole grid (interior stencils only: a yardstick, not the definition), then
# trilinear gathers at the vertices
def torch_curvature():
    F = grid.to(torch.float64)
    h = [float(x) for x in d]
    q = []
    for ax, hh in ((2, h[0]), (1, h[1]), (0, h[2])):
        q.append((torch.roll(F, -1, ax) - torch.roll(F, 1, ax)) / (2.0 * hh))
    for ax, hh in ((2, h[0]), (1, h[1]), (0, h[2])):
        q.append(((torch.roll(F, -1, ax) - F) - (F - torch.roll(F, 1, ax))) / (hh * hh))
    for (a0, h0), (a1, h1) in (((2, h[0]), (1, h[1])), ((2, h[0]), (0, h[2])), ((1, h[1]), (0, h[2]))):
        up, dn = torch.roll(F, -1, a0), torch.roll(F, 1, a0)
        q.append(((torch.roll(up, -1, a1) - torch.roll(up, 1, a1)) - (torch.roll(dn, -1, a1) - torch.roll(dn, 1, a1))) / ((2.0 * h0) * (2.0 * h1)))
        del up, dn
    vd = V.to(torch.float64)
    gi = [torch.clamp(torch.floor((vd[:, k] - r0[k]) / d[k]), 0, n - 2) for k in range(3)]
    fr = [torch.clamp((vd[:, k] - r0[k]) / d[k] - gi[k], 0.0, 1.0) for k in range(3)]
    gi = [x.to(torch.int64) for x in gi]
    val = []
    for Q in q:
        flat = Q.reshape(-1)
        acc = 0.0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = (fr[0] if dx else 1 - fr[0]) * (fr[1] if dy else 1 - fr[1]) * (fr[2] if dz else 1 - fr[2])
                    acc = acc + w * flat[((gi[2] + dz) * n + (gi[1] + dy)) * n + (gi[0] + dx)]
        val.append(acc)
    gx, gy, gz, hxx, hyy, hzz, hxy, hxz, hyz = val
    g2 = gx * gx + gy * gy + gz * gz
    gHg = gx * gx * hxx + gy * gy * hyy + gz * gz * hzz + 2.0 * (gx * gy * hxy + gx * gz * hxz + gy * gz * hyz)
    return ((gHg - g2 * (hxx + hyy + hzz)) / (2.0 * g2 * torch.sqrt(g2))).to(torch.float32)


try:
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mean_t = torch_curvature()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    diff = (mean_t - out[0]).abs()
    print("the mean curvature in torch (float64, differences of the whole grid, 8 gathers per quantity): %s ms; differs from the pass by at most %.3g (interior stencils)"
          % (" ".join("%.1f" % x for x in ms), float(diff[torch.isfinite(diff)].max().item())), flush=True)
except RuntimeError as e:  # (nine float64 grids of 1024^3 are 77 GB)
    print("the torch yardstick did not run: %s" % str(e).splitlines()[0], flush=True)
