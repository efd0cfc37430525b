#!/usr/bin/env python3
"""Developer timing of the distance between surfaces (results in profiles/distance_timing.txt).

On the bench surface - the 1024^3 float cos field at iso 0, extracted on the device - hipEvent time of mc33hip_surface_distance
with all three outputs, after a warm-up, median (and range) of 20 calls: the surface's vertices against itself, the vertices of the
2x2x2-simplified surface against the full surface, and the full surface's vertices against the simplified one.  Next to each the
library's own events around its three passes (MC33_HIP_TIMING=2, mc33hip_distance_timing: build - box, count, scan, fill -, query,
reduce), the lattice it cut and the point-triangle evaluations per point.  The call waits for the box, for the size of the lists
and for the summary, so its event time holds those host round trips.  For scale, mc33hip_probe_read's ceiling from the same
process.

usage: tools/time_distance.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, Distance, fields  # noqa: E402

REPS = 20
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")

grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
g = DeviceGrid(grid, r0=r0, d=d)
V, N, T, cnt = g.extract(0.0)
print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles, %.1f MB of V, N, T" % (n, cnt.nV, cnt.nT, (cnt.nV * 24 + cnt.nT * 12) / 1e6), flush=True)
best, med, nbytes = g.probe_read()
print("mc33hip_probe_read: %.1f MB in %.4f ms (median %.4f): %.0f GB/s" % (nbytes / 1e6, best, med, nbytes / best / 1e6), flush=True)
V2, N2, T2, _, _, info = g.simplify(V, T, tuple(2.0 * x for x in d))
print("simplified on cells of 2x2x2: %d vertices, %d triangles" % (info["nV_out"], info["nT_out"]), flush=True)
g.set_timing(2)


def timed(name, P, tV, tT):
    nP = P.shape[0]
    a = Distance()
    oDist = torch.empty((nP,), dtype=torch.float32, device=dev)
    oTri = torch.empty((nP,), dtype=torch.int32, device=dev)
    oPoint = torch.empty((nP, 3), dtype=P.dtype, device=dev)
    a.P, a.nP, a.V, a.T, a.nV, a.nT = P.data_ptr(), nP, tV.data_ptr(), tT.data_ptr(), tV.shape[0], tT.shape[0]
    a.oDist, a.oTri, a.oPoint = oDist.data_ptr(), oTri.data_ptr(), oPoint.data_ptr()
    whole, passes = [], []
    for k in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = g.lib.mc33hip_surface_distance(g.ctx, C.byref(a))
        e1.record()
        e1.synchronize()
        assert rc == 0, g.lib.mc33hip_last_error().decode(errors="replace")
        if k:  # (the first call makes the scratch)
            whole.append(e0.elapsed_time(e1))
            passes.append(g.distance_timing())
    whole.sort()
    mid = [sorted(p[j] for p in passes)[REPS // 2] for j in range(3)]
    print("%-28s %9d points, %9d triangles | call: median %.3f ms (%.3f .. %.3f) | build %.3f, query %.3f, reduce %.3f | lattice %s, %.1f tests a point | "
          "max %.6g (point %d), mean %.6g, rms %.6g"
          % (name, nP, tT.shape[0], whole[REPS // 2], whole[0], whole[-1], mid[0], mid[1], mid[2], "x".join(str(x) for x in a.lattice), a.triangle_tests / max(nP, 1),
             a.max, a.argmax, a.sum / max(a.matched_points, 1), (a.sum_sq / max(a.matched_points, 1)) ** 0.5), flush=True)


timed("the surface against itself", V, V, T)
timed("simplified against full", V2, V, T)
timed("full against simplified", V, V2, T2)
