#!/usr/bin/env python3
"""Developer timing of the caps at the grid faces (results in profiles/cap_timing.txt).

A float grid of n^3 points (default 1024) holds R^2 - |x - c|^2 with the centre off the lattice and R large enough to cut all six
faces; the surface of iso 0 is extracted on the device.  hipEvent time of mc33hip_cap_surface alone, in place in arrays allocated
beforehand whose first rows are restored - outside the timed window - before every call, on a warm context: 20 repetitions,
median and range.  Beside it, in the same process and on the same mesh: mc33hip_surface_topology of the uncapped surface, which
builds the whole-mesh edge table the cap builds too, and the extraction itself.  Every timed call waits once for its counts, so
its event time holds that host round trip.

usage: tools/time_cap.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid  # noqa: E402
from mc33_c_library_amd.api import CAP_COUNTS, Capping  # noqa: E402

REPS = 20
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")


def timed(call, before=None, reps=REPS, warm=2):
    ev = []
    for _ in range(reps + warm):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    ev = sorted(ev[warm:])
    return ev[len(ev) // 2], ev[0], ev[-1]


def ball(n):
    """R^2 - |x - c|^2, plane by plane (bounded temporaries)"""
    c = [0.5 * (n - 1) + 0.3, 0.5 * (n - 1) - 0.2, 0.5 * (n - 1) + 0.4]
    R = 0.56 * (n - 1)  # beyond every face centre (0.5), short of the edges of the box (0.707)
    ax = torch.arange(n, dtype=torch.float64, device=dev)
    xy = (ax[None, :] - c[0]) ** 2 + (ax[:, None] - c[1]) ** 2
    out = torch.empty((n, n, n), dtype=torch.float32, device=dev)
    for k in range(0, n, 64):
        z = (ax[k:k + 64] - c[2]) ** 2
        out[k:k + 64] = (R * R - (xy[None, :, :] + z[:, None, None])).to(torch.float32)
    return out


grid = ball(n)
g = DeviceGrid(grid)
V, N, T, cnt = g.extract(0.0)
nV, nT = cnt.nV, cnt.nT
print("%d^3 float, a ball that cuts all six faces, iso 0: %d vertices, %d triangles" % (n, nV, nT), flush=True)

a = Capping()
a.V, a.N, a.T, a.nV, a.nT, a.iso = V.data_ptr(), N.data_ptr(), T.data_ptr(), nV, nT, 0.0
a.lo, a.hi = (C.c_uint * 3)(0, 0, 0), (C.c_uint * 3)(n - 1, n - 1, n - 1)
rc = g.lib.mc33hip_cap_surface(g.ctx, C.byref(a))  # the size query
assert rc == -4, g.lib.mc33hip_last_error().decode(errors="replace")
nV2, nT2 = int(a.nV_out), int(a.nT_out)
V2 = torch.empty((nV2, 3), dtype=V.dtype, device=dev)
N2 = torch.empty((nV2, 3), dtype=torch.float32, device=dev)
T2 = torch.empty((nT2, 3), dtype=torch.int32, device=dev)
a.V, a.N, a.T, a.capV, a.capT = V2.data_ptr(), N2.data_ptr(), T2.data_ptr(), nV2, nT2


def restore():
    V2[:nV].copy_(V)
    N2[:nV].copy_(N)
    T2[:nT].copy_(T)


def cap():
    assert g.lib.mc33hip_cap_surface(g.ctx, C.byref(a)) == 0, g.lib.mc33hip_last_error().decode(errors="replace")


restore()
cap()
print("capped: " + ", ".join("%s %d" % (k, int(getattr(a, k))) for k in CAP_COUNTS), flush=True)
t = g.topology(T2, nV2)
print("topology of the result: closed %d, manifold %d, oriented %d, boundary edges %d" % (t.closed, t.manifold, t.oriented, t.boundary_edges), flush=True)
med, lo, hi = timed(cap, restore)
print("mc33hip_cap_surface, %d calls: median %.3f ms, range %.3f .. %.3f" % (REPS, med, lo, hi), flush=True)
med, lo, hi = timed(lambda: g.topology(T, nV))
print("mc33hip_surface_topology of the uncapped surface, %d calls: median %.3f ms, range %.3f .. %.3f" % (REPS, med, lo, hi), flush=True)
med, lo, hi = timed(lambda: g.extract_into(0.0, V, N, T))
print("mc33hip_extract of the same surface into the same arrays, %d calls: median %.3f ms, range %.3f .. %.3f" % (REPS, med, lo, hi), flush=True)
