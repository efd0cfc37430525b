#!/usr/bin/env python3
"""Developer timing of the vertex clustering (results in profiles/simplify_timing.txt).

On the bench surface - the 1024^3 float cos field at iso 0, extracted on the device - hipEvent time of
mc33hip_simplify_surface into exact-size outputs, with the map and no attribute, after a warm-up, median (and best) of 7 calls, at
cells of 2, 4 and 8 grid cells, in both modes, with and without duplicate removal, with the normals of the output and without.
Next to each: the bytes of the simplified surface (V, N, T) beside those of the full one, and the time either takes over the link
at the device-to-host rate this process measures with a pinned buffer.  As a yardstick that is not the code under test, the same
clustering in torch - keys, torch.unique(return_inverse), index_add_ of the positions in float64 and a count - timed the same
way (3 calls), and mc33hip_probe_read's ceiling from the same process.  The call waits for its counts (twice with normals), so its
event time holds those host round trips.

usage: tools/time_simplify.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402
from mc33_c_library_amd.api import ECAPACITY, SIMPLIFY_MODES, Simplification  # noqa: E402

REPS = 7
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")


def timed(call, reps=REPS, warm=1):
    ev = []
    for _ in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    ev = sorted(ev[warm:])
    return ev[0], ev[len(ev) // 2]


grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
g = DeviceGrid(grid, r0=r0, d=d)
V, N, T, cnt = g.extract(0.0)
nV, nT = cnt.nV, cnt.nT
full_bytes = nV * (3 * V.element_size() + 12) + nT * 12
print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles, %.1f MB of V, N, T" % (n, nV, nT, full_bytes / 1e6), flush=True)
best, med, nbytes = g.probe_read()
print("mc33hip_probe_read: %.1f MB in %.4f ms (median %.4f): %.0f GB/s" % (nbytes / 1e6, best, med, nbytes / best / 1e6), flush=True)
host = torch.empty((64 << 20,), dtype=torch.int32, pin_memory=True)
src = torch.empty((64 << 20,), dtype=torch.int32, device=dev)
lbest, lmed = timed(lambda: host.copy_(src, non_blocking=True))
link = host.numel() * 4 / lmed / 1e6  # GB/s
print("device to pinned host, %.0f MB: median %.3f ms (best %.3f): %.1f GB/s; the full surface takes %.3f ms at that rate" % (host.numel() * 4 / 1e6, lmed, lbest, link, full_bytes / link / 1e6),
      flush=True)
del host, src

for cells in (2.0, 4.0, 8.0):
    cell = tuple(cells * x for x in d)
    for mode in ("mean", "first"):
        for drop in (True, False):
            a = Simplification()
            a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), nV, nT
            a.origin, a.cell = (C.c_double * 3)(*r0), (C.c_double * 3)(*cell)
            a.mode, a.drop_duplicates = SIMPLIFY_MODES[mode], int(drop)
            rc = g.lib.mc33hip_simplify_surface(g.ctx, C.byref(a))  # the size query
            assert rc in (0, ECAPACITY), g.lib.mc33hip_last_error().decode(errors="replace")
            nV2, nT2 = int(a.nV_out), int(a.nT_out)
            oV = torch.empty((max(nV2, 1), 3), dtype=V.dtype, device=dev)
            oN = torch.empty((max(nV2, 1), 3), dtype=torch.float32, device=dev)
            oT = torch.empty((max(nT2, 1), 3), dtype=torch.int32, device=dev)
            oMap = torch.empty((nV,), dtype=torch.int32, device=dev)
            a.oV, a.oT, a.oMap, a.capV, a.capT = oV.data_ptr(), oT.data_ptr(), oMap.data_ptr(), nV2, nT2

            def call():
                assert g.lib.mc33hip_simplify_surface(g.ctx, C.byref(a)) == 0
            a.oN = None
            pbest, pmed = timed(call)
            a.oN = oN.data_ptr()
            best, med = timed(call)
            out_bytes = nV2 * (3 * V.element_size() + 12) + nT2 * 12
            print("cell %g, %-5s, duplicates %-7s %9d vertices, %9d triangles (%5.2f %% of them), %d clusters, largest %d, %d collapsed, %d duplicates | "
                  "call: median %.3f ms (best %.3f), without the normals %.3f (%.3f) | %.2f MB: %.3f ms over the link, %.3f ms saved"
                  % (cells, mode, "dropped" if drop else "kept", nV2, nT2, 100.0 * nT2 / nT, int(a.clusters), int(a.max_cluster), int(a.collapsed_triangles),
                     int(a.duplicate_triangles), med, best, pmed, pbest, out_bytes / 1e6, out_bytes / link / 1e6, (full_bytes - out_bytes) / link / 1e6), flush=True)
            del oV, oN, oT, oMap
    # the yardstick: the same clusters and their means in torch
    origin = torch.tensor(r0, dtype=torch.float64, device=dev)
    width = torch.tensor(cell, dtype=torch.float64, device=dev)

    def yardstick():
        P = V.double()
        k = torch.floor((P - origin) / width).clamp_(0, 2097151).long()
        key = k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)
        uniq, inv = torch.unique(key, return_inverse=True)
        sums = torch.zeros((uniq.numel(), 3), dtype=torch.float64, device=dev).index_add_(0, inv, P)
        return sums / torch.bincount(inv, minlength=uniq.numel()).unsqueeze(1)
    ybest, ymed = timed(yardstick, reps=3)
    print("cell %g, torch (keys, unique, index_add_; the vertices alone, no triangles): median %.3f ms (best %.3f)" % (cells, ymed, ybest), flush=True)
    torch.cuda.empty_cache()
