#!/usr/bin/env python3
"""Developer timing of the clipping by planes (results in profiles/clip_timing.txt).

On the bench surface - the 1024^3 float cos field at iso 0, extracted on the device - hipEvent time of mc33hip_clip_surface into
outputs allocated beforehand, with the map and no attribute, after a warm-up, median (and best) of 7 calls, with the normals and
without, for three cuts: the plane x >= 0, which halves the surface; the box [-2, 2]^3, which keeps about an eighth, as six calls
from one set of arrays into the other; and a plane that misses.  Held against two yardsticks that are not the code under test:
the time the rows that are no longer downloaded would take over the link, at the device-to-host rate this process measures with a
pinned buffer; and the easy half of the work alone in torch - s per vertex and the triangles without a corner outside,
index_select'ed - timed the same way (3 calls).  The call waits once for its counts, so its event time holds that host round trip.

usage: tools/time_clip.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, clip_box, fields  # noqa: E402
from mc33_c_library_amd.api import CLIP_COUNTS, Clipping  # noqa: E402

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
row = 3 * V.element_size() + 12


def surface_bytes(v, t, normals=True):
    return v * (row if normals else 3 * V.element_size()) + t * 12


print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles, %.1f MB of V, N, T" % (n, nV, nT, surface_bytes(nV, nT) / 1e6), flush=True)
best, med, nbytes = g.probe_read()
print("mc33hip_probe_read: %.1f MB in %.4f ms (median %.4f): %.0f GB/s" % (nbytes / 1e6, best, med, nbytes / best / 1e6), flush=True)
host = torch.empty((64 << 20,), dtype=torch.int32, pin_memory=True)
src = torch.empty((64 << 20,), dtype=torch.int32, device=dev)
lbest, lmed = timed(lambda: host.copy_(src, non_blocking=True))
link = host.numel() * 4 / lmed / 1e6  # GB/s
print("device to pinned host, %.0f MB: median %.3f ms (best %.3f): %.1f GB/s; the full surface takes %.3f ms at that rate"
      % (host.numel() * 4 / 1e6, lmed, lbest, link, surface_bytes(nV, nT) / link / 1e6), flush=True)
del host, src

# two sets of outputs, each large enough for any of the cuts below (a cut adds few vertices to what it keeps)
capV, capT = nV + nV // 8, nT + nT // 8
sets = [dict(V=torch.empty((capV, 3), dtype=V.dtype, device=dev), N=torch.empty((capV, 3), dtype=torch.float32, device=dev),
             T=torch.empty((capT, 3), dtype=torch.int32, device=dev)) for _ in range(2)]
oMap = torch.empty((capV,), dtype=torch.int32, device=dev)


def clip_once(src, nv, nt, plane, dst, normals):
    a = Clipping()
    a.V, a.N, a.T, a.nV, a.nT = src["V"].data_ptr(), (src["N"].data_ptr() if normals else None), src["T"].data_ptr(), nv, nt
    a.plane = (C.c_double * 4)(*plane)
    a.oV, a.oN, a.oT, a.oMap, a.capV, a.capT = dst["V"].data_ptr(), (dst["N"].data_ptr() if normals else None), dst["T"].data_ptr(), oMap.data_ptr(), capV, capT
    rc = g.lib.mc33hip_clip_surface(g.ctx, C.byref(a))
    assert rc == 0, g.lib.mc33hip_last_error().decode(errors="replace")
    return a


def chain(planes, normals):
    src, nv, nt, last = dict(V=V, N=N, T=T), nV, nT, None
    for k, plane in enumerate(planes):
        last = clip_once(src, nv, nt, plane, sets[k & 1], normals)
        src, nv, nt = sets[k & 1], int(last.nV_out), int(last.nT_out)
        if not nt:
            break
    return last


def torch_easy_half(plane):
    a, b, c, w = plane
    P = V.double()
    s = ((P[:, 0] * a + P[:, 1] * b) + P[:, 2] * c) + w
    inside = s >= 0
    keep = inside[T.long()].all(dim=1)
    return T.index_select(0, keep.nonzero().squeeze(1))


cuts = [("the plane x >= 0 (halves the surface)", [(1.0, 0.0, 0.0, 0.0)]),
        ("the box [-2, 2]^3 (six planes, about an eighth)", clip_box((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))),
        ("a plane that misses (x >= -100)", [(1.0, 0.0, 0.0, 100.0)])]
for name, planes in cuts:
    last = chain(planes, True)
    nV2, nT2 = int(last.nV_out), int(last.nT_out)
    counts = ", ".join("%s %d" % (k, int(getattr(last, k))) for k in CLIP_COUNTS[2:])
    best, med = timed(lambda: chain(planes, True))
    pbest, pmed = timed(lambda: chain(planes, False))
    saved = surface_bytes(nV, nT) - surface_bytes(nV2, nT2)
    print("%s: %d vertices, %d triangles left (%.2f %% of them); the last call: %s" % (name, nV2, nT2, 100.0 * nT2 / nT, counts), flush=True)
    print("    %d call%s: median %.3f ms (best %.3f), without the normals %.3f (%.3f) | %.1f MB no longer downloaded: %.3f ms over the link -> %s"
          % (len(planes), "" if len(planes) == 1 else "s", med, best, pmed, pbest, saved / 1e6, saved / link / 1e6,
             "the cut costs LESS than the download it saves" if med < saved / link / 1e6 else "the cut costs MORE than the download it saves"), flush=True)
    ybest, ymed = timed(lambda: torch_easy_half(planes[0]), reps=3)
    print("    torch, the easy half of the first plane alone (s per vertex, triangles without a corner outside, index_select): median %.3f ms (best %.3f)"
          % (ymed, ybest), flush=True)
    torch.cuda.empty_cache()
