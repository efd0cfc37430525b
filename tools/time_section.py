#!/usr/bin/env python3
"""Developer timing of the sections by planes (results in profiles/section_timing.txt).

On the bench surface - the 1024^3 float cos field at iso 0, extracted on the device - hipEvent time of mc33hip_section_surface
into outputs allocated beforehand, with the optional outputs and no attribute, after a warm-up, median (and best) of 7 calls, for
the plane x >= 0 and for a plane that misses; of mc33hip_section_ladder with 64 offsets along z; and of 64 single calls on the
same 64 planes.  Held against two yardsticks that are not the code under test, taken in the same process: mc33hip_clip_surface on
the same plane, without normals, timed the same way; and the time the whole surface, which a section on the host would need,
takes over the link at the device-to-host rate this process measures with a pinned buffer.  Every call waits once for its counts,
so its event time holds that host round trip.  The lines EXPECTATION say whether a section costs no more than the clip of the same
plane, and whether the ladder costs less than its single calls.

usage: tools/time_section.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402
from mc33_c_library_amd.api import SECTION_COUNTS, Clipping, Sectioning  # noqa: E402

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
whole = nV * 3 * V.element_size() + nT * 12
print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles, %.1f MB of V and T" % (n, nV, nT, whole / 1e6), flush=True)
host = torch.empty((64 << 20,), dtype=torch.int32, pin_memory=True)
src = torch.empty((64 << 20,), dtype=torch.int32, device=dev)
lbest, lmed = timed(lambda: host.copy_(src, non_blocking=True))
link = host.numel() * 4 / lmed / 1e6  # GB/s
print("device to pinned host, %.0f MB: median %.3f ms (best %.3f): %.1f GB/s; V and T take %.3f ms at that rate"
      % (host.numel() * 4 / 1e6, lmed, lbest, link, whole / link / 1e6), flush=True)
del host, src

capP, capS = 1 << 20, 1 << 20  # far more than any plane below needs
oP = torch.empty((capP, 3), dtype=V.dtype, device=dev)
oS = torch.empty((capS, 2), dtype=torch.int32, device=dev)
oLabel, oNext = (torch.empty((capP,), dtype=torch.int32, device=dev) for _ in range(2))
oMap = torch.empty((nV,), dtype=torch.int32, device=dev)
capV, capT = nV + nV // 8, nT + nT // 8
cV = torch.empty((capV, 3), dtype=V.dtype, device=dev)
cT = torch.empty((capT, 3), dtype=torch.int32, device=dev)
cMap = torch.empty((nV,), dtype=torch.int32, device=dev)


def section_once(plane):
    a = Sectioning()
    a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), nV, nT
    a.plane = (C.c_double * 4)(*plane)
    a.oP, a.oS, a.oLabel, a.oNext, a.oPointMap, a.capP, a.capS = oP.data_ptr(), oS.data_ptr(), oLabel.data_ptr(), oNext.data_ptr(), oMap.data_ptr(), capP, capS
    rc = g.lib.mc33hip_section_surface(g.ctx, C.byref(a))
    assert rc == 0, g.lib.mc33hip_last_error().decode(errors="replace")
    return a


def clip_once(plane):
    a = Clipping()
    a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), nV, nT
    a.plane = (C.c_double * 4)(*plane)
    a.oV, a.oT, a.oMap, a.capV, a.capT = cV.data_ptr(), cT.data_ptr(), cMap.data_ptr(), capV, capT
    rc = g.lib.mc33hip_clip_surface(g.ctx, C.byref(a))
    assert rc == 0, g.lib.mc33hip_last_error().decode(errors="replace")
    return a


for name, plane in (("the plane x >= 0", (1.0, 0.0, 0.0, 0.0)), ("a plane that misses (x >= -100)", (1.0, 0.0, 0.0, 100.0))):
    a = section_once(plane)
    print("%s: %s; length %.6f, area %.6f" % (name, ", ".join("%s %d" % (k, int(getattr(a, k))) for k in SECTION_COUNTS), a.length, a.area), flush=True)
    best, med = timed(lambda: section_once(plane))
    cbest, cmed = timed(lambda: clip_once(plane))
    out_bytes = int(a.nP_out) * (3 * V.element_size() + 8) + int(a.nS_out) * 8
    print("    section: median %.3f ms (best %.3f) | mc33hip_clip_surface on the same plane, no normals: median %.3f ms (best %.3f) | the section is %.3f MB, "
          "V and T over the link %.3f ms" % (med, best, cmed, cbest, out_bytes / 1e6, whole / link / 1e6), flush=True)
    print("    EXPECTATION a section costs no more than the clip of the same plane: %s (%.3f ms against %.3f, %+.0f %%)"
          % ("CONFIRMED" if med <= cmed else "REFUTED", med, cmed, 100.0 * (med - cmed) / cmed), flush=True)

steps = 64
normal = (0.0, 0.0, 1.0)
offsets = [-(-3.9 + 7.8 * k / (steps - 1)) for k in range(steps)][::-1]  # the planes z = -3.9 .. 3.9, ascending offsets
seg, length, area = g.section_ladder(V, T, normal, offsets)
lbest, lmed = timed(lambda: g.section_ladder(V, T, normal, offsets))
sbest, smed = timed(lambda: [section_once(normal + (w,)) for w in offsets], reps=3)
singles = [int(section_once(normal + (w,)).nS_out) for w in offsets]
assert singles == seg.tolist()
print("a ladder of %d planes along z: %d to %d segments a plane, area %.4f to %.4f" % (steps, seg.min(), seg.max(), area.min(), area.max()), flush=True)
print("    mc33hip_section_ladder: median %.3f ms (best %.3f) | %d single calls: median %.3f ms (best %.3f), %.3f ms a call"
      % (lmed, lbest, steps, smed, sbest, smed / steps), flush=True)
print("    EXPECTATION a %d-step ladder costs less than %d single calls: %s (%.3f ms against %.3f, a factor of %.1f)"
      % (steps, steps, "CONFIRMED" if lmed < smed else "REFUTED", lmed, smed, smed / lmed), flush=True)
