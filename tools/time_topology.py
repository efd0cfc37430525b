#!/usr/bin/env python3
"""Developer timing of the topology passes.

  On the bench's 1024^3 float field at iso 0 (one component, 7.8 M triangles) and on the same spacing over a five times wider
  domain at iso 2 (some 15 000 closed blobs, 55.8 M triangles): hipEvent time and wall of mc33hip_label_components - the
  existing pass of the same kind - mc33hip_surface_topology and mc33hip_component_topology in one process on one mesh, best /
  median of 20 calls.

usage: tools/time_topology.py [points per axis, default 1024]
       rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_topology.py [n] --trace-run
                      only mc33hip_surface_topology, 1 + 10 calls per field, for the trace
       tools/time_topology.py --trace-summary <kernel_trace.csv>
                      best / median of each kernel per block of calls of that trace, and the insertion rate"""
import collections
import ctypes as C
import os
import sys
import time

TRACE_CALLS = 11

if "--trace-summary" in sys.argv:
    import csv
    rows = sorted(csv.DictReader(open(sys.argv[sys.argv.index("--trace-summary") + 1])), key=lambda r: int(r["Start_Timestamp"]))
    names = ["one component", "many components"]
    per = collections.defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if name.startswith(("k_topo_", "k_cc_", "k_mesh_")):  # (k_mesh_*: the shared scan and table clear these calls launch)
            per[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in per.items():
        k = len(us) // len(names)
        print("%-24s %4d launches" % (name, len(us)))
        for b, label in enumerate(names):
            x = sorted(us[b * k:(b + 1) * k][k // TRACE_CALLS:])  # (without the warm-up call's launches)
            print("    %-18s best %9.1f median %9.1f us" % (label, x[0], x[len(x) // 2]))
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402

REPS = 20
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")
TRACE = "--trace-run" in sys.argv


def timed(call):
    ev, wall = [], []
    for _ in range(REPS + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    ev, wall = sorted(ev[2:]), sorted(wall[2:])
    return ev[0], ev[len(ev) // 2], wall[0], wall[len(wall) // 2]


def device_part(label, lo, hi, iso):
    grid, r0, d = fields.cos_field_cube(n, dev, lo, hi)
    g = DeviceGrid(grid, r0=r0, d=d)
    V, N, T, cnt = g.extract(iso)
    del N, V
    nV, nT = cnt.nV, cnt.nT
    print("\n%s: %d^3 float on [%g, %g]^3, iso %g: %d vertices, %d triangles" % (label, n, lo, hi, iso, nV, nT), flush=True)
    if TRACE:
        for _ in range(TRACE_CALLS):
            t = g.topology(T, nV)
        print(t)
    else:
        labels, nc, nu = g.label_components(T, nV)
        b, md, wb, wm = timed(lambda: g.label_components(T, nV))
        print("mc33hip_label_components: event best %.4f ms, median %.4f ms; wall best %.4f, median %.4f ms" % (b, md, wb, wm), flush=True)
        t = g.topology(T, nV)
        table = g.component_topology(T, nV, labels)
        print("%r; table of %d rows, genus of the first %d" % (t, table.shape[0], table["genus"][0]))
        b, md, wb, wm = timed(lambda: g.topology(T, nV))
        print("mc33hip_surface_topology: event best %.4f ms, median %.4f ms; wall best %.4f, median %.4f ms; %.3f ns per triangle, %.1f M edge uses per ms of the call"
              % (b, md, wb, wm, b / nT * 1e6, 3 * nT / b / 1e6), flush=True)
        b, md, wb, wm = timed(lambda: g.lib.mc33hip_component_topology(g.ctx, C.c_void_p(T.data_ptr()), nT, nV, C.c_void_p(labels.data_ptr()),
                                                                      C.c_void_p(table.ctypes.data), nc, C.byref(C.c_ulonglong())))
        print("mc33hip_component_topology (labels given, table of %d rows fetched): event best %.4f ms, median %.4f ms; wall best %.4f, median %.4f ms"
              % (nc, b, md, wb, wm), flush=True)
    del g, grid, T
    torch.cuda.empty_cache()


device_part("one component", -4.0, 4.0, 0.0)
device_part("many components", -80.0 * n / 1024, 80.0 * n / 1024, 2.0)
