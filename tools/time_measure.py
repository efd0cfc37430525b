#!/usr/bin/env python3
"""Developer timing of the measuring passes (results in profiles/r08_measure.txt).

  device ABI : on the bench's 1024^3 float field at iso 0 (one component) and on the same spacing over a five times wider domain
               at iso 2 (some 15 000 closed blobs, more than 2^24 vertices): hipEvent time and wall of mc33hip_measure_surface,
               mc33hip_label_components and mc33hip_measure_components, best / median of 22 calls; the bytes each must move
               (12 nT of T, 12 nV of V once, 4 nV of labels) over that time, beside the 8 TB/s peak and mc33hip_probe_read's
               ceiling in this process.  The time of each kernel by itself comes from running this part under
               `rocprofv3 --kernel-trace --stats -- python tools/time_measure.py --device-only`.
  C API      : wall of MC33_measure_isosurface against calculate_isosurface + free_surface_memory (what a caller had to do
               before to get at the numbers, not counting its own pass over the mesh), alternated pairs; MC33_measure_isosurfaces
               with 8 isovalues against calculate_isosurfaces with the same 8.

usage: tools/time_measure.py [points per axis, default 1024] [--device-only | --capi-only]
       tools/time_measure.py --trace-summary <kernel_trace.csv>    best / median of each new kernel per field, from that trace"""
import ctypes as C
import os
import sys
import time

if "--trace-summary" in sys.argv:  # (the device part runs its calls on the one-component field first, then on the other)
    import collections
    import csv
    rows = sorted(csv.DictReader(open(sys.argv[sys.argv.index("--trace-summary") + 1])), key=lambda r: int(r["Start_Timestamp"]))
    per = collections.defaultdict(list)
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if name.startswith(("k_measure", "k_cc_", "k_mesh_")):  # (k_mesh_*: the shared scan the component table launches)
            per[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, us in per.items():
        a, b = sorted(us[:len(us) // 2]), sorted(us[len(us) // 2:])
        print("%-34s %3d calls | one component: best %7.1f median %7.1f us | many components: best %7.1f median %7.1f us"
              % (name, len(a), a[0], a[len(a) // 2], b[0], b[len(b) // 2]))
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402
from mc33_capi import MC33Lib, product_path  # noqa: E402

PEAK = 8000.0  # GB/s, HBM3E spec peak of the MI355X
REPS = 22
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")


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
    del N
    nV, nT = cnt.nV, cnt.nT
    best, med, nbytes = g.probe_read(10)
    ceiling = nbytes / best / 1e6
    print("\n%s: %d^3 float on [%g, %g]^3, iso %g: %d vertices, %d triangles" % (label, n, lo, hi, iso, nV, nT))
    print("mc33hip_probe_read over the grid: best %.3f ms -> %.0f GB/s (%.1f %% of peak)" % (best, ceiling, 100 * ceiling / PEAK), flush=True)
    m = g.measure(V, T)
    labels, nc, nu = g.label_components(T, nV)
    table = g.measure_components(V, T, labels)
    print("area %.9g volume %.9g; %d components, %d unreferenced vertices; largest component %d triangles" % (m.area, m.volume, nc, nu, int(table["nT"].max())))
    rows = (("mc33hip_measure_surface", lambda: g.measure(V, T), 12 * nT + 12 * nV + 12 * nV, "12 nT + 12 nV gathered + 12 nV for the box"),
            ("mc33hip_label_components", lambda: g.label_components(T, nV), 12 * nT + 4 * nV * 3 + 12 * nT + nV * 2 + 5 * nV, "T twice, labels written twice and read twice, flags"),
            ("mc33hip_measure_components (table fetched, %d rows)" % nc, lambda: g.lib.mc33hip_measure_components(g.ctx, C.c_void_p(V.data_ptr()), nV, C.c_void_p(T.data_ptr()), nT, C.c_void_p(labels.data_ptr()), C.c_void_p(table.ctypes.data), nc, C.byref(C.c_ulonglong())),
             2 * 12 * nT + 12 * nV + 4 * nV * 3 + 4 * nV + 3 * nV, "T twice, V once, labels three times, ranks, flags"))
    res = {}
    for name, call, moved, what in rows:
        b, md, wb, wm = timed(call)
        gbs = moved / b / 1e6
        res[name.split()[0]] = b
        print("%s: event best %.4f ms, median %.4f ms; wall best %.4f, median %.4f ms; %s = %.1f MB -> %.0f GB/s = %.1f %% of peak, %.1f %% of the read ceiling"
              % (name, b, md, wb, wm, what, moved / 1e6, gbs, 100 * gbs / PEAK, 100 * gbs / ceiling), flush=True)
    del g, grid, V, T, labels
    torch.cuda.empty_cache()
    return res, nT


if "--capi-only" not in sys.argv:
    one, nT1 = device_part("one component", -4.0, 4.0, 0.0)
    many, nTm = device_part("many components", -80.0 * n / 1024, 80.0 * n / 1024, 2.0)
    a, b = one["mc33hip_label_components"] / nT1 * 1e6, many["mc33hip_label_components"] / nTm * 1e6
    print("\nmc33hip_label_components: %.3f ns per triangle on the one-component surface, %.3f on the many-component one: ratio %.2f" % (a, b, a / b), flush=True)
if "--device-only" in sys.argv:
    sys.exit(0)

# --- the C API -------------------------------------------------------------------------------------------------------------------
from test_gpu_measure import CMeasure, bind_measure_api  # noqa: E402

grid, r0, d = fields.cos_field_cube(n, dev)
data = grid.cpu().numpy()
del grid
torch.cuda.empty_cache()
lib = MC33Lib(product_path("f32"), "f32")
bind_measure_api(lib)
L = lib.lib
L.calculate_isosurfaces.restype = C.c_uint
L.calculate_isosurfaces.argtypes = [C.POINTER(lib.MC33), C.POINTER(lib.real), C.c_uint, C.POINTER(C.POINTER(lib.SURFACE))]
G, keep = lib.make_grid(data, r0, d)
M = L.create_MC33(G)
assert M
m = CMeasure()


def download():
    S = L.calculate_isosurface(M, C.c_float(0.0))
    assert S
    L.free_surface_memory(S)


def measure():
    assert L.MC33_measure_isosurface(M, C.c_float(0.0), C.byref(m)) == 0


def wall(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


for _ in range(3):
    download(); measure()
pairs = [(wall(download), wall(measure)) for _ in range(12)]
print("\nC API, %d^3, iso 0, alternated pairs: calculate_isosurface + free_surface_memory / MC33_measure_isosurface, ms" % n)
print("  " + "  ".join("%.2f/%.2f" % p for p in pairs))
dl, ms = sorted(p[0] for p in pairs), sorted(p[1] for p in pairs)
print("  download path best %.3f median %.3f; measure best %.3f median %.3f; measure lower in %d of %d pairs; area %.9g volume %.9g"
      % (dl[0], dl[6], ms[0], ms[6], sum(1 for p in pairs if p[1] < p[0]), len(pairs), m.area, m.volume), flush=True)

isos = (C.c_float * 8)(*[-1.4 + 0.4 * k for k in range(8)])
out = (C.POINTER(lib.SURFACE) * 8)()
many = (CMeasure * 8)()


def download8():
    assert L.calculate_isosurfaces(M, isos, 8, out) == 8
    for k in range(8):
        L.free_surface_memory(out[k])


def measure8():
    assert L.MC33_measure_isosurfaces(M, isos, 8, many) == 8


download8(); measure8()
pairs = [(wall(download8), wall(measure8)) for _ in range(5)]
print("8 isovalues, alternated pairs: calculate_isosurfaces + 8 free_surface_memory / MC33_measure_isosurfaces, ms")
print("  " + "  ".join("%.2f/%.2f" % p for p in pairs), flush=True)
L.free_MC33(M)
