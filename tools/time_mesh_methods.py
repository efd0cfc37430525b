#!/usr/bin/env python3
"""Developer timing of the DeviceGrid methods of the mesh passes themselves (results in
profiles/host_layer_timing.txt).

The other timing tools of the mesh passes time the library's calls on a 1024^3 surface, where the host's share of a call does not
show.  This one times the Python methods on the 64^3 cos field at iso 0 (15072 vertices): wall per call with the stream
synchronized before and after, median and best of 200 calls after 20, for extract, measure_iso, topology_iso,
measure_components, component_topology, compact_components, simplify and clip - the last three with one attribute riding along.

usage: tools/time_mesh_methods.py [points per axis, default 64] [calls, default 200]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402

args = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, calls = args[0] if args else 64, args[1] if len(args) > 1 else 200
dev = torch.device("cuda:0")
grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
g = DeviceGrid(grid, r0=r0, d=d)
V, N, T, cnt = g.extract(0.0)
labels, nc, nu = g.label_components(T, cnt.nV)
roots = g.measure_components(V, T, labels)["root"]
attr = torch.arange(cnt.nV, dtype=torch.int32, device=dev)
cell = tuple(2.0 * x for x in d)
print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles, %d components; %d calls after 20" % (n, cnt.nV, cnt.nT, nc, calls), flush=True)

methods = (("extract", lambda: g.extract(0.0)),
           ("measure_iso", lambda: g.measure_iso(0.0)),
           ("topology_iso", lambda: g.topology_iso(0.0)),
           ("measure_components", lambda: g.measure_components(V, T, labels)),
           ("component_topology", lambda: g.component_topology(T, cnt.nV, labels)),
           ("compact_components", lambda: g.compact_components(V, N, T, labels, roots, attrs=(attr,))),
           ("simplify", lambda: g.simplify(V, T, cell, attrs=(attr,))),
           ("clip", lambda: g.clip(V, N, T, (0.0, 0.0, 1.0, 0.0), attrs=(attr,))))
for name, call in methods:
    wall = []
    for _ in range(20 + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall = sorted(wall[20:])
    print("%-20s median %.4f ms, best %.4f" % (name, wall[len(wall) // 2], wall[0]), flush=True)
