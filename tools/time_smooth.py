#!/usr/bin/env python3
"""Developer timing of the surface smoothing (results in profiles/smooth_timing.txt).

On the bench's 1024^3 float field at iso 0, extracted on the device: one mc33hip_smooth_surface call of 10 iterations (20 passes)
with normals, after a warm-up call, at timing level 2 - hipEvent times of the adjacency build, of every pass (median and best of
the 20) and of the normals (mc33hip_smooth_timing).  Beside the pass:

  - its rate on its algorithmic bytes: per vertex 2 row bounds (8) + the fixed flag (1) + deg (4) + a row read and a row written,
    per directed neighbour a 4-byte index and a gathered row (12 bytes; 24 in the double build);
  - mc33hip_probe_read's ceiling on the resident grid, in this process;
  - the same pass written in torch on the same device and mesh - index_add_ in float64 over the directed edge list, then the
    update: a yardstick that is not the code under test.  Its result is compared with the library's (not bit for bit: the
    atomics of index_add_ add in any order).

usage: tools/time_smooth.py [points per axis, default 1024]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402

PEAK = 8000.0  # GB/s, HBM3E spec peak of the MI355X
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")

grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
g = DeviceGrid(grid, r0=r0, d=d)
V, N, T, cnt = g.extract(0.0)
nV, nT = cnt.nV, cnt.nT
print("%d^3 float on [-4, 4]^3, iso 0: %d vertices, %d triangles" % (n, nV, nT), flush=True)
best, med, nbytes = g.probe_read(10)
print("read ceiling (mc33hip_probe_read, %d MB): best %.4f ms = %.0f GB/s, median %.4f ms" % (nbytes >> 20, best, nbytes / best / 1e6, med), flush=True)

out = torch.empty_like(V)
g.smooth(V, T, out=out)  # warm-up: the scratch is allocated here
g.set_timing(2)
_, N2, info = g.smooth(V, T, out=out)
adj, nrm, passes = g.smooth_timing()
g.set_timing(0)
print("counts: %s" % info)
ps = sorted(passes)
pmed, pbest = ps[len(ps) // 2], ps[0]

# the directed edge list, from T alone (distinct neighbours: torch.unique of the packed pairs)
t = T.to(torch.int64)
a = torch.cat([t[:, 0], t[:, 1], t[:, 2], t[:, 1], t[:, 2], t[:, 0]])
b = torch.cat([t[:, 1], t[:, 2], t[:, 0], t[:, 0], t[:, 1], t[:, 2]])
key = torch.unique(a * (1 << 32) + b)
src, dst = key >> 32, key & 0xFFFFFFFF
sum_deg = int(key.numel())
del a, b, t
deg = torch.bincount(src, minlength=nV).to(torch.float64)
fixed = deg == 0  # (compared with a library pass that pins nothing)
rb = V.element_size() * 3
alg = nV * (8 + 1 + 4 + 2 * rb) + sum_deg * (4 + rb)
print("adjacency build %.4f ms | pass: median %.4f ms, best %.4f of %d; algorithmic bytes %.1f MB (sum of degrees %d) -> %.0f GB/s at the median "
      "(%.1f %% of peak, %.2f of the read ceiling) | normals %.4f ms"
      % (adj, pmed, pbest, len(ps), alg / 1e6, sum_deg, alg / pmed / 1e6, 100 * alg / pmed / 1e6 / PEAK, (alg / pmed) / (nbytes / best), nrm), flush=True)


def torch_pass(P, f):
    s = torch.zeros((nV, 3), dtype=torch.float64, device=dev)
    s.index_add_(0, src, P[dst].to(torch.float64))
    p = P.to(torch.float64)
    L = s / deg[:, None] - p
    q = (p + f * L).to(P.dtype)
    return torch.where(fixed[:, None], P, q)


ev = []
for _ in range(7):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    Q = torch_pass(V, 0.5)
    e1.record()
    e1.synchronize()
    ev.append(e0.elapsed_time(e1))
ev = sorted(ev[2:])
one, _, _ = g.smooth(V, T, iterations=1, mu=0.0, pin_boundary=False, normals=False)
diff = (one.to(torch.float64) - Q.to(torch.float64)).abs().max().item()
print("the same pass in torch (index_add_ in float64 over %d directed edges, then the update): median %.4f ms, best %.4f | ratio to the library's pass %.2f | "
      "largest difference between the two results %.3g" % (sum_deg, ev[len(ev) // 2], ev[0], ev[len(ev) // 2] / pmed, diff), flush=True)
