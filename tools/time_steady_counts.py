#!/usr/bin/env python3
"""Developer tool: the no-regression figures beside the flagship (profiles/r11_block_skip.txt D, profiles/r12_plan_balance.txt E),
one figure per process.

  python tools/time_steady_counts.py u8 | u16 | nodead | alt     steady counts at 1024^3, two isovalues alternated: 30 counts
                                                                  after 8, ms per count (host wall, the device drained)
  python tools/time_steady_counts.py oneshot                     a fresh DeviceGrid over the 512^3 c3 field, create + extract,
                                                                  best of 5, ms
u8: 128 + 40 f as uchar, 128.5 / 129.5; u16: 32768 + 10000 f, 32768.5 / 32769.5; nodead: cos(2 pi x / 256 + 0.3), a field with a
table and no dead tile, 0 / 0.01; alt: the c3 field f = cos x + cos y + cos z on [-4, 4]^3, 0 / 1.5.
MC33_LIB_DIR names the build (two trees side by side)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mc33_c_library_amd import api, fields  # noqa: E402

dev = torch.device("cuda:0")
which = sys.argv[1] if len(sys.argv) > 1 else "alt"
if which == "oneshot":
    t, r0, d = fields.cos_field_cube(512, dev)
    best = None
    for rep in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = api.DeviceGrid(t, r0=r0, d=d)
        V, N, T, cnt = g.extract(0.0)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
        g.close()
    print("oneshot 512^3: best of 5 %.4f ms (nV %d)" % (best, cnt.nV))
    sys.exit(0)
if which == "u8":
    f, _, _ = fields.cos_field_cube(1024, dev)
    t = (128.0 + 40.0 * f).clamp_(0, 255).to(torch.uint8)
    del f
    isos = (128.5, 129.5)
elif which == "u16":
    t = fields.cos_field_u16(1024, 1024, 1024, dev)
    isos = (32768.5, 32769.5)
elif which == "nodead":
    x = torch.arange(1024, device=dev, dtype=torch.float64)
    row = torch.cos(2.0 * torch.pi * x / 256.0 + 0.3).to(torch.float32)
    t = row.expand(1024, 1024, 1024).contiguous()
    isos = (0.0, 0.01)
else:
    t, _, _ = fields.cos_field_cube(1024, dev)
    isos = (0.0, 1.5)
g = api.DeviceGrid(t)
for k in range(8):
    g.count(isos[k & 1])
torch.cuda.synchronize()
t0 = time.perf_counter()
for k in range(30):
    cnt = g.count(isos[k & 1])
torch.cuda.synchronize()
print("%s: %.4f ms per count (nV %d)" % (which, (time.perf_counter() - t0) * 1e3 / 30.0, cnt.nV))
