#!/usr/bin/env python3
"""Developer tool: per-wave start/end stamps of k_sweep (MC33_HIP_TRACE_FILE) on the 1024^3 bench field.

Prints how long waves live, when they start and finish relative to the kernel, and the spread per XCD
(block index mod 8), to see whether the kernel is bound by a tail of late waves.
usage (GPU box): python tools/trace_sweep.py [n]
"""
import os as _os; _os.environ.setdefault("MC33_HIP_TIMING", "2")  # per-pass hipEvents for timing(): DeviceGrid starts without them
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
out = os.path.join("gpurun_out", "sweep_trace.bin")
os.makedirs("gpurun_out", exist_ok=True)
os.environ["MC33_HIP_TRACE_FILE"] = out

import torch  # noqa: E402

from mc33_c_library_amd import api, fields  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
dev = torch.device("cuda:0")
grid, r0, d = fields.cos_field_cube(n, dev)
g = api.DeviceGrid(grid, r0=r0, d=d)
for iso in (0.004, 0.003, 0.002, 0.001, 0.0):  # (five sweeps - a repeated count of one isovalue is answered from the last; the second
    # builds the table and publishes its live count, the third asks for a size, the fourth agrees and is the first by the sized
    # plan - it pays for making it - and the fifth, the one traced, goes by a plan that stays)
    cnt = g.count(iso)
torch.cuda.synchronize()
print("nV", cnt.nV, "nT", cnt.nT, "timing", g.timing())
# one record per LAUNCHED wave (block index * 4 + wave): with a range table block b streams the four tiles of entry b of the packed
# live list (mc33hip_sweep_packed; a library from before it: the tiles of live[1 + b], mc33hip_sweep_live), blocks beyond the list
# leave no stamp
t = np.fromfile(out, dtype=np.uint64).reshape(-1, 4).astype(np.int64)
import ctypes as C  # noqa: E402
wave = np.arange(len(t))            # launched wave = launched block * 4 + wave of the block
tile = wave.copy()                  # ... and the tile it streamed: its own without a live list
dead_wave = np.zeros(len(t), bool)  # the wave of a dead tile in a block with live ones (it walks an empty tile)
info = (C.c_ulonglong * 3)()
tiles = None
if hasattr(g.lib, "mc33hip_sweep_plan") and g.lib.mc33hip_sweep_plan(g.ctx, None, 0, C.byref(info)) == 0:
    tiles = np.zeros((int(info[0]), 4), np.uint32)
    assert g.lib.mc33hip_sweep_plan(g.ctx, C.c_void_p(tiles.ctypes.data), tiles.shape[0], C.byref(info)) == 0
    print("plan %d: %d tiles, %d blocks resident" % (info[2], len(tiles), info[1]))
linfo = (C.c_ulonglong * 2)()
pinfo = (C.c_ulonglong * 3)()
if hasattr(g.lib, "mc33hip_sweep_packed") and g.lib.mc33hip_sweep_packed(g.ctx, None, 0, C.byref(pinfo)) == 0:
    ent = np.zeros((max(int(pinfo[0]), 1), 4), np.uint32)
    assert g.lib.mc33hip_sweep_packed(g.ctx, C.c_void_p(ent.ctypes.data), ent.shape[0], C.byref(pinfo)) == 0
    nlive = int(pinfo[0])
    whole = int(((ent[:nlive, 0] >> 31) != 0).sum())
    print("packed blocks %d (%d whole groups) for %d live tiles of %d planned: %.2f of the %d resident blocks" % (nlive, whole, pinfo[1], pinfo[2], nlive / max(int(info[1]), 1), info[1]))
    ent[:, 0] &= 0x7FFFFFFF
    b = np.minimum(wave // 4, max(nlive - 1, 0))
    tile = ent[b, wave % 4].astype(np.int64)
    dead_wave = tile == 0xFFFFFFFF
    tile[dead_wave | (wave // 4 >= nlive)] = -1
elif hasattr(g.lib, "mc33hip_sweep_live") and g.lib.mc33hip_sweep_live(g.ctx, None, 0, C.byref(linfo)) == 0:
    live = np.zeros(max(int(linfo[1]), 1), np.uint32)
    assert g.lib.mc33hip_sweep_live(g.ctx, C.c_void_p(live.ctypes.data), live.shape[0], C.byref(linfo)) == 0
    nlive = int(linfo[0])
    print("live blocks %d of %d planned" % (nlive, linfo[1]))
    b = np.minimum(wave // 4, max(nlive - 1, 0))
    tile = (live[b] >> 4).astype(np.int64) * 4 + wave % 4
    dead_wave = ((live[b] >> (wave % 4)) & 1) != 0
    tile[wave // 4 >= nlive] = -1
launched = wave // 4
keep = t[:, 1] > 0
t, launched, tile, dead_wave = t[keep], launched[keep], tile[keep], dead_wave[keep]
t0 = t[:, 0].min()
s = (t[:, 0] - t0) / 100.0  # us (100 MHz)
e = (t[:, 1] - t0) / 100.0
print("waves", len(t), "kernel span us", e.max())
for name, v in (("start", s), ("end", e), ("life", e - s)):
    q = np.percentile(v, [0, 5, 25, 50, 75, 95, 99, 100])
    print(name.ljust(6), " ".join("%8.1f" % x for x in q))
blk = launched
for x in range(8):
    m = (blk % 8) == x
    print("xcd %d: waves %5d  start med %7.1f max %7.1f  end med %7.1f max %7.1f" % (x, m.sum(), np.median(s[m]), s[m].max(), np.median(e[m]), e[m].max()))
# waves in flight over time
ts = np.linspace(0, e.max(), 21)
print("in flight:", " ".join("%d" % ((s <= x) & (e > x)).sum() for x in ts))
if dead_wave.any():
    print("dead waves of mixed blocks: %d, life med %.1f max %.1f us" % (dead_wave.sum(), np.median((e - s)[dead_wave]), (e - s)[dead_wave].max()))
lw = ~dead_wave
print("live waves: %d, life med %.1f us; the five that end last:" % (lw.sum(), np.median((e - s)[lw])))
for i in np.argsort(e)[-5:]:
    where = tuple(int(x) for x in tiles[tile[i]]) if tiles is not None and 0 <= tile[i] < len(tiles) else "?"
    print("  block %5d tile %6d (seg, yt, z_lo, z_hi) %s  start %7.1f end %7.1f" % (launched[i], tile[i], where, s[i], e[i]))
