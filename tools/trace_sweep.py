#!/usr/bin/env python3
"""Developer tool: per-wave start/end stamps of k_sweep (MC33_HIP_TRACE_FILE) on the 1024^3 bench field.

Prints how long waves live, when they start and finish relative to the kernel, and the spread per XCD
(block index mod 8), to see whether the kernel is bound by a tail of late waves.
usage (GPU box): python tools/trace_sweep.py [n] [--fit]

--fit: the cost of a wave's life (profiles/r12_plan_balance.txt A).  Every live wave's life is joined with the geometry of the
tile it streamed - its planes, its batches (planes x batches of sample rows per plane of its y tile), whether its block is a
whole group - and with its live blocks, summed from mc33hip_block_words over the strips of the tile (none with
MC33_HIP_BLOCKS=0), and a least-squares fit life ~ a batches + b planes + c live blocks + d grouped is printed with the spread
of its residual and the share of the variance each term carries.  b / a is the weight of a plane in batches (plan_sweep).
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

fit = "--fit" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--fit"]
n = int(argv[0]) if argv else 1024
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
    pw = C.c_double(0.0)
    if hasattr(g.lib, "mc33hip_sweep_plan_weight") and g.lib.mc33hip_sweep_plan_weight(g.ctx, C.byref(pw)) == 0:
        print("cut with a plane weight of %.2f batches" % pw.value)
    for y in sorted(set(tiles[:, 1].tolist())):
        d = (tiles[tiles[:, 1] == y, 3] - tiles[tiles[:, 1] == y, 2]).astype(np.int64) + 1
        if y in (0, int(tiles[:, 1].max())):
            print("  y tile %d: %d tiles, planes %d - %d (median %d)" % (y, len(d), d.min(), d.max(), np.median(d)))
linfo = (C.c_ulonglong * 2)()
pinfo = (C.c_ulonglong * 3)()
if hasattr(g.lib, "mc33hip_sweep_packed") and g.lib.mc33hip_sweep_packed(g.ctx, None, 0, C.byref(pinfo)) == 0:
    ent = np.zeros((max(int(pinfo[0]), 1), 4), np.uint32)
    assert g.lib.mc33hip_sweep_packed(g.ctx, C.c_void_p(ent.ctypes.data), ent.shape[0], C.byref(pinfo)) == 0
    nlive = int(pinfo[0])
    whole = int(((ent[:nlive, 0] >> 31) != 0).sum())
    print("packed blocks %d (%d whole groups) for %d live tiles of %d planned: %.2f of the %d resident blocks" % (nlive, whole, pinfo[1], pinfo[2], nlive / max(int(info[1]), 1), info[1]))
    group_entry = (ent[:, 0] >> 31) != 0
    ent[:, 0] &= 0x7FFFFFFF
    b = np.minimum(wave // 4, max(nlive - 1, 0))
    tile = ent[b, wave % 4].astype(np.int64)
    dead_wave = tile == 0xFFFFFFFF
    grouped_wave = group_entry[b] & (wave // 4 < nlive)
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
grouped_wave = grouped_wave[keep] if "grouped_wave" in globals() else np.zeros(len(t), bool)
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


def fit_lives():
    """life ~ a batches + b planes + c live blocks + d grouped over the live waves of the traced sweep"""
    m = lw & (tile >= 0) & (tile < len(tiles))
    tl = tiles[tile[m]].astype(np.int64)
    life = (e - s)[m]
    ny = grid.shape[1] - 1
    rows = np.minimum(64, ny + 1 - 63 * tl[:, 1])
    per_plane = (rows + 3) // 4                       # batches of 4 sample rows (float samples)
    planes = tl[:, 3] - tl[:, 2] + 1                  # a tile re-reads the plane it begins with
    batches = planes * per_plane
    grouped = grouped_wave[m].astype(np.float64)
    cols = [("batches", batches.astype(np.float64)), ("planes", planes.astype(np.float64))]
    nyt, nseg = (ny + 62) // 63, (grid.shape[2] - 1 + 255) // 256
    words = np.zeros((grid.shape[0], nyt, nseg), np.uint64)
    if hasattr(g.lib, "mc33hip_block_words") and g.lib.mc33hip_block_words(g.ctx, C.c_void_p(words.ctypes.data), words.nbytes) == 0:
        live_of_word = np.zeros(words.shape, np.int64)
        for k in range(16):                           # entries 0 .. 15: the 64 x 16 sample blocks of a strip, two bits each, 0 live
            live_of_word += ((words >> np.uint64(2 * k)) & np.uint64(3)) == 0
        live_of_word[words == np.uint64(0xFFFFFFFFFFFFFFFF)] = 0   # (no sweep wrote the word: a strip of a dead tile)
        cum = np.concatenate([np.zeros((1, nyt, nseg), np.int64), np.cumsum(live_of_word, axis=0)])
        hi = np.minimum(tl[:, 3] + 1, grid.shape[0])
        blocks = cum[hi, tl[:, 1], tl[:, 0]] - cum[tl[:, 2], tl[:, 1], tl[:, 0]]
        cols.append(("live blocks", blocks.astype(np.float64)))
        print("live blocks per live wave: med %d, min %d, max %d; of 16 per plane: %.3f" % (np.median(blocks), blocks.min(), blocks.max(), blocks.sum() / (16.0 * planes.sum())))
    else:
        print("no block words (no sweep has left blocks out): the fit goes without the live-blocks term")
    if grouped.any() and not grouped.all():
        cols.append(("grouped", grouped))
    print("fit over %d live waves; octiles of their lives, us: %s" % (m.sum(), " ".join("%.1f" % x for x in np.percentile(life, np.arange(9) * 12.5))))
    print("y tiles: " + ", ".join("yt %d: %d waves, %d batches/plane, planes med %d, life med %.1f" % (
        y, (tl[:, 1] == y).sum(), per_plane[tl[:, 1] == y][0], np.median(planes[tl[:, 1] == y]), np.median(life[tl[:, 1] == y])) for y in sorted(set(tl[:, 1].tolist()))))
    for names in ([c[0] for c in cols[:2]], [c[0] for c in cols]):
        X = np.stack([v for k, v in cols if k in names], axis=1)
        for const in (False, True):
            A = np.concatenate([X, np.ones((len(X), 1))], axis=1) if const else X
            coef, *_ = np.linalg.lstsq(A, life, rcond=None)
            res = life - A @ coef
            var = life.var()
            print("life ~ " + " + ".join("%.4f %s" % (coef[k], names[k]) for k in range(len(names))) + (" + %.2f" % coef[-1] if const else ""))
            print("    residual: sd %.2f us (sd of the lives %.2f), 5 / 50 / 95 %%: %.1f %.1f %.1f; variance explained %.3f" % (
                res.std(), life.std(), *np.percentile(res, [5, 50, 95]), 1.0 - res.var() / var))
            print("    share of the variance by term: " + ", ".join("%s %.3f" % (names[k], np.cov(coef[k] * X[:, k], life)[0, 1] / life.var(ddof=1)) for k in range(len(names))))
            print("    b / a = %.2f batches per plane" % (coef[1] / coef[0]))
            if len(names) > 2 and "live blocks" in names:
                print("    c / a = %.2f batches per live block" % (coef[2] / coef[0]))


if fit:
    if tiles is None:
        sys.exit("--fit needs mc33hip_sweep_plan")
    fit_lives()
