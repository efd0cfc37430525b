#!/usr/bin/env python3
"""Developer timing of the contour spectrum (results in profiles/spectrum_timing.txt).

On the bench's 1024^3 float cos field, on white noise of the same size - the adverse case: every cell is cut at many isovalues and
neighbouring samples share no rank - and, if memory allows, on a 2048 x 2048 x 1024 ushort field: mc33hip_grid_spectrum with
ladders of 8, 64 and 255 isovalues, timed with stream events through torch around the call, after a warm-up, median (and best) of
7 calls.  The call copies its isovalues, waits for its stream and brings 4 KB back, so the event time holds that host round trip.
Beside each line two yardsticks taken in the same process on the same buffer:
  - mc33hip_probe_read: what a single stream of the grid reaches; the spectrum's time as a fraction of it;
  - the n counts a caller needs without the spectrum: mc33hip_sweep_many over groups of 8 isovalues, then mc33hip_count of each
    (the path as it is: this tool changes nothing of it).  Wall time of the whole ladder, median of 3 after a warm-up.  On the
    noise field only the first 8 isovalues are counted - every cell becomes a work record there - and the line says so.

usage: tools/time_spectrum.py [points per axis of the float grids, default 1024] [--no-cos] [--no-noise] [--no-u16]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, MC33Error, fields, isovalue_ladder  # noqa: E402

REPS = 7
LADDERS = (8, 64, 255)
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


def counts(g, isos):
    """the yardstick: the active cells of every isovalue by the count path"""
    out = []
    for k in range(0, len(isos), 8):
        group = isos[k:k + 8]
        g.sweep_many(group)
        out += [int(g.count(v).active_cells) for v in group]
    return out


def wall(call, reps=3, warm=1):
    t = []
    for _ in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    t = sorted(t[warm:])
    return t[0], t[len(t) // 2]


def study(name, tensor, r0, d, count_at_most=None):
    g = DeviceGrid(tensor, r0=r0, d=d)
    nbytes_grid = tensor.numel() * tensor.element_size()
    best, med, nbytes = g.probe_read()
    ceiling_ms = best * nbytes_grid / nbytes
    print("%s: %.1f MB; mc33hip_probe_read %.4f ms (median %.4f): %.0f GB/s" % (name, nbytes_grid / 1e6, best, med, nbytes / best / 1e6), flush=True)
    first = g.spectrum([])
    print("    samples %g .. %g, %d NaN" % (first.sample_min, first.sample_max, first.nan_samples), flush=True)
    for steps in LADDERS:
        isos = isovalue_ladder(first.sample_min, first.sample_max, steps, g.dtype)
        got = g.spectrum(isos)
        best, med = timed(lambda: g.spectrum(isos))
        line = "%s, n = %3d: median %.3f ms (best %.3f): %.0f GB/s of the grid, %.2f of the read ceiling; cut cells at most %.1f %% of the cells" % (
            name, steps, med, best, nbytes_grid / med / 1e6, ceiling_ms / med, 100.0 * int(got.cut_cells.max()) / got.cells)
        print(line, flush=True)
        few = isos if count_at_most is None else isos[:count_at_most]
        try:
            assert counts(g, few) == [int(x) for x in got.cut_cells[:len(few)]], "the count path disagrees with the spectrum"
            cbest, cmed = wall(lambda: counts(g, few))
            if len(few) == steps:
                print("    the %d counts it replaces (sweep_many by 8, count each): median %.3f ms (best %.3f), %.1f times the spectrum" % (steps, cmed, cbest, cmed / med), flush=True)
            else:
                print("    the first %d of the %d counts it replaces: median %.3f ms (best %.3f): %.1f times the WHOLE spectrum already" % (len(few), steps, cmed, cbest, cmed / med), flush=True)
        except (MC33Error, RuntimeError) as e:  # (out of memory)
            print("    the counts it replaces: %s" % str(e).splitlines()[0][:100], flush=True)
        torch.cuda.empty_cache()
    g.close()


if "--no-cos" not in sys.argv:
    grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
    study("%d^3 float cos" % n, grid, r0, d)
    del grid
    torch.cuda.empty_cache()
if "--no-noise" not in sys.argv:
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    noise = torch.empty((n, n, n), dtype=torch.float32, device=dev)
    noise.uniform_(-1.0, 1.0, generator=gen)
    study("%d^3 float white noise" % n, noise, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), count_at_most=8)
    del noise
    torch.cuda.empty_cache()
if "--no-u16" not in sys.argv:
    try:
        x = torch.cos(torch.linspace(-8.0, 8.0, 2 * n, dtype=torch.float64, device=dev))
        z = torch.cos(torch.linspace(-4.0, 4.0, n, dtype=torch.float64, device=dev))
        u16 = torch.empty((n, 2 * n, 2 * n), dtype=torch.int16, device=dev)
        for k in range(n):  # (a plane at a time: the float64 volume would be 34 GB)
            f = 32768.0 + 10000.0 * ((x[None, :] + x[:, None]) + z[k])
            u16[k] = torch.round(f).to(torch.int32).to(torch.int16)
        study("%d x %d x %d ushort" % (2 * n, 2 * n, n), u16, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    except torch.cuda.OutOfMemoryError as e:
        print("the ushort grid does not fit: %s" % str(e).splitlines()[0], flush=True)
