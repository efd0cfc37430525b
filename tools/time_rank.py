#!/usr/bin/env python3
"""Developer timing of the rank filter (results in profiles/rank_timing.txt).

On the bench's 1024^3 float cos field and, if memory allows, on a 2048 x 2048 x 1024 ushort field: mc33hip_rank_grid into a
tensor with rows on 16-byte boundaries - the median at radii (1, 1, 1) and (1, 1, 0), the minimum at (1, 1, 1), the maximum at
(2, 2, 2) and the copy (0, 0, 0) - timed with stream events through torch around the call, after a warm-up, median (and best) of 7
calls.  The call waits for its stream, so the event time holds that host round trip.  Per case: milliseconds,
(source bytes + output bytes) / time, and that as a fraction of mc33hip_probe_read's ceiling on the same buffer in the same process.
Beside them the nearest operation the library had before: mc33hip_resample_grid with three taps per axis at stride 1 - the same
halo, the same bytes - timed in the same process.

usage: tools/time_rank.py [points per axis of the float grid, default 1024] [--no-u16]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402

REPS = 7
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")
CASES = (("median", (1, 1, 1)), ("median", (1, 1, 0)), ("min", (1, 1, 1)), ("max", (2, 2, 2)), ("median", (0, 0, 0)))


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


def study(name, tensor, r0, d):
    g = DeviceGrid(tensor, r0=r0, d=d)
    sb = tensor.element_size()
    npz, npy, npx = tensor.shape
    src_bytes = tensor.numel() * sb
    best, med, nbytes = g.probe_read()
    ceiling = nbytes / best / 1e6
    print("%s: %.1f MB; mc33hip_probe_read %.4f ms (median %.4f): %.0f GB/s" % (name, src_bytes / 1e6, best, med, ceiling), flush=True)
    unit = max(1, 16 // sb)
    out = torch.empty((npz, npy, (npx + unit - 1) // unit * unit), dtype=tensor.dtype, device=dev)
    moved = 2 * src_bytes

    def row(label, call):
        best, med = timed(call)
        print("%s, %-32s median %.3f ms (best %.3f): %.0f GB/s of source + output, %.2f of the read ceiling" % (
            name, label + ":", med, best, moved / med / 1e6, moved / med / 1e6 / ceiling), flush=True)
        return med

    t3 = [0.25, 0.5, 0.25]
    base = row("resample, 3 taps per axis, stride 1", lambda: g.resample_into(out, npx, (t3, t3, t3), (1, 1, 1)))
    flat = row("resample, 3 taps along x and y", lambda: g.resample_into(out, npx, (t3, t3, None), (1, 1, 1)))
    for rank, radius in CASES:
        label = "copy (0, 0, 0)" if radius == (0, 0, 0) else "%s (%d, %d, %d)" % ((rank,) + radius)
        med = row(label, lambda: g.rank_into(out, npx, rank, radius))
        print("    %.2f times the 3-tap resampling of the same halo" % (med / (flat if radius[2] == 0 and radius != (0, 0, 0) else base)), flush=True)
    del out
    torch.cuda.empty_cache()
    g.close()


grid, r0, d = fields.cos_field_cube(n, dev, -4.0, 4.0)
study("%d^3 float" % n, grid, r0, d)
del grid
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
