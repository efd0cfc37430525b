#!/usr/bin/env python3
"""Developer timing of the grid resampling (results in profiles/resample_timing.txt).

On the bench's 1024^3 float cos field and, if memory allows, on a 2048 x 2048 x 1024 ushort field: mc33hip_resample_grid into a
tensor with rows on 16-byte boundaries - identity taps, a Gaussian of sigma 1 (radius 3) and of sigma 2 (radius 6), each at strides
1 and 2 - timed with stream events through torch around the call, after a warm-up, median (and best) of 7 calls.  The call copies
its taps and waits for its stream, so the event time holds that host round trip.  Per configuration: milliseconds and
(source bytes + output bytes) / time, beside mc33hip_probe_read's ceiling on the same buffer in the same process, and beside the
same resampling done the way a caller can do it on the device without this library: three strided torch.nn.functional.conv3d
passes in float64 over replicate-padded planes (a time only: it is not the same arithmetic bit for bit, and it runs over slabs of
planes where the float64 volume does not fit).

usage: tools/time_resample.py [points per axis of the float grid, default 1024] [--no-u16]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields, gaussian_taps  # noqa: E402

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


def conv_passes(t, taps, stride, slab=32):
    """the yardstick: x, y, z passes of conv3d in float64 with replicate padding, over slabs of output planes (with their halo in z)"""
    npz = t.shape[0]
    rz = (len(taps[2]) - 1) // 2
    w = [torch.tensor(k, dtype=torch.float64, device=dev) for k in taps]
    outs = []
    nz_out = (npz - 1) // stride[2] + 1
    for z0 in range(0, nz_out, slab):
        z1 = min(z0 + slab, nz_out)
        lo, hi = z0 * stride[2] - rz, (z1 - 1) * stride[2] + rz
        idx = torch.arange(lo, hi + 1, device=dev).clamp_(0, npz - 1)
        a = t.index_select(0, idx)
        a = (a.to(torch.int32) & 0xFFFF if t.dtype == torch.int16 else a).to(torch.float64)[None, None]
        rx, ry = (len(taps[0]) - 1) // 2, (len(taps[1]) - 1) // 2
        a = Fn.conv3d(Fn.pad(a, (rx, rx, 0, 0, 0, 0), mode="replicate"), w[0].view(1, 1, 1, 1, -1), stride=(1, 1, stride[0]))
        a = Fn.conv3d(Fn.pad(a, (0, 0, ry, ry, 0, 0), mode="replicate"), w[1].view(1, 1, 1, -1, 1), stride=(1, stride[1], 1))
        a = Fn.conv3d(a, w[2].view(1, 1, -1, 1, 1), stride=(stride[2], 1, 1))
        outs.append(a[0, 0].to(torch.float32) if t.dtype == torch.float32 else a[0, 0].add_(0.5).floor_().clamp_(0, 65535).to(torch.int32))
    return outs


def study(name, tensor, r0, d):
    g = DeviceGrid(tensor, r0=r0, d=d)
    sb = tensor.element_size()
    src_bytes = tensor.numel() * sb
    best, med, nbytes = g.probe_read()
    ceiling = nbytes / best / 1e6
    print("%s: %.1f MB; mc33hip_probe_read %.4f ms (median %.4f): %.0f GB/s" % (name, src_bytes / 1e6, best, med, ceiling), flush=True)
    for label, taps in (("identity", None), ("sigma 1 (r = 3)", gaussian_taps(1.0)), ("sigma 2 (r = 6)", gaussian_taps(2.0))):
        for s in (1, 2):
            stride = (s, s, s)
            t3 = (taps, taps, taps)
            npx, npy, npz = g.resampled_size(t3, stride)
            unit = max(1, 16 // sb)
            out = torch.empty((npz, npy, (npx + unit - 1) // unit * unit), dtype=tensor.dtype, device=dev)
            best, med = timed(lambda: g.resample_into(out, npx, t3, stride))
            moved = src_bytes + npx * npy * npz * sb
            line = "%s, %-15s stride %d: %d x %d x %d out | median %.3f ms (best %.3f): %.0f GB/s of source + output, %.2f of the read ceiling" % (
                name, label + ",", s, npx, npy, npz, med, best, moved / med / 1e6, moved / med / 1e6 / ceiling)
            del out
            torch.cuda.empty_cache()
            print(line, flush=True)
            line = "    the same"
            try:
                k = taps or [1.0]
                ybest, ymed = timed(lambda: conv_passes(tensor, (k, k, k), stride), reps=2)
                line += " as torch conv3d x 3 in float64: median %.3f ms (best %.3f), %.1f times the call" % (ymed, ybest, ymed / med)
            except RuntimeError as e:  # (out of memory)
                line += " as torch conv3d x 3: %s" % str(e).splitlines()[0][:60]
            print(line, flush=True)
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
