#!/usr/bin/env python3
"""Developer timing of the component compaction (results in profiles/filter_times.txt).

On the bench's 1024^3 float field at iso 0 (one component) and on the same spacing over a five times wider domain at iso 2 (some
15 000 closed blobs, more than 2^24 vertices): hipEvent time of mc33hip_compact_components into exact-size outputs, with the map
and no attribute, after a warm-up, median (and best) of 22 calls, for three selections - keep all, keep every second component,
keep one component.  Next to each: a device-to-device copy of as many bytes as the call writes into oV, oN, oT and oMap, made in this
process and timed the same way, and the bytes the algorithm must move, computed here from nV, nT, nV_out and nT_out:

    per vertex    4 (label) + 4 (new[] written) + 4 (new[] read by the row pass) + 4 (oMap) + 2 (flags written and read)
    per triangle  3 x 12 (T read by the flag, the count and the renumbering pass)
    per kept row  2 x (12 or 24) + 2 x 12 (V and N read and written), 12 per kept triangle written

(the gathers through new[] and the flags hit lines that neighbours share and are not counted).  The call waits for its counts, so
its event time holds one host round trip as the measuring calls' does.

usage: tools/time_filter.py [points per axis, default 1024]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mc33_c_library_amd import DeviceGrid, fields  # noqa: E402
from mc33_c_library_amd.api import Compaction, ECAPACITY  # noqa: E402

PEAK = 8000.0  # GB/s, HBM3E spec peak of the MI355X
REPS = 22
n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1024
dev = torch.device("cuda:0")


def timed(call):
    ev = []
    for _ in range(REPS + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    ev = sorted(ev[2:])
    return ev[0], ev[len(ev) // 2]


def algorithmic_bytes(nV, nT, nV2, nT2, real_bytes):
    return nV * (4 + 4 + 4 + 4 + 2) + nT * 36 + nV2 * (2 * 3 * real_bytes + 2 * 12) + nT2 * 12


def part(label, lo, hi, iso):
    grid, r0, d = fields.cos_field_cube(n, dev, lo, hi)
    g = DeviceGrid(grid, r0=r0, d=d)
    V, N, T, cnt = g.extract(iso)
    nV, nT = cnt.nV, cnt.nT
    labels, nc, nu = g.label_components(T, nV)
    table = g.measure_components(V, T, labels)
    print("\n%s: %d^3 float on [%g, %g]^3, iso %g: %d vertices, %d triangles, %d components, %d unreferenced vertices"
          % (label, n, lo, hi, iso, nV, nT, nc, nu), flush=True)
    roots_all = np.ascontiguousarray(table["root"], dtype=np.uint32)
    for what, roots in (("keep all", roots_all), ("keep every second component", roots_all[1::2].copy()), ("keep one component", roots_all[:1].copy())):
        a = Compaction()
        a.V, a.N, a.T, a.label, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), labels.data_ptr(), nV, nT
        a.roots, a.n_roots = (roots.ctypes.data if roots.size else None), roots.size
        rc = g.lib.mc33hip_compact_components(g.ctx, C.byref(a))  # the size query
        assert rc in (0, ECAPACITY), g.lib.mc33hip_last_error().decode(errors="replace")
        nV2, nT2 = int(a.nV_out), int(a.nT_out)
        oV = torch.empty((max(nV2, 1), 3), dtype=V.dtype, device=dev)
        oN = torch.empty((max(nV2, 1), 3), dtype=torch.float32, device=dev)
        oT = torch.empty((max(nT2, 1), 3), dtype=torch.int32, device=dev)
        oMap = torch.empty((nV,), dtype=torch.int32, device=dev)
        a.oV, a.oN, a.oT, a.oMap, a.capV, a.capT = oV.data_ptr(), oN.data_ptr(), oT.data_ptr(), oMap.data_ptr(), nV2, nT2

        def call():
            assert g.lib.mc33hip_compact_components(g.ctx, C.byref(a)) == 0
        best, med = timed(call)
        out_bytes = nV2 * (3 * V.element_size() + 12) + nT2 * 12 + nV * 4  # oV, oN, oT and oMap
        src = torch.empty((max(out_bytes, 4) // 4,), dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        cbest, cmed = timed(lambda: dst.copy_(src))
        alg = algorithmic_bytes(nV, nT, nV2, nT2, V.element_size())
        print("%-28s %9d of %9d vertices, %9d of %9d triangles, %6d components | compaction: median %.4f ms (best %.4f); algorithmic bytes %.1f MB -> %.0f GB/s "
              "(%.1f %% of peak) | copy of the %.1f MB it writes: median %.4f ms (best %.4f) | ratio %.2f"
              % (what, nV2, nV, nT2, nT, int(a.components_kept), med, best, alg / 1e6, alg / med / 1e6, 100 * alg / med / 1e6 / PEAK, out_bytes / 1e6, cmed, cbest,
                 med / cmed), flush=True)
        del oV, oN, oT, oMap, src, dst
    del g, grid, V, N, T, labels
    torch.cuda.empty_cache()


part("one component", -4.0, 4.0, 0.0)
part("many components", -80.0 * n / 1024, 80.0 * n / 1024, 2.0)
