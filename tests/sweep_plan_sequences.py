"""The call sequences whose sweep plans are recorded in tests/golden/sweep_plans.json (tools/record_sweep_plans.py) and replayed by
tests/test_gpu_sweep_plan_golden.py: after every step the plan in force as mc33hip_sweep_plan reports it - tiles {seg, yt, z_lo,
z_hi} in launch order, info[] = tiles, resident blocks, plan bit - and mc33hip_sweep_plan_weight.  The file records what the
library planned BEFORE planning moved into mc33_sweep_plan.h; a change that is meant to alter a plan records it again.

Shapes, isovalues and fields (steep, banded) are those of tests/sweep_harness.py.  Shapes are points z, y, x.  A sequence is (name, shape, environment, steps); the environment is read when the context is made."""
import ctypes as C
import os

import numpy as np

from sweep_harness import A, B, BIG, HIGH, LOW, SHALLOW, STEEP_ISO, banded, steep

ONE_ROUND = {"MC33_HIP_SWEEP_BLOCKS_PER_CU": "1", "MC33_HIP_LIVE": "1"}   # BIG: one block per compute unit, every sweep with a table by a list
GHOST_FROM = 17                                                       # the sub-range of B: slices 17 .. 39 with a ghost slice below


def thrice(iso):
    return [("extract", iso)] * 3   # no table, the table just built, the table with a count available


def sequences():
    out = []
    # 1. three single extractions at a steep isovalue
    out.append(("steep A", A, {}, thrice(STEEP_ISO[A])))
    out.append(("steep B", B, {}, thrice(STEEP_ISO[B])))
    out.append(("steep BIG", BIG, dict(ONE_ROUND, MC33_HIP_RZ_TABLE="1"), thrice(STEEP_ISO[BIG])))
    # 2. a sized plan: a forced size between one round (1024 tiles at one block per CU of a 256-CU device) and BIG's cap at one
    # plane per tile (1639), and a narrow grid that takes the weighted cut only with MC33_HIP_BLOCKS=1; with and without a weight
    for weight in (None, "0"):
        w = {} if weight is None else {"MC33_HIP_PLANE_WEIGHT": weight}
        tag = "" if weight is None else ", plane weight 0"
        out.append(("sized BIG" + tag, BIG, dict(ONE_ROUND, MC33_HIP_TABLE_TILES="1300", MC33_HIP_BLOCKS="1", **w), thrice(STEEP_ISO[BIG])))
        out.append(("sized A" + tag, A, dict(MC33_HIP_LIVE="1", MC33_HIP_TABLE_TILES="150", MC33_HIP_BLOCKS="1", **w), thrice(STEEP_ISO[A])))
    # ... and sized by the counts the sweeps publish: three tiles in four live, then one in four
    out.append(("sized by the count", "banded 96", dict(ONE_ROUND), [("extract", LOW[0])] * 6 + [("extract", HIGH)] * 6))
    # 3. passes over 4, then 2 + 1 isovalues, the counts that consume the lanes, then single extractions until slot 2 holds a
    # sized plan beside the default one in slot 1
    out.append(("many, then single", "banded 96", dict(ONE_ROUND),
                [("sweep_many", LOW[:4]), ("sweep_many", LOW[:3]), ("count", LOW[2]), ("count", LOW[1]), ("count", LOW[0])] +
                [("extract", LOW[0] + 1.0)] * 4 + [("extract", HIGH)] * 4 + [("sweep_many", LOW[:4]), ("count", LOW[3]), ("extract", HIGH)]))
    # 4. a sub-range with z_begin > 0 and a ghost plane below, in a window with plane0 > 0
    out.append(("ghost below", B, {"MC33_HIP_LIVE": "1", "MC33_HIP_TABLE_TILES": "90"}, [("count_ghost", STEEP_ISO[B])] * 3))
    # (a range one slice deep is planned on the host alone: tests/test_sweep_plan_cpu.py)
    # 5. columns asked for more chunks than there are planes
    out.append(("shallow", SHALLOW, dict(ONE_ROUND, MC33_HIP_TABLE_TILES="100000"), thrice(STEEP_ISO[SHALLOW])))
    out.append(("shallow by depth", SHALLOW, dict(ONE_ROUND, MC33_HIP_RZ_TABLE="1"), thrice(STEEP_ISO[SHALLOW])))
    # 6. MC33_HIP_RZ alone: the two plans are one;  7. with MC33_HIP_RZ_TABLE they are two again
    for shape, name in ((B, "B"), (BIG, "BIG")):
        out.append(("rz 2 " + name, shape, dict(ONE_ROUND, MC33_HIP_RZ="2"), thrice(STEEP_ISO[shape])))
        out.append(("rz 2, rz table 1 " + name, shape, dict(ONE_ROUND, MC33_HIP_RZ="2", MC33_HIP_RZ_TABLE="1"), thrice(STEEP_ISO[shape])))
    return out


def field_of(shape):
    return banded(96) if shape == "banded 96" else steep(shape)


def plan_in_force(g):
    """{tiles: flat list of seg, yt, z_lo, z_hi, info: [tiles, resident blocks, plan bit], weight}"""
    info = (C.c_ulonglong * 3)()
    assert g.lib.mc33hip_sweep_plan(g.ctx, None, 0, C.byref(info)) == 0
    t = np.zeros((int(info[0]), 4), np.uint32)
    assert g.lib.mc33hip_sweep_plan(g.ctx, C.c_void_p(t.ctypes.data), t.shape[0], C.byref(info)) == 0
    w = C.c_double(-1.0)
    assert g.lib.mc33hip_sweep_plan_weight(g.ctx, C.byref(w)) == 0
    return {"tiles": [int(x) for x in t.reshape(-1)], "info": [int(x) for x in info], "weight": w.value}


def replay(seq, tensor):
    """the plan in force after every step of a sequence; tensor: its field on the device (field_of)"""
    from mc33_c_library_amd import DeviceGrid, Range
    name, shape, env, steps = seq
    keep = {k: os.environ.get(k) for k in os.environ if k.startswith("MC33_HIP_")}
    for k in keep:
        del os.environ[k]
    os.environ.update(env)
    try:
        nz_total = tensor.shape[0] - 1
        if steps[0][0] == "count_ghost":
            g = DeviceGrid(tensor[GHOST_FROM - 2:], nz_total=nz_total, plane0=GHOST_FROM - 2)
        else:
            g = DeviceGrid(tensor)
        out = []
        for what, arg in steps:
            if what == "extract":
                g.extract(arg)
            elif what == "count":
                g.count(arg)
            elif what == "sweep_many":
                g.sweep_many(arg)
            elif what == "count_ghost":
                g.count(arg, Range(GHOST_FROM, nz_total, 1, 0))
            else:
                raise ValueError(what)
            out.append(plan_in_force(g))
        g.close()
        return out
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in keep.items() if v is not None})
