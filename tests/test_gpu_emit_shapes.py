"""The emit passes at forced launch shapes.  Every pass behind the sweep sizes its grid by the device and by the counts of the
extraction before (enqueue_emit, enqueue_tail): on a test-sized grid a wave of k_emit_vertices walks zero or one batch, a block
of k_emit_fast_triangles makes one round, the slow kernels one - the software pipeline over a wave's batches (d0 / d1 / d2,
rec0 / rec1, more / more2, finish_rec for the next batch, next_batch of a batch that creates nothing), the later rounds of the
triangle pass and the grid-stride loops of the slow kernels are reached by a full-size run or not at all.  Here the shapes are
forced small (MC33_HIP_EMIT_V_BLOCKS, MC33_HIP_EMIT_BLOCKS, MC33_HIP_SLOW_BLOCKS, MC33_HIP_SLOW_SLOTS, MC33_HIP_TRI_FIRST,
MC33_HIP_CELLS_BLOCKS; read when a context is created) on the small grids of tests/emit_cases.py.

Every id makes a fresh context under its shape and extracts at the case's isovalue twice (the second call picks its kernels
from the first call's counts), at a second isovalue that moves the record count by more than a factor of two, and at the first
again: the hints are stale in both directions.  Every extraction writes into canaried tensors (tests/canaries.py) and is
compared with the unmodified reference (oracle/_ref) on the dense array: counts, T as uint32, V and N by bit pattern, no
tolerance anywhere; a NaN normal must be a NaN in the same place.  (One case more than the reference can judge, iso = -0.0 on
float samples that hold zeros, is compared with the library's own arrays under the default shape: emit_cases.py.)  Every id reads the shape that was launched
(DeviceGrid.emit_shape), checks the block counts against what it asked for, and books what tests/emit_shapes.py makes of it;
the last test of the module asserts what the whole module reached.  Nothing may be left out there: if the device's batch
counts ever miss a walk length, the block list changes, not the assertion."""
import collections
import math
import types

import numpy as np
import pytest

import emit_cases as ec
import emit_shapes as es
import layouts as lo
from canaries import FRONT, canaried, only_the_rows_were_written, windows

pytestmark = pytest.mark.gpu

# what the module reached: tag -> walk lengths of k_emit_vertices (4: at least 4); rounds of the other loops
REACH = {"walk": collections.defaultdict(set), "triangle_rounds": set(), "thread_rounds": set(), "slots_rounds": set(), "fallback": 0,
         "negzero": set(), "ghost_batch": 0, "t12_launched": set(), "ids": 0}
SEEN = {}          # (case, shape, step) -> EmitShape, for the report
DEFAULT_SLOW = {}  # case -> slow records of its first extraction under the default shape
_refs, _nneg, _tensors, _own = {}, {}, {}, {}


def data_key(case):
    return (case.make.func.__name__,) + case.make.args


def reference(reflibs, case, iso):
    """the unmodified reference on the dense array, once per (grid, geometry, isovalue), shared and never written"""
    key = (case.dtype, data_key(case), repr(iso), case.r0, case.d, case.inclined, case.normal_neg)
    if case.own_reference and negzero(iso):
        return _own[case.name]
    if key not in _refs:
        lib = reflibs[case.dtype]
        if case.normal_neg:
            from mc33_capi import MC33Lib, ref_path
            if case.dtype not in _nneg:
                _nneg[case.dtype] = MC33Lib(ref_path(case.dtype, nneg=True), case.dtype)
            lib = _nneg[case.dtype]
        lib.set_triangular(case.inclined == "cell")
        try:
            s = lib.isosurface(case.make(), iso, case.r0, case.d, inclined=ec.matrices(case.inclined) if case.inclined else None)
        finally:
            lib.set_triangular(False)
        for a in (s.V, s.N, s.T):
            a.setflags(write=False)
        _refs[key] = s
    return _refs[key]


def own_reference(reflibs, monkeypatch, case):
    """For iso = -0.0 on a float grid that holds zeros, where the reference's triangles depend on its earlier calls: what the
    library gives under the launch shape the device picks, by count and emit from a fresh context - with the reference's number
    of vertices.  Every forced shape must give these arrays, bit for bit."""
    if case.name not in _own:
        from mc33_c_library_amd import DeviceGrid
        for k in ec.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        g = configure(DeviceGrid(device_tensor(case), r0=case.r0, d=case.d), case)
        V, N, T, cnt = g.extract(case.iso)
        s = types.SimpleNamespace(nV=cnt.nV, nT=cnt.nT, V=V.cpu().numpy(), N=N.cpu().numpy(), T=T.cpu().numpy().view(np.uint32))
        g.close()
        assert s.nV == reflibs[case.dtype].isosurface(case.make(), case.iso, case.r0, case.d).nV and s.nT > 0
        _own[case.name] = s


def device_tensor(case):
    """the grid on the device, once per (grid, layout): dense, or a strided window of a poisoned flat tensor"""
    key = (case.dtype, data_key(case), case.layout)
    if key not in _tensors:
        data = case.make()
        assert data.dtype == ec.NP[case.dtype]
        if case.layout:
            lay = lo.layout(case.layout, data.shape, data.dtype.itemsize)
            flat = lo.to_device(lo.place(data, lay, (case.iso, case.iso2)))
            _tensors[key] = (flat, lo.device_view(flat, data.shape, lay))
        else:
            t = lo.to_device(np.ascontiguousarray(data))
            _tensors[key] = (t, t)
    return _tensors[key][1]


def configure(g, case):
    import ctypes as C
    if case.inclined:
        A, Ai = ec.matrices(case.inclined)
        g.set_inclined(A, Ai, triangular=case.inclined == "cell")
    if case.normal_neg:
        assert g.lib.mc33hip_set_normal_neg(g.ctx, C.c_int(1)) == 0
    return g


def negzero(iso):
    return iso == 0.0 and math.copysign(1.0, iso) < 0.0


def check_rows(V, N, T, ref, what):
    """the canaried tensors against the reference; a NaN normal of the reference must be a NaN here (its payload is the
    device's own), everything else equal by bit pattern"""
    got = N[FRONT:FRONT + ref.nV].cpu().numpy()
    nan = np.isnan(ref.N)
    assert np.array_equal(np.isnan(got), nan), what
    n = ref.N
    if nan.any():
        n = ref.N.copy()
        n[nan] = got[nan]
    only_the_rows_were_written(V, N, T, types.SimpleNamespace(V=ref.V, N=n, T=ref.T), what)


def check_blocks(sh, env, what):
    """the block counts that were launched are what the switches asked for, after rounding"""
    assert sh.vertex_blocks % 8 == 0 and sh.triangle_blocks % 8 == 0, (what, sh)
    if "MC33_HIP_EMIT_V_BLOCKS" in env:
        assert sh.vertex_blocks == es.round8(env["MC33_HIP_EMIT_V_BLOCKS"]), (what, sh)
    else:
        assert sh.vertex_blocks >= 64, (what, sh)  # (a block per CU at least)
    if "MC33_HIP_EMIT_BLOCKS" in env:
        assert sh.triangle_blocks == es.round8(env["MC33_HIP_EMIT_BLOCKS"]), (what, sh)
    else:
        assert sh.triangle_blocks >= 16384, (what, sh)
    if "MC33_HIP_SLOW_BLOCKS" in env:
        assert sh.slow_blocks == int(env["MC33_HIP_SLOW_BLOCKS"]), (what, sh)
    if "MC33_HIP_SLOW_SLOTS" in env:
        assert sh.slow_kernel in (int(env["MC33_HIP_SLOW_SLOTS"]), 2), (what, sh)
    if "MC33_HIP_TRI_FIRST" in env:
        assert sh.triangles_first == int(env["MC33_HIP_TRI_FIRST"]), (what, sh)


def book(case, shape, step, iso, sh, env, ghost=False):
    SEEN[(case.name, shape, step)] = sh
    check_blocks(sh, env, (case.name, shape, step))
    lengths = es.walk_lengths(sh.batches, sh.vertex_blocks)
    for tag in ec.tags(case) + (("ghost",) if ghost else ()):
        REACH["walk"][tag] |= lengths
    REACH["triangle_rounds"].add(es.triangle_rounds(sh.records, sh.triangle_blocks))
    if shape == "t12":
        REACH["t12_launched"].add(sh.triangle_blocks)
    if sh.slow_kernel != 2 and sh.slow_records:
        rounds, fell_back = es.slow_rounds(sh.slow_records, sh.slow_blocks, sh.slow_kernel == 1)
        if fell_back:
            REACH["fallback"] += 1
        elif sh.slow_kernel == 1:
            REACH["slots_rounds"].add(rounds)
        else:
            REACH["thread_rounds"].add(rounds)
        if negzero(iso) and not fell_back:
            REACH["negzero"].add(sh.slow_kernel)


def put_in_force(monkeypatch, case, shape, reflibs):
    env = dict(ec.SHAPES[shape])
    env.update(dict(case.env))
    if shape == "slow2":
        if case.name not in DEFAULT_SLOW:  # (the id was picked alone: its default shape first)
            run_slabs(reflibs, monkeypatch, case, "default") if case.slabs else run(reflibs, monkeypatch, case, "default", steps=1)
        env["MC33_HIP_SLOW_BLOCKS"] = str(max(1, (DEFAULT_SLOW[case.name] + 31) // 32))
    for k in ec.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return env


def run(reflibs, monkeypatch, case, shape, steps=4):
    import torch
    from mc33_c_library_amd import DeviceGrid
    env = put_in_force(monkeypatch, case, shape, reflibs)
    g = configure(DeviceGrid(device_tensor(case), r0=case.r0, d=case.d), case)
    records = []
    for step, iso in enumerate((case.iso, case.iso, case.iso2, case.iso)[:steps]):
        ref = reference(reflibs, case, iso)
        what = (case.name, shape, step, iso)
        V, N, T = canaried(ref.nV, ref.nT, case.dtype == "f64")
        cnt, ok = g.extract_into(iso, *windows(V, N, T, ref.nV, ref.nT))
        torch.cuda.synchronize()
        assert ok and (cnt.nV, cnt.nT) == (ref.nV, ref.nT), (what, cnt.nV, cnt.nT, ref.nV, ref.nT)
        check_rows(V, N, T, ref, what)
        sh = g.emit_shape()
        assert sh.records == cnt.active_cells, (what, sh)
        print("%-20s %-14s step %d iso %-14r nV %7d nT %7d %s" % (case.name, shape, step, iso, cnt.nV, cnt.nT, tuple(sh)))
        book(case, shape, step, iso, sh, env)
        records.append(sh.records)
        if shape == "default" and step == 0:
            DEFAULT_SLOW[case.name] = sh.slow_records
    g.close()
    if steps == 4:
        assert records[0] == records[1] == records[3] and max(records[0], records[2]) > 2 * min(records[0], records[2]), (case.name, records)


def run_slabs(reflibs, monkeypatch, case, shape):
    """test_gpu_layouts.test_z_slabs_as_windows_of_one_strided_buffer's arrangement on a dense tensor: every slab a context on
    its window of planes, counted, then emitted at the vertex base of the slabs below into canaried tensors of its own; slab k's
    rows are rows of the reference's arrays, so the concatenated arrays are the reference's"""
    import torch
    from mc33_c_library_amd import DeviceGrid, Range
    env = put_in_force(monkeypatch, case, shape, reflibs)
    t = device_tensor(case)
    nz_total = t.shape[0] - 1
    bounds = ec.slab_bounds(nz_total)
    slabs = []
    for zb, ze in zip(bounds[:-1], bounds[1:]):
        ghost = 1 if zb else 0
        p_lo, p_hi = max(zb - ghost - 1, 0), min(ze + 1, nz_total)
        slabs.append((DeviceGrid(t[p_lo:p_hi + 1], nz_total=nz_total, plane0=p_lo), Range(zb, ze, ghost, 0)))
    assert sum(1 for _, r in slabs if r.ghost_below) >= 1
    for step, iso in enumerate((case.iso, case.iso, case.iso2, case.iso)):
        ref = reference(reflibs, case, iso)
        counts = [g.count(iso, r) for g, r in slabs]
        assert sum(c.nV for c in counts) == ref.nV and sum(c.nT for c in counts) == ref.nT, (case.name, shape, step)
        vbase = tbase = 0
        for k, ((g, r), c) in enumerate(zip(slabs, counts)):
            what = (case.name, shape, step, iso, "slab %d" % k)
            V, N, T = canaried(c.nV, c.nT, False)
            g.emit_into(*windows(V, N, T, c.nV, c.nT), vbase)
            torch.cuda.synchronize()
            part = types.SimpleNamespace(nV=c.nV, V=ref.V[vbase:vbase + c.nV], N=ref.N[vbase:vbase + c.nV], T=ref.T[tbase:tbase + c.nT])
            check_rows(V, N, T, part, what)
            sh = g.emit_shape()
            print("%-20s %-14s step %d iso %-6r slab %d nV %7d nT %7d ghost nV %5d %s" % (case.name, shape, step, iso, k, c.nV, c.nT, c.nV_ghost, tuple(sh)))
            book(case, shape, step, iso, sh, env, ghost=bool(r.ghost_below))
            if r.ghost_below and c.nV_ghost:  # vertices of the slice below z_begin: records there, in batches of their own slot
                REACH["ghost_batch"] += 1
            if shape == "default" and step == 0:
                DEFAULT_SLOW[case.name] = max(DEFAULT_SLOW.get(case.name, 0), sh.slow_records)
            vbase += c.nV
            tbase += c.nT
    for g, _ in slabs:
        g.close()


@pytest.mark.parametrize("shape", list(ec.SHAPES))
@pytest.mark.parametrize("case", [c.name for c in ec.CASES])
def test_emit_at_launch_shape(reflibs, monkeypatch, case, shape):
    c = ec.BY_NAME[case]
    if c.own_reference:
        own_reference(reflibs, monkeypatch, c)
    (run_slabs if c.slabs else run)(reflibs, monkeypatch, c, shape)
    REACH["ids"] += 1


def test_the_module_reached_every_loop():
    """Over all ids above (the whole module must have run): per sample type, for the inclined store and for a ghost slab some
    wave of k_emit_vertices walked exactly 1, exactly 2, exactly 3 and at least 4 batches; the triangle pass made at least 2
    and at least 4 rounds; k_emit_slow at least 2; k_emit_slow_slots exactly 2, and it fell back; both slow kernels ran with
    iso = -0.0; a ghost slab had a batch below z_begin; MC33_HIP_EMIT_BLOCKS=12 launched 16."""
    for tag in sorted(REACH["walk"]):
        print("walk lengths %-9s %s" % (tag, sorted(REACH["walk"][tag])))
    print("triangle rounds %s\nk_emit_slow rounds %s\nk_emit_slow_slots rounds %s, fell back %d times\n-0.0 under kernels %s, ghost batches in %d emits" % (
        sorted(REACH["triangle_rounds"]), sorted(REACH["thread_rounds"]), sorted(REACH["slots_rounds"]), REACH["fallback"],
        sorted(REACH["negzero"]), REACH["ghost_batch"]))
    assert REACH["ids"] == len(ec.CASES) * len(ec.SHAPES), "run the whole module: %d of %d ids ran" % (REACH["ids"], len(ec.CASES) * len(ec.SHAPES))
    for tag in ("f32", "f64", "u8", "u16", "u32", "inclined", "ghost"):
        assert REACH["walk"][tag] >= {1, 2, 3, 4}, (tag, sorted(REACH["walk"][tag]))
    assert any(2 <= r < 4 for r in REACH["triangle_rounds"]) and any(r >= 4 for r in REACH["triangle_rounds"]), sorted(REACH["triangle_rounds"])
    assert any(r >= 2 for r in REACH["thread_rounds"]), sorted(REACH["thread_rounds"])
    assert 2 in REACH["slots_rounds"], sorted(REACH["slots_rounds"])
    assert REACH["fallback"] > 0
    assert REACH["negzero"] == {0, 1}, REACH["negzero"]
    assert REACH["ghost_batch"] > 0
    assert REACH["t12_launched"] == {16}, REACH["t12_launched"]
