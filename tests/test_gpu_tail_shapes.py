"""The tail of an extraction - the passes between the sweep and the emit passes - on long thin grids.  Every pass of the tail
changes shape with the size of the grid: the slow-cell and dirty-segment lists are cut into at most 1024 groups of 2^shift slice
slots (ListChunks; shift grows above 65536 slots), and from 4096 chunks of 2048 row segments on the prefix sums go by groups of
32 chunks (SCAN_GROUPED_FROM).  Both thresholds count slots and row segments, not samples: the grids of tests/tail_shapes.py
cross them with a few megabytes - 65536 to 131076 planes of 6 x 6 samples, 64 y tiles, 8193 row segments, 4100 slices of 2048
rows.  test_tail_shapes_cpu.py checks, without a GPU, that those grids put work into every list group and every scan chunk.

Every id makes a fresh context, extracts into canaried tensors (tests/canaries.py) and compares with the unmodified reference
(oracle/_ref) on the dense array: counts, T as uint32, V and N by bit pattern, no tolerance anywhere; a NaN normal must be a NaN
in the same place.  It then reads DeviceGrid.tail_shape() and asserts what tail_shapes.tail() predicted.  The list ids extract at
the case's isovalue twice, at a second isovalue that lies on no sample (no slow cell: the alias gate closes and opens), and at
the first again, and assert from DeviceGrid.list_counts() that every list group in use held slow cells and dirty segments.  The
scan ids run sequences of ranges on one context: grouped, ungrouped and grouped again, a ghost slice, a second isovalue, the
scan sums reallocated, three lanes at once.  A range that is not the whole grid is counted, emitted at the vertex base of the
slices below it and compared with its rows of the reference's arrays (the arrangement of test_gpu_emit_shapes.run_slabs); a
second context counts the rest of the grid, and the counts add up to the reference's.

One case more than the reference can judge: iso = -0.0 on float samples that hold zeros.  There the reference reads id caches
that no cell has written - its triangles hold arbitrary numbers that change with its earlier calls (DESIGN.md 8,
test_gpu_parity.test_negative_zero_isovalue_is_deterministic) - and the library leaves an id that is no vertex in those places.
At that isovalue the 65540-slot grid (shift 7) is held to the reference's number of vertices and to the library's own arrays
from two z-slabs of half the planes, which have fewer than 65536 slots each (shift 6): V and N bit for bit, and every entry of T
that is a vertex of the surface; the other entries must be the same entries with the same words on every step.  The step at the
second isovalue is compared with the reference like the rest.

The last test asserts what the whole module reached.  If the device reports another shape than tail_shapes.py predicts, the
case table changes, not the assertion."""
import math
import types

import numpy as np
import pytest

import emit_cases as ec
import layouts as lo
import tail_shapes as ts
from canaries import FRONT, canaried, only_the_rows_were_written, windows

pytestmark = pytest.mark.gpu

REACH = {"shifts": set(), "full": set(), "orders": set(), "partial_group": 0, "ghost_grouped": 0, "lanes_grouped": set(),
         "gate": set(), "forced": set(), "negzero": 0, "ids": 0}
IDS = len(ts.LIST_CASES) + len(ts.FORCED_SHAPES) + 4
_tensor, _refs = {}, {}


def device_tensor(case):
    """the grid on the device; the one before it is let go (a grid here has up to 73 M samples)"""
    if case.name not in _tensor:
        _tensor.clear()
        _tensor[case.name] = lo.to_device(np.ascontiguousarray(case.make()))
    return _tensor[case.name]


def reference(reflibs, case, iso):
    """the unmodified reference on the dense array, once per (case, isovalue) while the case is at work, never written"""
    key = (case.name, repr(iso))
    if key not in _refs:
        for k in [k for k in _refs if k[0] != case.name]:
            del _refs[k]
        s = reflibs[case.dtype].isosurface(case.make(), iso)
        for a in (s.V, s.N, s.T):
            a.setflags(write=False)
        _refs[key] = s
    return _refs[key]


def negzero(iso):
    return iso == 0.0 and math.copysign(1.0, iso) < 0.0


def check_rows(V, N, T, ref, what):
    """the canaried tensors against the reference; a NaN normal of the reference must be a NaN here (its payload is the
    device's own), everything else equal by bit pattern"""
    got = N[FRONT:FRONT + ref.V.shape[0]].cpu().numpy()
    nan = np.isnan(ref.N)
    assert np.array_equal(np.isnan(got), nan), what
    n = ref.N
    if nan.any():
        n = ref.N.copy()
        n[nan] = got[nan]
    only_the_rows_were_written(V, N, T, types.SimpleNamespace(V=ref.V, N=n, T=ref.T), what)


def check_shape(g, points, rng, what):
    """tail_shape() is what tail_shapes.tail() makes of the grid and the range"""
    sh = g.tail_shape()
    want = ts.tail(points, rng.z_begin, rng.z_end, rng.ghost_below)
    assert (sh.nslots, sh.groups, sh.shift, sh.scan_chunks, bool(sh.grouped), sh.slots_blocks) == \
        (want.nslots, want.groups, want.shift, want.nb, want.grouped, want.slots_blocks), (what, sh, want)
    return sh


def own_arrays(reflibs, case, iso):
    """iso = -0.0 on float samples: the library's own arrays from two z-slabs (contexts on windows of planes, the upper one with a
    ghost slice, emitted at the vertex base of the lower), each below 65536 slots - with the reference's number of vertices"""
    import torch
    from mc33_c_library_amd import DeviceGrid, Range
    key = (case.name, "own")
    if key not in _refs:
        t = device_tensor(case)
        nz = t.shape[0] - 1
        parts, vbase = [], 0
        for zb, ze in ((0, nz // 2), (nz // 2, nz)):
            ghost = 1 if zb else 0
            p_lo, p_hi = max(zb - ghost - 1, 0), min(ze + 1, nz)
            g = DeviceGrid(t[p_lo:p_hi + 1], nz_total=nz, plane0=p_lo)
            c = g.count(iso, Range(zb, ze, ghost, 0))
            V = torch.empty((c.nV + 1, 3), dtype=torch.float32, device="cuda")
            N, T = torch.empty_like(V), torch.empty((c.nT + 1, 3), dtype=torch.int32, device="cuda")
            g.emit_into(V, N, T, vbase)
            torch.cuda.synchronize()
            sh = g.tail_shape()
            assert sh.shift == 6 and sh.nslots < 65536, sh
            parts.append((V[:c.nV].cpu().numpy(), N[:c.nV].cpu().numpy(), T[:c.nT].cpu().numpy().view(np.uint32)))
            vbase += c.nV
            g.close()
        s = types.SimpleNamespace(V=np.concatenate([p[0] for p in parts]), N=np.concatenate([p[1] for p in parts]), T=np.concatenate([p[2] for p in parts]))
        s.nV, s.nT = s.V.shape[0], s.T.shape[0]
        assert s.nV == reference(reflibs, case, iso).nV and s.nT > 0
        _refs[key] = s
    return _refs[key]


def put_in_force(monkeypatch, shape):
    for k in ec.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in ec.SHAPES[shape].items():
        monkeypatch.setenv(k, v)


def extract_whole(g, ref, iso, what, loose=None):
    """loose (the -0.0 id: a list that collects T of every step): entries of T that are no vertex of the surface are not
    compared with ref, but must be the same on every step"""
    import torch
    V, N, T = canaried(ref.nV, ref.nT, False)
    cnt, ok = g.extract_into(iso, *windows(V, N, T, ref.nV, ref.nT))
    torch.cuda.synchronize()
    assert ok and (cnt.nV, cnt.nT) == (ref.nV, ref.nT), (what, cnt.nV, cnt.nT, ref.nV, ref.nT)
    if loose is not None:
        got = T[FRONT:FRONT + ref.nT].cpu().numpy().view(np.uint32)
        no_vertex = got >= ref.nV
        assert (ref.T[~no_vertex] < ref.nV).all() and 2 * int(no_vertex.sum()) < got.size, (what, int(no_vertex.sum()))
        t = ref.T.copy()
        t[no_vertex] = got[no_vertex]
        ref = types.SimpleNamespace(V=ref.V, N=ref.N, T=t)
        loose.append(got)
        assert np.array_equal(loose[0], got), what
    check_rows(V, N, T, ref, what)
    return cnt


def run_list(reflibs, monkeypatch, case, shape):
    from mc33_c_library_amd import DeviceGrid
    put_in_force(monkeypatch, shape)
    want = ts.tail(case.points)
    assert (want.shift, want.groups) == (case.shift, case.groups)
    own = case.dtype == "f32" and negzero(case.iso)
    if own:
        own_arrays(reflibs, case, case.iso)
    g = DeviceGrid(device_tensor(case))
    kernels, loose = [], []
    for step, iso in enumerate((case.iso, case.iso, case.iso2, case.iso)):
        what = (case.name, shape, step, iso)
        ref = own_arrays(reflibs, case, iso) if own and negzero(iso) else reference(reflibs, case, iso)
        cnt = extract_whole(g, ref, iso, what, loose if own and negzero(iso) else None)
        sh, em = check_shape(g, case.points, g.full_range(), what), g.emit_shape()
        assert (sh.shift, sh.groups) == (case.shift, case.groups), (what, sh)
        slow, dirty = g.list_counts()
        n = sh.groups
        assert int(slow.sum()) == sh.slow_total == em.slow_records and int(dirty.sum()) == sh.dirty_total, (what, sh, em, int(slow.sum()), int(dirty.sum()))
        assert not slow[n:].any() and not dirty[n:].any(), what
        if iso == case.iso:  # every group in use has work
            assert slow[:n].all() and dirty[:n].all(), (what, np.nonzero(slow[:n] == 0)[0][:8], np.nonzero(dirty[:n] == 0)[0][:8])
        else:                # no sample on the isovalue: nothing listed
            assert sh.slow_total == 0 and sh.dirty_total == 0, (what, sh)
        kernels.append(em.slow_kernel)
        print("%-20s %-13s step %d iso %-8r nV %7d nT %7d %s slow per group %d .. %d, dirty %d .. %d, slow kernel %d" % (
            case.name, shape, step, iso, cnt.nV, cnt.nT, tuple(sh), slow[:n].min(), slow[:n].max(), dirty[:n].min(), dirty[:n].max(), em.slow_kernel))
    g.close()
    REACH["shifts"].add(case.shift)
    if case.groups == ts.LIST_CHUNKS:
        REACH["full"].add(case.shift)
    REACH["gate"].add(tuple(kernels))
    if own:
        REACH["negzero"] += 1
    if shape != "default":
        REACH["forced"].add(shape)
    REACH["ids"] += 1


@pytest.mark.parametrize("case", [c.name for c in ts.LIST_CASES])
def test_list_groups(reflibs, monkeypatch, case):
    run_list(reflibs, monkeypatch, ts.LIST_BY_NAME[case], "default")


@pytest.mark.parametrize("shape", ts.FORCED_SHAPES)
def test_list_groups_at_forced_launch_shapes(reflibs, monkeypatch, shape):
    """a single block of the slow kernels (both emit kernels), a single block of k_cells: the grid-stride loops walk the group map
    of 513 groups of 256 slots many times"""
    run_list(reflibs, monkeypatch, ts.LIST_BY_NAME[ts.FORCED_CASE], shape)


def run_steps(reflibs, g, helper, case, steps, tag):
    """the steps on context g; helper: a second context on the same tensor, which counts what a step's range leaves out"""
    import torch
    from mc33_c_library_amd import Range
    nz = case.points[0] - 1
    flags = []
    for k, st in enumerate(steps):
        iso = case.iso2 if st.second else case.iso
        ref = reference(reflibs, case, iso)
        ze = nz if st.z_end is None else st.z_end
        rng = Range(st.z_begin, ze, st.ghost, 0)
        what = (case.name, tag, k, iso, (st.z_begin, ze, st.ghost))
        if st.z_begin == 0 and ze == nz:
            cnt = extract_whole(g, ref, iso, what)
        else:
            cnt = g.count(iso, rng)
            if st.z_begin == 0:   # the slices above, with their ghost slice
                rest = helper.count(iso, Range(ze, nz, 1, 0))
                vbase = tbase = 0
            else:                 # the slices below
                assert ze == nz
                rest = helper.count(iso, Range(0, st.z_begin, 0, 0))
                vbase, tbase = rest.nV, rest.nT
            assert (cnt.nV + rest.nV, cnt.nT + rest.nT) == (ref.nV, ref.nT), (what, cnt.nV, rest.nV, ref.nV, cnt.nT, rest.nT, ref.nT)
            V, N, T = canaried(cnt.nV, cnt.nT, False)
            g.emit_into(*windows(V, N, T, cnt.nV, cnt.nT), vbase)
            torch.cuda.synchronize()
            part = types.SimpleNamespace(V=ref.V[vbase:vbase + cnt.nV], N=ref.N[vbase:vbase + cnt.nV], T=ref.T[tbase:tbase + cnt.nT])
            check_rows(V, N, T, part, what)
        sh = check_shape(g, case.points, rng, what)
        assert (sh.scan_chunks, bool(sh.grouped)) == (st.nb, st.grouped), (what, sh)
        print("%-14s %-8s step %d iso %-8r range %5d .. %5d ghost %d nV %7d nT %7d ghost nV %3d %s" % (
            case.name, tag, k, iso, st.z_begin, ze, st.ghost, cnt.nV, cnt.nT, cnt.nV_ghost, tuple(sh)))
        flags.append(bool(sh.grouped))
        if sh.grouped and sh.scan_chunks % ts.SCAN_GROUP:
            REACH["partial_group"] += 1
        if sh.grouped and st.ghost:
            assert cnt.nV_ghost > 0, what  # (the ghost slice holds vertices: the scans start the numbering behind them)
            REACH["ghost_grouped"] += 1
    for a, b in zip(flags, flags[1:]):
        REACH["orders"].add((a, b))


def test_scans_grouped_ungrouped_ghost_on_one_context(reflibs):
    from mc33_c_library_amd import DeviceGrid
    case = ts.SCAN_A
    g, helper = DeviceGrid(device_tensor(case)), DeviceGrid(device_tensor(case))
    run_steps(reflibs, g, helper, case, ts.SEQUENCE, "sequence")
    g.close()
    helper.close()
    REACH["ids"] += 1


def test_scans_grow_from_a_short_range(reflibs):
    """Range(0, 100) first: the scan sums are reallocated for the whole grid, and the group sums lie in fresh memory"""
    from mc33_c_library_amd import DeviceGrid
    case = ts.SCAN_A
    g, helper = DeviceGrid(device_tensor(case)), DeviceGrid(device_tensor(case))
    run_steps(reflibs, g, helper, case, ts.GROW, "grow")
    g.close()
    helper.close()
    REACH["ids"] += 1


def test_scans_of_three_lanes(reflibs):
    """sweep_many over the whole grid and the three extractions (a tail each, behind a shared sweep); then prepare_many, which
    makes the tails ahead - two lanes in one launch and one in the next, blockIdx.y picks the lane's own group sums - and a
    count and an emit per isovalue, last isovalue first"""
    import torch
    from mc33_c_library_amd import DeviceGrid
    case = ts.SCAN_A
    g = DeviceGrid(device_tensor(case))
    g.sweep_many(list(ts.MANY_ISOS))
    for iso in ts.MANY_ISOS:
        what = (case.name, "sweep_many", iso)
        extract_whole(g, reference(reflibs, case, iso), iso, what)
        assert check_shape(g, case.points, g.full_range(), what).grouped
    g.prepare_many(list(ts.MANY_ISOS))
    for lane, iso in reversed(list(enumerate(ts.MANY_ISOS))):
        what = (case.name, "prepare_many", iso)
        ref = reference(reflibs, case, iso)
        cnt = g.count(iso)
        assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT), (what, cnt.nV, cnt.nT, ref.nV, ref.nT)
        V, N, T = canaried(ref.nV, ref.nT, False)
        g.emit_into(*windows(V, N, T, ref.nV, ref.nT))
        torch.cuda.synchronize()
        check_rows(V, N, T, ref, what)
        sh = check_shape(g, case.points, g.full_range(), what)
        assert sh.grouped
        print("%-14s prepare_many lane %d iso %-8r nV %7d nT %7d %s" % (case.name, lane, iso, cnt.nV, cnt.nT, tuple(sh)))
        REACH["lanes_grouped"].add(lane)
    g.close()
    REACH["ids"] += 1


def test_scans_with_chunk_boundaries_inside_a_slice(reflibs):
    """1998 rows: a chunk of 2048 row segments ends inside a slice's rows; 4195 chunks, the last group holds 3"""
    from mc33_c_library_amd import DeviceGrid
    case = ts.SCAN_B
    nb = ts.tail(case.points).nb
    assert nb % ts.SCAN_GROUP not in (0, 4)
    g = DeviceGrid(device_tensor(case))
    steps = [ts.Step(0, None, 0, second, nb, True) for second in (False, False, True, False)]
    run_steps(reflibs, g, None, case, steps, "rows1998")
    g.close()
    REACH["ids"] += 1


def test_the_module_reached_every_tail_shape():
    """Over all ids above (the whole module must have run): list groups at shifts 6, 7 and 8, all 1024 groups in use at two
    shifts; a step without slow cells between steps with them on every context; the forced launch shapes; grouped and ungrouped scans
    on one context in both orders; a partly filled last group; a ghost range under grouped scans; tails of several lanes with
    grouped scans."""
    print("shifts %s, 1024 groups at shifts %s\nslow kernels per step %s\nforced shapes %s, -0.0 ids %d\nscan orders (grouped before, after) %s\n"
          "partly filled last groups %d, ghost ranges under grouped scans %d, lanes with tails ahead %s" % (
              sorted(REACH["shifts"]), sorted(REACH["full"]), sorted(REACH["gate"]), sorted(REACH["forced"]), REACH["negzero"],
              sorted(REACH["orders"]), REACH["partial_group"], REACH["ghost_grouped"], sorted(REACH["lanes_grouped"])))
    assert REACH["ids"] == IDS, "run the whole module: %d of %d ids ran" % (REACH["ids"], IDS)
    assert REACH["shifts"] == {6, 7, 8} and REACH["full"] == {6, 7}
    assert REACH["forced"] == set(ts.FORCED_SHAPES) and REACH["negzero"] == 1
    assert all(k[0] != 2 and k[3] != 2 for k in REACH["gate"]), REACH["gate"]  # (slow cells there: the emit ran a slow kernel, whatever the step before had)
    assert {(True, False), (False, True), (True, True)} <= REACH["orders"], REACH["orders"]
    assert REACH["partial_group"] > 0 and REACH["ghost_grouped"] > 0
    assert REACH["lanes_grouped"] == {0, 1, 2}
    _tensor.clear()
    _refs.clear()
