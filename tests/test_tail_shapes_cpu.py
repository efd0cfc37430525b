"""The case tables of tests/tail_shapes.py reach what they claim - judged by the formulas, by the fixtures and by the reference's
output alone.  No GPU, no product library: a change of fixture that empties a list group or a scan chunk fails here.

List-group cases: the predicted (shift, groups); every list group holds a cell that is cut, is not on a face of the grid and has
a corner on the isovalue (a slow record and a dirty row segment for that group), computed from the samples; the reference
puts vertices on grid points at the first isovalue and none at the second (no slow cell: the alias gate closes).
Scan cases: the predicted (nb, grouped) of every step; every scan chunk holds a vertex and a triangle of the reference's
output; the caps."""
import numpy as np
import pytest

import emit_cases as ec
import tail_shapes as ts

_refs = {}


def reference(reflibs, case, iso):
    key = (case.name, repr(iso))
    if key not in _refs:
        s = reflibs[case.dtype].isosurface(case.make(), iso)
        for a in (s.V, s.N, s.T):
            a.setflags(write=False)
        _refs[key] = s
    return _refs[key]


def test_the_formulas_at_the_sizes_the_issue_names():
    # the grid with the most slots of the suite before: 2048 slices of 95 rows of 39 cells
    t = ts.tail((2049, 96, 40))
    assert (t.nslots, t.shift, t.groups, t.nb, t.grouped) == (4104, 6, 65, 95, False)
    # a cube of 1024 cells: shift 7, 547 groups, scans not grouped yet; 1024 x 2048 x 2048 cells: shift 9, grouped
    t = ts.tail((1025, 1025, 1025))
    assert (t.nslots, t.shift, t.groups, t.nb, t.grouped) == (69904, 7, 547, 2048, False)
    assert ts.tail((1025, 2049, 2049)).grouped and ts.tail((1025, 2049, 2049)).shift == 9
    # the four edges of the shift
    assert [ts.tail((p, 6, 6))[:3] for p in (65536, 65540, 131072, 131076)] == [(65536, 1024, 6), (65540, 513, 7), (131072, 1024, 7), (131076, 513, 8)]
    assert ts.tail((65533, 6, 6)).nslots == 65536 and ts.tail((65537, 6, 6)).nslots == 65540  # (the fewest planes of these slot counts)
    assert ts.tail((7, 5, 9)) == ts.Tail(8, 1, 6, 24, 1, False, 1, 0, 2, 1, 1, 6)
    assert ts.tail((7, 5, 9), 2, 5, 1).depth == 4 and ts.tail((7, 5, 9), 2, 5, 1).ghost_segs == 4


def slow_groups(case):
    """per list group: interior cells that are cut (a corner below and a corner above the isovalue) and have a corner on it"""
    f = case.make()
    iso = f.dtype.type(case.iso)
    t = ts.tail(case.points)

    def corners(a, op):
        for axis in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            a = op(a[tuple(lo)], a[tuple(hi)])
        return a
    slow = (corners(f, np.minimum) < iso) & (corners(f, np.maximum) > iso) & corners(f == iso, np.logical_or)
    z, y, x = np.nonzero(slow[1:-1, 1:-1, 1:-1])
    z, y, x = z + 1, y + 1, x + 1
    slot = ts.slice_slot(z, y // ts.Y_TILE, x // ts.SEG_CELLS, t)
    assert slot.max() < t.nslots
    return np.bincount(slot >> t.shift, minlength=ts.LIST_CHUNKS)


@pytest.mark.parametrize("name", [c.name for c in ts.LIST_CASES])
def test_list_case_reaches_every_group(reflibs, name):
    c = ts.LIST_BY_NAME[name]
    t = ts.tail(c.points)
    assert (t.shift, t.groups) == (c.shift, c.groups), t
    assert t.nslots > 65536 or t.shift == 6
    assert not t.grouped  # (the list cases stay below the scans' threshold: one thing at a time)
    per_group = slow_groups(c)
    assert (per_group[:t.groups] > 0).all(), np.nonzero(per_group[:t.groups] == 0)[0][:8]
    assert (per_group[t.groups:] == 0).all()
    assert per_group[:t.groups].min() != per_group[:t.groups].max()  # (the groups differ: a wrong group base moves a position)
    first, second = reference(reflibs, c, c.iso), reference(reflibs, c, c.iso2)
    on_point = lambda s: int((s.V == np.floor(s.V)).all(axis=1).sum())
    assert on_point(first) > t.groups and on_point(second) == 0 and second.nV > 0
    assert max(first.nV, second.nV) <= ts.VERTEX_CAP and max(first.nT, second.nT) <= 2 * ts.VERTEX_CAP
    print("%-20s slots %6d shift %d groups %4d slow cells per group %d .. %d, nV %d nT %d / nV %d nT %d" % (
        name, t.nslots, t.shift, t.groups, per_group[:t.groups].min(), per_group.max(), first.nV, first.nT, second.nV, second.nT))


def test_the_list_cases_cover_what_the_module_claims():
    shapes = {(c.shift, c.groups) for c in ts.LIST_CASES}
    assert {s for s, _ in shapes} == {6, 7, 8} and sum(1 for _, g in shapes if g == 1024) == 2
    assert {c.dtype for c in ts.LIST_CASES} == {"u8", "u16", "f32"}
    assert sum(1 for c in ts.LIST_CASES if c.iso == 0.0 and np.signbit(c.iso)) == 1
    long_axis = {int(np.argmax(c.points)) for c in ts.LIST_CASES}
    assert long_axis == {0, 1, 2}
    assert ts.tail(ts.Y_LONG).nYT == 64 and ts.tail(ts.X_LONG).nseg == 8193
    # one plane less on the x-long grid: the second z group would hold no slice off the top face
    assert ts.tail((ts.X_LONG[0] - 1,) + ts.X_LONG[1:]).depth - 2 < 4
    assert np.prod(ts.X_LONG) <= 75_000_000
    # the forced launch shapes are shapes of the emit tests, and set the switches of the slow kernels and of k_cells
    assert ts.FORCED_CASE in ts.LIST_BY_NAME and ts.LIST_BY_NAME[ts.FORCED_CASE].shift == 8
    assert set(ts.FORCED_SHAPES) <= set(ec.SHAPES)
    assert set().union(*[set(ec.SHAPES[s]) for s in ts.FORCED_SHAPES]) >= ts.FORCED_SWITCHES
    assert {ec.SHAPES[s].get("MC33_HIP_SLOW_SLOTS") for s in ts.FORCED_SHAPES} >= {"0", "1"}


def chunks_reached(case, s):
    """(vertices, triangles) per scan chunk that are there for sure.  A vertex inside a z edge (z not an integer) is made by slice
    floor(z); the row that counts it is y or y - 1: it is booked when both lie in one chunk.  A triangle belongs to the cell
    its centroid lies strictly inside."""
    t = ts.tail(case.points)
    ny = case.points[1] - 1
    V = s.V.astype(np.float64)  # (r0 = 0, d = 1: coordinates are grid indices, x first)
    fl = np.floor(V)
    on_z_edge = (V[:, 2] != fl[:, 2]) & (V[:, 0] == fl[:, 0]) & (V[:, 1] == fl[:, 1])
    z, y, x = fl[on_z_edge, 2].astype(np.int64), fl[on_z_edge, 1].astype(np.int64), fl[on_z_edge, 0].astype(np.int64)
    hi = ts.chunk_of_row(z, np.minimum(y, ny - 1), x // ts.SEG_CELLS, ny, t.nseg)
    lo = ts.chunk_of_row(z, np.maximum(y - 1, 0), x // ts.SEG_CELLS, ny, t.nseg)
    v = np.bincount(hi[hi == lo], minlength=t.nb)
    c = V[s.T.astype(np.int64)].mean(axis=1)
    inside = (c != np.floor(c)).all(axis=1)
    cz, cy, cx = (np.floor(c[inside, k]).astype(np.int64) for k in (2, 1, 0))
    tr = np.bincount(ts.chunk_of_row(cz, cy, cx // ts.SEG_CELLS, ny, t.nseg), minlength=t.nb)
    assert v.size == t.nb and tr.size == t.nb
    return v, tr


@pytest.mark.parametrize("name", [c.name for c in ts.SCAN_CASES])
def test_scan_case_fills_every_chunk(reflibs, name):
    c = ts.SCAN_BY_NAME[name]
    t = ts.tail(c.points)
    assert t.grouped and t.nseg == 1
    first, second = reference(reflibs, c, c.iso), reference(reflibs, c, c.iso2)
    v, tr = chunks_reached(c, first)
    assert (v > 0).all() and (tr > 0).all(), (np.nonzero(v == 0)[0][:8], np.nonzero(tr == 0)[0][:8])
    assert len(set(v.tolist())) > 2 and len(set(tr.tolist())) > 2  # (chunk sums differ from chunk to chunk)
    assert 0 < first.nV <= ts.VERTEX_CAP and first.nT <= 2 * ts.VERTEX_CAP
    assert 0 < 2 * second.nV < first.nV and 0 < 2 * second.nT < first.nT
    assert int((second.V == np.floor(second.V)).all(axis=1).sum()) > 0  # (the second isovalue lies on samples: slow cells under grouped scans)
    print("%-14s nb %d, vertices per chunk %d .. %d, triangles %d .. %d, nV %d nT %d / nV %d nT %d" % (
        name, t.nb, v.min(), v.max(), tr.min(), tr.max(), first.nV, first.nT, second.nV, second.nT))


def test_the_scan_sequences():
    a, b = ts.tail(ts.SCAN_A.points), ts.tail(ts.SCAN_B.points)
    assert ts.SCAN_A.points[1] - 1 == ts.SCAN_CHUNK and a.nb == a.depth == 4100  # a chunk is one slice's rows
    assert 4 <= ts.SCAN_A.points[2] <= 8
    for step in ts.SEQUENCE + ts.GROW:
        t = ts.tail(ts.SCAN_A.points, step.z_begin, step.z_end, step.ghost)
        assert (t.nb, t.grouped) == (step.nb, step.grouped), (step, t)
    s = ts.SEQUENCE
    assert s[0].nb % ts.SCAN_GROUP == 4 and not s[1].grouped and s[1].nb == ts.SCAN_GROUPED_FROM - 1
    assert s[2].nb == ts.SCAN_GROUPED_FROM and s[2].nb % ts.SCAN_GROUP == 0
    ghost = ts.tail(ts.SCAN_A.points, s[3].z_begin, s[3].z_end, s[3].ghost)
    assert ghost.grouped and ghost.ghost_segs and ghost.ghost_segs % ts.SCAN_CHUNK == 0
    assert s[4].second and not s[5].second and s[5][:3] == s[0][:3]
    assert not ts.GROW[0].grouped and ts.GROW[1].grouped
    assert len(ts.MANY_ISOS) == 3 and ts.MANY_ISOS[0] == ts.SCAN_A.iso and ts.MANY_ISOS[2] == ts.SCAN_A.iso2
    # the second shape: chunk boundaries inside a slice's rows, nb just above the threshold, a last group neither empty nor step 1's
    assert (ts.SCAN_B.points[1] - 1) % ts.SCAN_CHUNK and b.nsegs % ts.SCAN_CHUNK
    assert ts.SCAN_GROUPED_FROM < b.nb < ts.SCAN_GROUPED_FROM + 128 and b.nb % ts.SCAN_GROUP not in (0, 4)
