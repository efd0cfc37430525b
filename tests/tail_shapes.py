"""The shape of the tail of an extraction restated in plain Python, and the long thin grids that drive it across its thresholds.

From a grid shape (points, [z][y][x]) and a z range, tail() computes what slot_geometry, set_range (fill_params) and
enqueue_tail compute (mc33_extract.hip.h): the slice slots, the groups the slow-cell and dirty-segment lists are cut into
(ListChunks: at most 1024 groups of 2^shift slots, shift from 6 up), the row segments, the chunks of 2048 of them the prefix
sums go by, and whether those sums are grouped (from 4096 chunks on).  Both thresholds count slots and row segments, not
samples: a grid a few samples wide and tens of thousands of planes deep crosses them with a few megabytes.

The case tables below are shared by test_tail_shapes_cpu.py (the tables reach what they claim, judged by the formulas and by
the reference's output alone) and test_gpu_tail_shapes.py (the device against the reference on these grids, and
DeviceGrid.tail_shape() against tail()).  Nothing here looks at the library."""
import collections
import functools

import numpy as np

SEG_CELLS, Y_TILE = 256, 63          # cells of a row segment, rows of a y tile
LIST_CHUNKS, FIRST_SHIFT = 1024, 6   # groups of the slow / dirty lists at most; log2 of the slots of a group at least
SLOT_CHUNK = 512                     # slots per block of k_slots
SCAN_CHUNK, SCAN_GROUP, SCAN_GROUPED_FROM = 2048, 32, 4096

NP = {"f32": np.float32, "u8": np.uint8, "u16": np.uint16}

Tail = collections.namedtuple("Tail", "nslots groups shift nsegs nb grouped slots_blocks ghost_segs nZG nYT nseg depth")


def ceil_div(a, b):
    return (a + b - 1) // b


def tail(points, z_begin=0, z_end=None, ghost_below=0):
    """the tail of an extraction over slices [z_begin, z_end) (with the slice below z_begin when ghost_below) of a grid of
    `points` = (npz, npy, npx) samples"""
    npz, npy, npx = (int(n) for n in points)
    nx, ny, nz = npx - 1, npy - 1, npz - 1
    z_end = nz if z_end is None else int(z_end)
    zs = z_begin - (1 if ghost_below else 0)
    assert 0 <= zs < z_end <= nz
    depth = z_end - zs
    nseg = ceil_div(nx, SEG_CELLS)
    nYT = (ny + Y_TILE - 1) // Y_TILE
    nZG = (depth + 4) // 4            # planes, one more than slices, in groups of 4
    nslots = 4 * nZG * nYT * nseg
    shift = FIRST_SHIFT
    while ceil_div(nslots, 1 << shift) > LIST_CHUNKS:
        shift += 1
    nsegs = depth * ny * nseg
    nb = ceil_div(nsegs, SCAN_CHUNK)
    return Tail(nslots, ceil_div(nslots, 1 << shift), shift, nsegs, nb, nb >= SCAN_GROUPED_FROM, ceil_div(nslots, SLOT_CHUNK),
                ny * nseg if ghost_below else 0, nZG, nYT, nseg, depth)


def slice_slot(dz, yt, seg, t):
    """slice_slot of mc33_records.hip.h: the slot of cell slice dz (counted from the range's first), y tile yt, row segment seg"""
    return ((((dz >> 2) * t.nYT + yt) * t.nseg + seg) << 2) | (dz & 3)


def planes_for_zgroups(nZG):
    """the most planes whose slices and top plane fill nZG groups of four: the last slot of the last group holds a plane, so the
    slots before it in that group hold slices"""
    return 4 * nZG


# ---- the fields: tubes with a diamond cross-section ----------------------------------------------------------------------
# Along the tube axis t the cross-section is the diamond |a - a0(t)| + |b - b0(t)| <= r(t); the sample is r - distance, an integer,
# clipped to [-CLIP, CLIP].  Samples next to each other in a plane differ by one, so at an integer level every cell the surface
# cuts has a corner ON the level (a slow record), and at a level + 0.5 none has.  r, a0, b0 repeat every 8 planes: the surface
# crosses other rows in every plane.
R8 = (1, 2, 2, 1, 2, 1, 1, 2)
A8 = (2, 2, 3, 3, 2, 3, 2, 3)
B8 = (2, 3, 3, 2, 2, 2, 3, 3)
R12 = (1, 3, 2, 3, 1, 2, 2, 1, 3, 1, 2, 3)  # (the scan grids: three radii, so that a high level leaves a third of the planes)


def tubes(points, a_axis, b_axis, a_period=None, radii=R8, clip=2, a_shift=0, a_drift=0):
    """int16 [z][y][x]: tubes along z; the cross-section lies in (a_axis, b_axis), repeated along a_axis every a_period samples
    (None: one tube), its a centre moved by a_shift, and by a_drift * (z % 97) more (the scan grids: other rows in every slice)"""
    z = np.arange(points[0])

    def along(axis, v):
        s = [1, 1, 1]
        s[axis] = -1
        return np.asarray(v).astype(np.int16).reshape(s)
    r = along(0, np.take(radii, z % len(radii)))
    a0 = along(0, np.take(A8, z % 8) + a_shift + a_drift * (z % 97))
    b0 = along(0, np.take(B8, z % 8))
    a = np.arange(points[a_axis])
    if a_period:
        a = a % a_period
    assert a.max() < 32000 and int(a0.max()) < 32000
    dist = np.abs(along(a_axis, a) - a0) + np.abs(along(b_axis, np.arange(points[b_axis])) - b0)
    return np.ascontiguousarray(np.broadcast_to(np.clip(r - dist, -clip, clip), points))


LEVEL = {"u8": 100, "u16": 30000, "f32": 0}


def as_samples(field, dtype):
    return (field + LEVEL[dtype]).astype(NP[dtype])


# ---- list-group cases ------------------------------------------------------------------------------------------------------
# name, sample type, points, () -> samples, isovalue (on samples all along the surface), second isovalue (on no sample), and
# what tail(points) must give: (shift, groups)
ListCase = collections.namedtuple("ListCase", "name dtype points make iso iso2 shift groups")


@functools.lru_cache(maxsize=2)
def _make_cached(points, dtype, kw):
    return as_samples(tubes(points, **dict(kw)), dtype)


def _make(points, dtype, kw):
    return _make_cached(points, dtype, tuple(sorted(kw.items())))


# y-long: 64 y tiles and just enough z groups for more than 65536 slots; a tube every 64 rows, so every y tile of every z group
# holds one (a list group is 32 y tiles of one z group: it cuts through the [zg][yt] order)
Y_LONG = (planes_for_zgroups(257), 63 * 63 + 2 + 4, 6)
# x-long: 4 rows of cells, 8193 row segments, two z groups (the second must hold a slice that is not on the top face: 7 planes
# at least); a tube in every row segment
X_LONG = (7, 5, SEG_CELLS * 8193 + 1)


def _list_cases():
    out = []

    def add(name, dtype, points, kw, iso_off, shift, groups):
        level = LEVEL[dtype]
        iso = -0.0 if iso_off == "negzero" else float(level)
        out.append(ListCase(name, dtype, points, functools.partial(_make, points, dtype, kw), iso, level + 0.5, shift, groups))
    zkw = dict(a_axis=1, b_axis=2)
    for nZG, shift, groups in ((16384, 6, 1024), (16385, 7, 513), (32768, 7, 1024), (32769, 8, 513)):
        add("z%d-u8" % (4 * nZG), "u8", (planes_for_zgroups(nZG), 6, 6), zkw, 0, shift, groups)
    add("z65540-f32", "f32", (planes_for_zgroups(16385), 6, 6), zkw, 0, 7, 513)
    add("z65540-f32-negzero", "f32", (planes_for_zgroups(16385), 6, 6), zkw, "negzero", 7, 513)
    add("z131072-u16", "u16", (planes_for_zgroups(32768), 6, 6), zkw, 0, 7, 1024)
    add("y-long-u8", "u8", Y_LONG, dict(a_axis=1, b_axis=2, a_period=64), 0, 7, 514)
    add("x-long-u8", "u8", X_LONG, dict(a_axis=2, b_axis=1, a_period=SEG_CELLS, a_shift=120), 0, 7, 513)
    return out


LIST_CASES = _list_cases()
LIST_BY_NAME = {c.name: c for c in LIST_CASES}
# the launch shapes of tests/emit_cases.py (SHAPES) that touch the slow kernels and k_cells, run on this case as well: there the
# grid-stride loops walk the group map many times
FORCED_CASE = "z131076-u8"
FORCED_SHAPES = ("slow1-thread", "slow1-slots", "narrow-vfirst")
FORCED_SWITCHES = {"MC33_HIP_SLOW_BLOCKS", "MC33_HIP_SLOW_SLOTS", "MC33_HIP_CELLS_BLOCKS"}


# ---- scan cases --------------------------------------------------------------------------------------------------------------
# name, sample type, points, () -> samples, isovalue (every slice cut, no sample on it), second isovalue (an integer: samples on
# it, and less than half the vertices)
ScanCase = collections.namedtuple("ScanCase", "name dtype points make iso iso2")
VERTEX_CAP = 2_000_000

# 2048 rows, one row segment: a chunk is one slice's rows, nb is the depth.  The tube drifts over the rows with z.
SCAN_A = ScanCase("rows2048-u8", "u8", (4101, 2049, 5),
                  functools.partial(_make, (4101, 2049, 5), "u8", dict(a_axis=1, b_axis=2, radii=R12, clip=3, a_shift=6, a_drift=20)), 100.5, 102.0)
# 1998 rows: chunk boundaries fall inside a slice's rows; a tube every 256 rows, so every run of 2048 row segments holds several -
# and the last chunk, the last 90 rows of the top slice, one (a_shift)
SCAN_B = ScanCase("rows1998-u16", "u16", (4300, 1999, 6),
                  functools.partial(_make, (4300, 1999, 6), "u16", dict(a_axis=1, b_axis=2, radii=R12, clip=3, a_period=256, a_shift=150)), 30000.5, 30002.0)
SCAN_CASES = (SCAN_A, SCAN_B)
SCAN_BY_NAME = {c.name: c for c in SCAN_CASES}

# The sequence one context runs on SCAN_A: (z_begin, z_end - None: the top -, ghost_below, which isovalue, nb, grouped)
Step = collections.namedtuple("Step", "z_begin z_end ghost second nb grouped")
SEQUENCE = (
    Step(0, None, 0, False, 4100, True),   # the whole grid: 128 full groups and one of 4 chunks
    Step(0, 4095, 0, False, 4095, False),  # ungrouped, step 1's group sums still in place
    Step(0, 4096, 0, False, 4096, True),   # exactly 128 full groups
    Step(2, 4100, 1, False, 4099, True),   # a ghost slice: ghost_segs = 2048 falls on a chunk boundary
    Step(0, None, 0, True, 4100, True),    # counts less than half
    Step(0, None, 0, False, 4100, True),
)
GROW = (Step(0, 100, 0, False, 100, False), Step(0, None, 0, False, 4100, True))  # the scan sums are reallocated in between
MANY_ISOS = (100.5, 101.5, 102.0)  # sweep_many over SCAN_A: three lanes, each tail set its own group sums


def chunk_of_row(z, y, seg, ny, nseg, z0=0):
    """the scan chunk of row segment (slice z, row y, segment seg) of a range that starts at slice z0: the order is [z][y][segment]"""
    return (((z - z0) * ny + y) * nseg + seg) // SCAN_CHUNK
