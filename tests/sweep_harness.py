"""What the GPU tests of the sweep with a range table share (tests/test_gpu_range_skip.py, test_gpu_sweep_refill.py,
test_gpu_sweep_pack.py, test_gpu_range_blocks.py, test_gpu_sweep_balance.py, test_gpu_block_batches.py, and the sequences of
tests/sweep_plan_sequences.py): shapes and isovalues, fields, arrays to the device and surfaces compared as bits, readers of the
library's developer entry points, the numpy restatements that are in none of sweep_pack_rules.py, sweep_plan_rules.py and
range_blocks_rules.py, the checks built from them, the fixtures, and ONE statement of the case of two z-slabs.

Every surface is compared with the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit: counts, T as uint32,
V and N by bit pattern (a NaN must be a NaN in the same place).  There is no tolerance in this file.

A test module imports what it uses by name, fixtures included: an autouse fixture is in force in the modules that import it and
in no other."""
import ctypes as C
import warnings

import numpy as np
import pytest

import range_blocks_rules as br
import sweep_pack_rules as pr
import sweep_plan_rules as sp

# ---- shapes (points z, y, x) and isovalues ----------------------------------------------------------------------------------------------

NP = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
REAL = {"f32": np.float32, "f64": np.float64, "u8": np.float32, "u16": np.float32, "u32": np.float32}
A, B, BIG, SHALLOW = (48, 200, 520), (40, 70, 1030), (160, 130, 1030), (12, 130, 1030)
C3 = (24, 130, 300)
MIXED = (56, 70, 1030)
DEPTHS = (1, 2, 16)
EINVAL = -1
STEEP_ISO = {A: 1840.0, B: 1930.5, BIG: 2600.5, SHALLOW: 2600.5}
MANY = {("f32", A): (1840.0, 300.5, 2400.0, 1200.25), ("u8", A): (100.5, 20.5, 180.5, 60.5), ("u16", A): (500.5, 100.5, 900.5, 700.5),
        # shape B: inside the group of four segments, segment 0 lies below all four isovalues, segment 3 above, 1 and 2 are cut
        ("f32", B): (1930.5, 1700.5, 2100.25, 1800.0), ("u16", B): (600.5, 560.5, 700.5, 650.5)}
LOW = (100.5, 50.5, 150.25, 200.0, 20.5, 120.75, 180.5, 220.0)   # isovalues of banded() with three tiles in four live
HIGH = 1100.5                                                      # ... and with one in four


# ---- fields ----------------------------------------------------------------------------------------------------------------------------

def ramp(shape, cx=1, cy=2, cz=3, off=0):
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return cx * x + cy * y + cz * z + off  # int64


def strips(shape):
    """(yt, seg, rows, columns) of every strip of a plane: both ends inclusive"""
    ny, nx = shape[1] - 1, shape[2] - 1
    for yt in range((ny + 62) // 63):
        for seg in range((nx + 255) // 256):
            yield yt, seg, slice(63 * yt, min(63 * yt + 63, ny) + 1), slice(256 * seg, min(256 * seg + 256, nx) + 1)


def steep(shape):
    """a steep ramp: whole columns of tiles on one side"""
    return ramp(shape, 3, 5, 1).astype(np.float32)


def typed_ramp(dtype, shape):
    """integer-valued ramps, for isovalues on the strips' own ends"""
    r = ramp(shape)
    if dtype == "u8":
        return (r // 5).astype(np.uint8)        # 0 .. 211
    if dtype == "u32":
        return (r * 4000000 + 77).astype(np.uint32)  # up to 4.2e9: (float)F is not one to one
    return r.astype(NP[dtype])


def typed(dtype, shape):
    r = ramp(shape, 3, 5, 1)
    return (r // 16).astype(np.uint8) if dtype == "u8" else r.astype(NP[dtype])


def ramp_isos(dtype, data):
    """of the strip (plane 20, y tile 1, segment 1): exactly its minimum, exactly its maximum - which is its halo-column sample of the
    row it shares with the next y tile - and half-integers beside both"""
    t = numpy_table(data, dtype)
    lo, hi = float(t[20, 1, 1, 0]), float(t[20, 1, 1, 1])
    assert hi == float(REAL[dtype](data[20, min(126, data.shape[1] - 1), 512]))
    half = 0.5 if dtype != "u32" else 2000000.0
    return (lo, hi, lo + half, hi - half)


def live_everywhere(shape):
    """every strip straddles 100.5 and few cells are cut: x mod 256 in the whole segments, 50 (x - 1024) in the narrow last one"""
    x = np.arange(shape[2])
    row = np.where(x < 1024, x % 256, 50 * (x - 1024)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(row, shape))


def banded(z0=120):
    """BIG: every strip of the planes below z0 straddles 100.5 (x mod 256; 50 (x - 1024) in the narrow last segment), every strip
    from z0 on straddles 1100.5, and few cells are cut: z0 / 160 of the tiles live for isovalues below 256 (three in four at 120),
    the others for isovalues between 1000 and 1256"""
    data = live_everywhere(BIG).copy()
    data[z0:] += 1000.0
    return data


def one_bump():
    data = np.zeros(B, np.float32)
    data[20, 20:24, 100:104] = 1.0
    return data


def mixed_field():
    """shape B, y tile 0: below 0.5 everywhere, but for one cell-sized bump per chosen (segment, plane) - planes 1 .. 12: segment 0
    only (three waves of the group of four dead), 14 .. 25: segments 0 and 2 (two), 27 .. 38: segments 0, 1 and 3 (one).  A block of
    the sweep is any four consecutive tiles of the plan, and with the fifth segment in between only every fourth z level's block is
    the group itself: every band is longer than that period at tiles two planes deep.  The bumps are 1.0, but for 3.0 in segment
    0, planes 4 .. 7 - the only thing above 2.5: every other tile with a bump is dead for 2.5 and live for 0.5."""
    data = np.zeros(B, np.float32)
    for planes, segs in ((range(1, 13), (0,)), (range(14, 26), (0, 2)), (range(27, 39), (0, 1, 3))):
        for p in planes:
            for s in segs:
                data[p, 20:24, 256 * s + 100:256 * s + 104] = 3.0 if (s == 0 and 4 <= p <= 7) else 1.0
    return data


def mixed_whole():
    """mixed_field on a grid 16 planes taller, with a fourth band: y tile 0 below 0.5 everywhere but
    for one cell-sized bump per chosen (segment, plane) - planes 1 .. 12: segment 0 only (three waves of the group of four dead),
    14 .. 25: segments 0 and 2 (two), 27 .. 38: segments 0, 1 and 3 (one), 40 .. 51: all four (a whole group)"""
    data = np.zeros(MIXED, np.float32)
    for planes, segs in ((range(1, 13), (0,)), (range(14, 26), (0, 2)), (range(27, 39), (0, 1, 3)), (range(40, 52), (0, 1, 2, 3))):
        for p in planes:
            for sg in segs:
                data[p, 20:24, 256 * sg + 100:256 * sg + 104] = 1.0
    return data


# ---- to the device, and surfaces as bits ------------------------------------------------------------------------------------------------

def to_device(a):
    import torch
    v = a.view(np.int16) if a.dtype == np.uint16 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def grid_of(t, **kw):
    from mc33_c_library_amd import DeviceGrid
    return DeviceGrid(t, **kw)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same(got, ref, what):
    V, N, T, cnt = got
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT), what
    v, n, t = V.cpu().numpy(), N.cpu().numpy(), T.cpu().numpy().view(np.uint32)
    assert v.dtype == ref.V.dtype and v.shape == ref.V.shape and n.shape == ref.N.shape, what
    assert np.array_equal(t, ref.T), what
    # (a NaN of the surface - a vertex interpolated from a NaN or infinite sample - is a NaN in the same place; which NaN is not
    # defined, as everywhere in this suite: tests/test_gpu_parity.py, test_gpu_sweep_halo.py)
    bad = []
    for x, y in ((v, ref.V), (n, ref.N)):
        assert np.array_equal(np.isnan(x), np.isnan(y)), what
        bad.append(int(np.count_nonzero((words(x) != words(y)) & ~np.isnan(y))))
    assert bad == [0, 0], "%s: %d position words, %d normal words differ" % (what, bad[0], bad[1])


def same_arrays(got, want, what):
    (V, N, T, cnt), (V2, N2, T2, cnt2) = got, want
    assert (cnt.nV, cnt.nT) == (cnt2.nV, cnt2.nT), what
    for x, y in ((V, V2), (N, N2), (T, T2)):
        assert np.array_equal(words(x.cpu().numpy()), words(y.cpu().numpy())), what


_refs = {}


def reference(reflibs, key, dtype, data, iso):
    """the reference's surface, computed once per (key, dtype, isovalue) for all the modules that import this"""
    k = (key, dtype, repr(float(iso)))
    if k not in _refs:
        _refs[k] = reflibs[dtype].isosurface(data, iso)
    return _refs[k]


# ---- readers of the developer entry points (include/mc33_hip.h; their argtypes: mc33_c_library_amd/api.py) -----------------------------

def table_of(g, dtype):
    """the library's table, or None when it has none (EINVAL)"""
    a = g.tensor
    t = np.empty((a.shape[0], (a.shape[1] - 1 + 62) // 63, (g.desc.npx - 1 + 255) // 256, 2), REAL[dtype])
    rc = g.lib.mc33hip_range_table(g.ctx, C.c_void_p(t.ctypes.data), t.nbytes)
    assert rc in (0, EINVAL), rc
    return t if rc == 0 else None


def skipped(g):
    out = (C.c_ulonglong * 3)()
    assert g.lib.mc33hip_sweep_skipped(g.ctx, C.byref(out)) == 0
    return tuple(out)


def plan_of(g):
    """(tiles [n][4] = seg, yt, z_lo, z_hi in launch order, blocks the device holds at once, which plan: 0 without a table, 1 with)"""
    info = (C.c_ulonglong * 3)()
    assert g.lib.mc33hip_sweep_plan(g.ctx, None, 0, C.byref(info)) == 0
    t = np.zeros((int(info[0]), 4), np.uint32)
    assert g.lib.mc33hip_sweep_plan(g.ctx, C.c_void_p(t.ctypes.data), t.shape[0], C.byref(info)) == 0
    return t, int(info[1]), int(info[2])


def weight_of(g):
    w = C.c_double(-1.0)
    assert g.lib.mc33hip_sweep_plan_weight(g.ctx, C.byref(w)) == 0
    return w.value


def live_of(g):
    """(entries, count word, blocks of the plan) of the last sweep with a table"""
    info = (C.c_ulonglong * 2)()
    assert g.lib.mc33hip_sweep_live(g.ctx, None, 0, C.byref(info)) == 0
    e = np.zeros(max(int(info[1]), 1), np.uint32)
    assert g.lib.mc33hip_sweep_live(g.ctx, C.c_void_p(e.ctypes.data), e.shape[0], C.byref(info)) == 0
    return e[:int(info[0])], int(info[0]), int(info[1])


def packed_of(g):
    """(entries [n][4], live tiles, tiles of the plan) of the last sweep with a table"""
    info = (C.c_ulonglong * 3)()
    assert g.lib.mc33hip_sweep_packed(g.ctx, None, 0, C.byref(info)) == 0
    e = np.zeros((max(int(info[0]), 1), 4), np.uint32)
    assert g.lib.mc33hip_sweep_packed(g.ctx, C.c_void_p(e.ctypes.data), e.shape[0], C.byref(info)) == 0
    return e[:int(info[0])], int(info[1]), int(info[2])


def blocks_of(g, dtype):
    a = g.tensor
    nyt, nseg = br.dims((a.shape[0], a.shape[1], g.desc.npx))
    t = np.empty((a.shape[0], nyt, nseg, br.BLOCKS, 2), REAL[dtype])
    rc = g.lib.mc33hip_range_blocks(g.ctx, C.c_void_p(t.ctypes.data), t.nbytes)
    assert rc in (0, EINVAL), rc
    return t if rc == 0 else None


def words_of(g):
    a = g.tensor
    nyt, nseg = br.dims((a.shape[0], a.shape[1], g.desc.npx))
    w = np.empty((a.shape[0], nyt, nseg), np.uint64)
    assert g.lib.mc33hip_block_words(g.ctx, C.c_void_p(w.ctypes.data), w.nbytes) == 0
    return w


def left_out(g):
    out = (C.c_ulonglong * 3)()
    assert g.lib.mc33hip_sweep_skipped_blocks(g.ctx, C.byref(out)) == 0
    return tuple(int(x) for x in out)


def alias_cells(g):
    out = C.c_ulonglong(0)
    assert g.lib.mc33hip_alias_cells(g.ctx, C.byref(out)) == 0
    return int(out.value)


# ---- numpy's own table, verdicts, live list and plan ------------------------------------------------------------------------------------

def numpy_table(a, dtype):
    """[plane][yt][seg]{min, max} of the samples converted to MC33_real; {-inf, +inf} where a strip holds a NaN"""
    r = a.astype(REAL[dtype])
    nyt, nseg = (a.shape[1] - 1 + 62) // 63, (a.shape[2] - 1 + 255) // 256
    t = np.empty((a.shape[0], nyt, nseg, 2), REAL[dtype])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for yt, seg, ys, xs in strips(a.shape):
            blk = r[:, ys, xs].reshape(a.shape[0], -1)
            bad = np.isnan(blk).any(axis=1)
            t[:, yt, seg, 0] = np.where(bad, -np.inf, np.nanmin(blk, axis=1))
            t[:, yt, seg, 1] = np.where(bad, np.inf, np.nanmax(blk, axis=1))
    return t


def dead_columns(data, iso, dtype="f32"):
    """(columns all of whose strips lie below the isovalue, above it, columns in all) - from numpy alone"""
    t = numpy_table(data, dtype)
    below, above = (t[..., 1] < iso).all(axis=0), (t[..., 0] > iso).all(axis=0)
    return int(below.sum()), int(above.sum()), below.size


def planned_tiles(shape, depth):
    """{(yt, seg): tiles} - a lower bound of the tiles plan_tiles (mc33_sweep_plan.h) cuts every column into, restated from its
    arithmetic for float samples (batches of 4 sample rows) with MC33_HIP_RZ = MC33_HIP_MIN_DEPTH = depth, on a grid so small that
    what the device holds at once does not cap the plan: the work of a wave per slice is its sample rows in whole batches, the
    plan wants B = W nzc / (64 depth) tiles, and a group of segments gets floor(B w / W) z pieces (one at least, a slice each at
    most); the remainder goes to the groups with the largest fractions, one piece more each - not counted here."""
    ny, nx, nzc = shape[1] - 1, shape[2] - 1, shape[0] - 1
    nseg, nyt = (nx + 255) // 256, (ny + 62) // 63
    groups = [(yt, xg, min(4, nseg - 4 * xg), (min(64, ny + 1 - 63 * yt) + 3) // 4 * 4) for yt in range(nyt) for xg in range((nseg + 3) // 4)]
    W = float(sum(w * waves for _, _, waves, w in groups))
    Bt = max(1, int(W * nzc / (64.0 * depth)))
    assert Bt < 1024  # (far below the wave slots of any device this runs on)
    out = {}
    for yt, xg, waves, w in groups:
        n = int(min(max(1.0, np.floor(Bt * w / W)), nzc))
        for seg in range(4 * xg, 4 * xg + waves):
            out[(yt, seg)] = n
    return out


def numpy_verdicts(tiles, tab, isos, zs=0, plane0=0):
    """per tile: (dead for every isovalue, below the FIRST isovalue, above it) - the planes a tile would read are z_lo + 1 .. z_hi, and
    z_lo too in the lowest tile of a column; both comparisons strict"""
    dead, below, above = np.zeros(len(tiles), bool), np.zeros(len(tiles), bool), np.zeros(len(tiles), bool)
    for i, (seg, yt, z_lo, z_hi) in enumerate(tiles.tolist()):
        p0 = z_lo if z_lo == zs else z_lo + 1
        s = tab[p0 - plane0:z_hi + 1 - plane0, yt, seg]
        lo = [bool((s[:, 1] < iso).all()) for iso in isos]
        hi = [bool((s[:, 0] > iso).all()) for iso in isos]
        dead[i] = all(x or y for x, y in zip(lo, hi))
        below[i], above[i] = dead[i] and lo[0], dead[i] and hi[0] and not lo[0]
    return dead, below, above


def expected_live(dead):
    """the live list of a plan whose tiles have these verdicts: a word per block with a live tile, in plan order"""
    n = len(dead)
    out = []
    for b in range((n + 3) // 4):
        mask = sum(1 << k for k in range(4) if 4 * b + k >= n or dead[4 * b + k])
        if mask != 15:
            out.append(b << 4 | mask)
    return np.array(out, np.uint32)


def live_mask(g, data, iso, zs=0, plane0=0):
    """the strips the live tiles of the plan in force read, from numpy's own verdicts"""
    tiles = plan_of(g)[0]
    dead = numpy_verdicts(tiles, numpy_table(data, "f32"), (iso,), zs, plane0)[0]
    nyt, nseg = br.dims(data.shape)
    return br.live_strips(tiles, dead, data.shape[0], nyt, nseg, zs, plane0)


# ---- checks ----------------------------------------------------------------------------------------------------------------------------

def four_runs(monkeypatch, make, isos, refs, dtype, data, what):
    """first extraction (no table), second (built and used), third (kept), and a context that never builds one"""
    g = make()
    assert table_of(g, dtype) is None
    for rep in range(3):
        for iso, ref in zip(isos, refs):
            same(g.extract(iso), ref, (what, iso, "extraction %d" % (rep + 1)))
        if rep == 0 and len(isos) == 1:
            assert table_of(g, dtype) is None, "a table after ONE sweep"
    t = table_of(g, dtype)
    assert t is not None
    assert np.array_equal(words(t), words(numpy_table(data, dtype))), (what, "the table differs from numpy's")
    g.close()
    monkeypatch.setenv("MC33_HIP_RANGES", "0")
    g = make()
    for rep in range(2):
        for iso, ref in zip(isos, refs):
            same(g.extract(iso), ref, (what, iso, "MC33_HIP_RANGES=0"))
    assert table_of(g, dtype) is None
    g.close()
    monkeypatch.delenv("MC33_HIP_RANGES")


def check_live(g, tab, isos, what, zs=0, plane0=0):
    tiles, resident, which = plan_of(g)
    dead, below, above = numpy_verdicts(tiles, tab, isos, zs, plane0)
    want = expected_live(dead)
    got, count, blocks = live_of(g)
    assert blocks == (len(tiles) + 3) // 4, what
    assert count == len(want) and np.array_equal(got, want), (what, "live list", count, len(want))
    return tiles, dead, below, above


def check_packed(g, tab, isos, what, zs=0, plane0=0):
    tiles, resident, which = plan_of(g)
    dead = numpy_verdicts(tiles, tab, isos, zs, plane0)[0]
    grouped = pr.grouped_blocks(tiles)
    want = pr.packed_entries(dead, grouped)
    got, live, ntiles = packed_of(g)
    assert ntiles == len(tiles) and live == int((~dead).sum()) and len(got) == (live + 3) // 4, (what, ntiles, live)
    pr.check_entries(got, dead)
    assert np.array_equal(got, want), (what, "packed list")
    return tiles, dead, grouped, got


def by_the_rule(g, what):
    """the plan in force is the finer one, and the packed blocks of the last sweep lie inside the band of the rule - or the plan is
    as fine as the rule's smallest depth allows (the chunks of a plan add up to a few tiles more or less than were asked for)"""
    tiles, resident, which = plan_of(g)
    e, live, ntiles = packed_of(g)
    assert which == 1 and ntiles == len(tiles) and len(e) == (live + 3) // 4, what
    unit = pr.unit_of(BIG)
    depth = pr.floor_depth(unit, resident)
    assert depth is not None, (what, "BIG is less than one round of this device", resident)
    cap = int(unit / depth)
    print("%s: %d tiles, %d live, %d packed blocks of %d resident (%.2f); cap %d" % (what, ntiles, live, len(e), resident, len(e) / resident, cap))
    one_round = abs(ntiles - 4 * resident) <= 8 and len(e) > pr.BAND_HI * resident   # (more than the fill live: one round, never less)
    assert pr.keeps(live, resident) or abs(ntiles - cap) <= 8 or one_round, (what, ntiles, live, resident, cap)
    return ntiles


def check_plan(g, shape, what, asked=None):
    """the plan in force is the share rule's with the weight the library reports: chunks per column for the target `asked` - or,
    where only the fill rule knows the target, for some target no more than a block of waves per column below the tiles there
    are - and every column cut into that many pieces of planes as equal as whole planes allow.  Returns (weight, chunks)."""
    tiles, resident, which = plan_of(g)
    weight = weight_of(g)
    t = tiles.astype(np.int64)
    zs, ze = int(t[:, 2].min()), int(t[:, 3].max())
    nzc = ze - zs
    cols = sp.columns(shape)
    chunks = sp.plan_chunks(tiles, shape)
    assert sum(c * col[2] for c, col in zip(chunks, cols)) == len(tiles), what
    for (yt, xg, waves, _), n in zip(cols, chunks):
        for seg in range(4 * xg, 4 * xg + waves):
            mine = t[(t[:, 0] == seg) & (t[:, 1] == yt)]
            mine = mine[np.argsort(mine[:, 2])]
            k = np.arange(n)
            assert np.array_equal(mine[:, 2], zs + nzc * k // n) and np.array_equal(mine[:, 3], zs + nzc * (k + 1) // n), (what, yt, seg)
    fits = []
    for target in ([asked] if asked else range(max(1, len(tiles) - 4 * len(cols)), len(tiles) + 1)):
        try:
            sp.check_chunks(chunks, cols, target, nzc, weight, unit=4.0)
            fits.append(target)
        except AssertionError:
            pass
    assert fits, (what, "the plan is not the share rule's", weight, chunks)
    return weight, chunks


# ---- fixtures: a test module imports the ones it wants by name --------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def live_list_always(monkeypatch):
    """by itself a sweep goes by a live list only under a plan of at least one round of the device (test_who_gets_a_live_list of
    tests/test_gpu_sweep_refill.py); the grids of these tests are small, and MC33_HIP_LIVE=1, read when a context is made, gives
    every sweep with a table one"""
    monkeypatch.setenv("MC33_HIP_LIVE", "1")


@pytest.fixture(autouse=True)
def blocks_always(live_list_always, monkeypatch):
    """... and MC33_HIP_BLOCKS=1 beside it, for the modules about blocks left out (they import both fixtures)"""
    monkeypatch.setenv("MC33_HIP_BLOCKS", "1")


def depth_fixture(params, ids=None):
    """a fixture `depth`: tiles that many planes deep (MC33_HIP_RZ / MC33_HIP_MIN_DEPTH, read when a context is made); 0: as they come"""
    @pytest.fixture(params=params, ids=ids)
    def depth(request, monkeypatch):
        if request.param:
            monkeypatch.setenv("MC33_HIP_RZ", str(request.param))
            monkeypatch.setenv("MC33_HIP_MIN_DEPTH", str(request.param))
        return request.param
    return depth


@pytest.fixture(params=[B, BIG], ids=["B", "BIG-two-plans"])
def switching(request, monkeypatch):
    """B as it comes; BIG with a device of one block per CU and a plan with a table of tiles one plane deep: the two plans differ"""
    if request.param == BIG:
        monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
        monkeypatch.setenv("MC33_HIP_RZ_TABLE", "1")
    return request.param


# ---- two z-slabs as windows of one tensor ----------------------------------------------------------------------------------------------

def emit_slab(g, c, base):
    """the surface of the counts c that g holds, emitted at the vertex base: (V, N, T as uint32, vertices)"""
    import torch
    V = torch.empty((max(c.nV, 1), 3), dtype=torch.float32, device="cuda")
    N = torch.empty_like(V)
    T = torch.empty((max(c.nT, 1), 3), dtype=torch.int32, device="cuda")
    g.emit_into(V, N, T, base)
    torch.cuda.synchronize()
    return V[:c.nV].cpu().numpy(), N[:c.nV].cpu().numpy(), T[:c.nT].cpu().numpy().view(np.uint32), c.nV


def slabs_are_the_surface(parts, ref):
    """the slabs of emit_slab, one behind the other, are the reference's V, N and T byte for byte"""
    assert np.array_equal(np.concatenate([p[2] for p in parts]), ref.T)
    assert np.array_equal(words(np.concatenate([p[0] for p in parts])), words(ref.V))
    assert np.array_equal(words(np.concatenate([p[1] for p in parts])), words(ref.N))


def two_slab_case(reflibs, per_slab, shape=B, timing=0):
    """steep(shape) at STEEP_ISO[shape] as two z-slabs, each a window of one tensor: slices 0 .. 17, and the upper ones with
    plane0 > 0 and a ghost slice below the range.  Per slab three counts that agree, the caller's check per_slab(g, the window's
    samples, its first plane, the first slice it reads, the counts), and the emit at the running vertex base; the two slabs
    together are the whole surface."""
    from mc33_c_library_amd import DeviceGrid, Range
    data = steep(shape)
    iso = STEEP_ISO[shape]
    ref = reference(reflibs, ("steep", shape), "f32", data, iso)
    t = to_device(data)
    nz_total = shape[0] - 1
    zb = 17
    parts = []
    for lo_plane, hi_plane, r in ((0, zb + 2, Range(0, zb, 0, 0)), (zb - 2, shape[0], Range(zb, nz_total, 1, 0))):
        g = DeviceGrid(t[lo_plane:hi_plane], nz_total=nz_total, plane0=lo_plane)
        if timing:
            g.set_timing(timing)
        cnts = [g.count(iso, r) for rep in range(3)]
        assert len({(c.nV, c.nT) for c in cnts}) == 1
        per_slab(g, data[lo_plane:hi_plane], lo_plane, zb - 1 if lo_plane else 0, cnts)
        parts.append(emit_slab(g, cnts[-1], sum(p[3] for p in parts)))
        g.close()
    slabs_are_the_surface(parts, ref)
