"""GPU tests of the block sweep's batch stream (a batch of k_sweep_live_blocks is one LIVE 64 x 16 block of a plane,
a dead block costs no instruction, and a plane's bit rows start as what its dead blocks are worth): surfaces against the
unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit, with the fields, helpers and comparison of
tests/sweep_harness.py.  There is no tolerance in this file.

Shapes (points z, y, x): B = 40 x 70 x 1030 - five segments: one grouped block of four waves, whose first three take their halo
bits from the mailbox, and one ungrouped wave; two y tiles, the second of 7 rows (one row group, two batches' worth of rows in
the per-quarter form).  C3 = 24 x 130 x 300 - its second segment has 44 samples, quarters clamped to the grid's last column, its
waves are ungrouped, and its third y tile has 4 rows.

Every case extracts three times (the first sweeps have no block table), and where blocks are to be left out it asserts that
they were: mc33hip_sweep_skipped_blocks equals range_blocks_rules.left_out, below and above both positive unless the case says
otherwise."""
import numpy as np
import pytest

import range_blocks_rules as br
from sweep_harness import (B, C3, alias_cells, blocks_always, grid_of, left_out, live_list_always, live_mask, plan_of, reference, same,  # noqa: F401
                           same_arrays, steep, to_device, words_of)   # (blocks_always, live_list_always: the module's fixtures)

pytestmark = pytest.mark.gpu

C3_ISO = 700.5   # (steep(C3) runs from 0 to 1565)


def two_slabs(shape):
    """-1 in the lower half of the planes, +1 in the upper half: every block of every plane is dead - below the isovalue 0 in the
    lower planes, above it in the upper ones - and every cell between the two middle planes is cut"""
    data = np.full(shape, -1.0, np.float32)
    data[shape[0] // 2:] = 1.0
    return data


def strips_of(shape):
    """(yt, seg, first sample row, sample rows, first sample, samples) of the strips of a plane"""
    nyt, nseg = br.dims(shape)
    for yt in range(nyt):
        for seg in range(nseg):
            yield yt, seg, 63 * yt, min(64, shape[1] - 63 * yt), 256 * seg, min(256, shape[2] - 256 * seg)


def wandering(shape):
    """two_slabs with one bump of 2 x 2 samples on the other side of the isovalue per (plane, strip), inside block
    (p + 5 seg) mod (4 x row groups of the strip) - the one batch of the plane is at a different place in every wave of a block
    and in every plane.  On the planes p = 0 mod 5 segment (p / 5) mod 5 has no bump: a wave goes through that plane without a
    batch.  A bump whose place lies beyond the grid (the narrow last segment) is left out too.  Rows 5 and 6 of a row group (4 and 5
    in the y tile of 7 rows) and samples 10 and 11 of a quarter: no bump touches the row two y tiles share, a segment's first sample
    or a block's border."""
    data = two_slabs(shape)
    placed = np.zeros(16, int)
    for p in range(shape[0]):
        for yt, seg, y0, nrows, x0, ncols in strips_of(shape):
            if p % 5 == 0 and seg == (p // 5) % 5:
                continue
            j = (p + 5 * seg) % (4 * ((nrows + 15) // 16))
            g, k = j // 4, j % 4
            y, x = y0 + 16 * g + min(5, nrows - 3), x0 + 64 * k + 10
            if y + 1 < y0 + nrows - 1 and x + 1 < min(x0 + ncols, shape[2]):
                data[p, y:y + 2, x:x + 2] = -data[p, y, x]
                placed[j] += 1
    assert (placed > 0).all()
    return data


def halo_bumps(shape, xs):
    """two_slabs with single samples on the other side of the isovalue at x in xs (multiples of 256: a segment's first sample, and
    the halo column of the segment to its left), one per plane and y tile"""
    data = two_slabs(shape)
    for p in range(shape[0]):
        for yt in range(br.dims(shape)[0]):
            nrows = min(64, shape[1] - 63 * yt)
            y = 63 * yt + 1 + (5 * p + 3) % (nrows - 2)   # (never the tile's first or last row: those are shared)
            for x in xs:
                data[p, y, x] = -data[p, y, x]
    return data


def rough(shape):
    """0 / 1 in bricks of 32 x 8 x 16 samples (x, y, z): every block of every plane - the 64 x 16 ones, the halo columns over 16 rows,
    the clamped ones of the narrow last segment and of the y tile of 7 rows - holds samples on both sides of 0.5"""
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    return ((x // 32 + y // 8 + z // 16) % 2).astype(np.float32)


def run_case(reflibs, data, iso, key, what, dead_sides=(True, True), ref=None):
    """three extractions against the reference, then the count of the blocks left out; returns the grid (the caller closes it)"""
    if ref is None:
        ref = reference(reflibs, key, "f32", data, iso)
    g = grid_of(to_device(data))
    g.set_timing(1)
    for rep in range(3):
        same(g.extract(iso), ref, (what, rep))
    live = live_mask(g, data, iso)
    want = br.left_out(br.numpy_blocks(data, np.float32), iso, live)
    got = left_out(g)
    assert got == want, (what, got, want)
    assert want[0] > 0 and (want[1] > 0) == dead_sides[0] and (want[2] > 0) == dead_sides[1], (what, want)
    return g, ref


# ---- 1. one live block per plane, at another place in every wave ------------------------------------------------------------------------

def test_wandering_block(reflibs):
    data = wandering(B)
    g, ref = run_case(reflibs, data, 0.0, ("batches", "wandering B"), "wandering")
    assert ref.nV > 70000   # (the sheet between the two slabs alone is 1029 x 69 cells)
    # a live strip has at most the bump's block live (and none where the bump was left out)
    w = words_of(g)
    lo = (w[w != br.UNWRITTEN] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    live_bits = ~(lo | lo >> np.uint32(1)) & np.uint32(0x55555555)
    nlive = np.array([bin(int(x)).count("1") for x in live_bits])
    assert len(nlive) > 200 and nlive.max() == 1 and (nlive == 1).sum() > len(nlive) // 2
    g.close()


# ---- 2. a dead quarter 3 whose halo block is live ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["B mailbox", "B own", "C3 own"])
def test_halo_only(reflibs, case):
    shape, xs = {"B mailbox": (B, (256, 512, 768)), "B own": (B, (1024,)), "C3 own": (C3, (256,))}[case]
    data = halo_bumps(shape, xs)
    g, ref = run_case(reflibs, data, 0.0, ("batches", "halo", case), case)
    # what the case is about, from the library's own words: in the strips left of a bump quarter 3 of the bump's row group is
    # dead, and the halo block of that group is live
    w, seen = words_of(g), 0
    for p in range(1, shape[0]):
        for x in xs:
            word = int(w[p, 0, x // 256 - 1])
            if word == int(br.UNWRITTEN):
                continue
            grp = (1 + (5 * p + 3) % 62) // 16
            assert (word >> (2 * (4 * grp + 3))) & 3 != 0 and (word >> (32 + 2 * grp)) & 3 == 0, (case, p, x, hex(word))
            seen += 1
    assert seen >= shape[0] // 2
    g.close()


# ---- 3. nothing dead: 16 batches a plane ----------------------------------------------------------------------------------------------------

def test_nothing_dead(reflibs, monkeypatch):
    """every block of the row groups a tile HAS is live.  (The y tile of 7 rows has one row group; the blocks of its other three
    are single clamped samples or single clamped rows, dead or not, and are never streamed - they are what the count below and
    above consists of here.)"""
    data = rough(B)
    c = br.codes(br.numpy_blocks(data, np.float32), 0.5)
    assert (c[:, 0] == 0).all() and (c[:, 1][..., [0, 1, 2, 3, 16]] == 0).all()
    g, ref = run_case(reflibs, data, 0.5, ("batches", "rough B"), "rough")
    on = g.extract(0.5)
    monkeypatch.setenv("MC33_HIP_BLOCKS", "0")
    g0 = grid_of(to_device(data))
    for rep in range(3):
        off = g0.extract(0.5)
    same_arrays(on, off, "every block live, with and without the block stream")
    g.close(); g0.close()


# ---- 4. samples equal to the isovalue beside dead blocks ---------------------------------------------------------------------------------

def equal_samples(shape):
    """+1 everywhere (above the isovalue 0) but for samples EQUAL to it: in block (row group 1, quarter 2) of segment 1 of y tile 0, on
    plane 7 - one in the block's first row, one in its last, one in between - and on plane 9 the first sample of segment 2 in row 20:
    column 0 of a wave of the group, whose bit and whose "equals the isovalue" mark go through the mailbox.  Each has one sample
    below the isovalue beside it, inside the same block, so that there is a surface through it.  Every neighbouring block is dead."""
    data = np.full(shape, 1.0, np.float32)
    x0 = 256 + 128
    data[7, 16, x0 + 7], data[7, 17, x0 + 7] = 0.0, -1.0
    data[7, 31, x0 + 40], data[7, 30, x0 + 40] = 0.0, -1.0
    data[7, 23, x0 + 63], data[7, 23, x0 + 62] = 0.0, -1.0
    data[9, 20, 512], data[9, 20, 513] = 0.0, -1.0
    return data


def test_equal_to_the_isovalue_beside_dead_blocks(reflibs, monkeypatch):
    data = equal_samples(B)
    g, ref = run_case(reflibs, data, 0.0, ("batches", "equal B"), "equal", dead_sides=(False, True))
    assert ref.nT > 0
    on, on_alias = g.extract(0.0), alias_cells(g)
    w = words_of(g)
    assert int(w[7, 0, 1]) & 0xFFFFFFFF == 0xAAAAAAAA & ~(3 << (2 * 6)), hex(int(w[7, 0, 1]))   # (one live block, 15 dead ones)
    monkeypatch.setenv("MC33_HIP_BLOCKS", "0")
    g0 = grid_of(to_device(data))
    for rep in range(3):
        off = g0.extract(0.0)
    same_arrays(on, off, "samples equal to the isovalue")
    assert on_alias == alias_cells(g0) and on_alias > 0
    g.close(); g0.close()


def test_negative_zero_on_zeros_with_a_bump(monkeypatch):
    """iso = -0.0 on the field of test_negative_zero_against_a_block_of_zeros: every sample but the bump's equals the isovalue and
    every block is live.  The reference is not a function of its input for this isovalue on zeros (see
    tests/test_gpu_range_skip.py), so the surface is held to the one a context with MC33_HIP_BLOCKS=0 gives, byte for byte."""
    data = np.zeros((6, 20, 300), np.float32)
    data[2, 5:8, 40:44] = 1.0
    g = grid_of(to_device(data))
    for rep in range(3):
        on = g.extract(-0.0)
    assert (words_of(g) == 0).all()
    monkeypatch.setenv("MC33_HIP_BLOCKS", "0")
    g0 = grid_of(to_device(data))
    for rep in range(3):
        off = g0.extract(-0.0)
    same_arrays(on, off, "iso -0.0 on zeros")
    assert alias_cells(g) == alias_cells(g0)
    g.close(); g0.close()


# ---- 5. clamped quarters, a 4-row tile, a partial row group --------------------------------------------------------------------------------

def test_c3_steep(reflibs):
    data = steep(C3)
    g, ref = run_case(reflibs, data, C3_ISO, ("steep", C3), "steep C3")
    assert ref.nV > 5000
    g.close()


# ---- 6. one tile per column, the whole grid deep: the log is flushed in the middle of the block stream -------------------------------------

def test_a_deep_tile(reflibs, monkeypatch):
    monkeypatch.setenv("MC33_HIP_RZ", str(B[0] - 1))
    monkeypatch.setenv("MC33_HIP_MIN_DEPTH", str(B[0] - 1))
    data = wandering(B)
    g, ref = run_case(reflibs, data, 0.0, ("batches", "wandering B"), "deep tile")
    tiles = plan_of(g)[0]
    assert (tiles[:, 3] - tiles[:, 2]).min() == B[0] - 1, "the tiles are not the grid's depth"
    g.close()
