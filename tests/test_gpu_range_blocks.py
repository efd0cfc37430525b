"""GPU tests of the block table and of the sweep that leaves dead 64 x 16 sample blocks out inside live tiles (DESIGN.md 21;
include/mc33_hip.h: mc33hip_range_blocks, mc33hip_block_words, mc33hip_sweep_skipped_blocks): k_ranges' block entries and
k_block_verdicts' words against the numpy restatement of tests/range_blocks_rules.py, and the surfaces of sweeps whose loads are
left out against the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit, with the fields, helpers and
comparison of tests/sweep_harness.py.  There is no tolerance in this file.

Shapes (points z, y, x): A = 48 x 200 x 520, B = 40 x 70 x 1030, and C3 = 24 x 130 x 300, whose second segment has 44 samples -
quarter 0 of it partly, quarters 1 - 3 wholly clamped to the grid's last column - and whose third y tile has 4 rows."""
import numpy as np
import pytest

import range_blocks_rules as br
from sweep_harness import (A, B, C3, REAL, STEEP_ISO, alias_cells, blocks_always, blocks_of, grid_of, left_out, live_list_always, live_mask,  # noqa: F401
                           mixed_whole, reference, same, same_arrays, steep, table_of, to_device, two_slab_case, typed, words,
                           words_of)   # (blocks_always, live_list_always: the module's fixtures)

pytestmark = pytest.mark.gpu


# ---- 1. the block table against numpy ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", [A, B, C3], ids=["A", "B", "C3"])
def test_block_table_is_numpys(shape, dtype):
    data = typed(dtype, shape)
    g = grid_of(to_device(data))
    iso = float(data.mean()) + 0.5
    g.extract(iso)
    assert blocks_of(g, dtype) is None, "a block table after ONE sweep"
    g.extract(iso)
    t = blocks_of(g, dtype)
    assert t is not None
    want = br.numpy_blocks(data, REAL[dtype])
    assert np.array_equal(words(t), words(want)), (shape, dtype, np.argwhere(words(t) != words(want))[:5])
    # the strip's own entry is the minimum and maximum over its blocks
    coarse = table_of(g, dtype)
    assert np.array_equal(coarse[..., 0], want[..., 0].min(axis=3)) and np.array_equal(coarse[..., 1], want[..., 1].max(axis=3))
    g.close()


def test_block_table_sample_by_sample():
    """base one sample off, an odd pitch, a slice with rows to spare: k_ranges goes sample by sample and gives the same table"""
    import torch
    data = steep(A)
    pitch, slc = A[2] + 3, (A[2] + 3) * (A[1] + 2) + 1
    flat = torch.full((1 + slc * A[0] + 64,), 77, dtype=torch.float32, device="cuda")
    view = torch.as_strided(flat, A, (slc, pitch, 1), 1)
    view.copy_(to_device(data))
    assert view.data_ptr() % 16 != 0 or (pitch * 4) % 16 != 0
    g = grid_of(view)
    for rep in range(2):
        g.extract(STEEP_ISO[A])
    assert np.array_equal(words(blocks_of(g, "f32")), words(br.numpy_blocks(data, np.float32)))
    g.close()


def test_one_nan_is_one_block():
    data = steep(A).copy()
    data[5, 10, 17] = np.nan   # (inside y tile 0, segment 0, row group 0, quarter 0: no shared row, no halo column)
    g = grid_of(to_device(data))
    for rep in range(2):
        g.extract(STEEP_ISO[A])
    t = blocks_of(g, "f32")
    assert np.array_equal(words(t), words(br.numpy_blocks(data, np.float32)))
    inf = np.argwhere(np.isinf(t[..., 0]))
    assert inf.tolist() == [[5, 0, 0, 0]] and t[5, 0, 0, 0].tolist() == [-np.inf, np.inf] and np.isfinite(t[5, 0, 0, 1:]).all()
    g.close()


# ---- 2. the verdict words against numpy -----------------------------------------------------------------------------------------------

def words_case(data, iso, what):
    g = grid_of(to_device(data))   # (a context of its own: the words no sweep has written are all ones)
    for rep in range(3):
        g.extract(iso)
    live = live_mask(g, data, iso)
    got, want = words_of(g), br.expected_words(br.numpy_blocks(data, np.float32), iso, live)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5])
    g.close()
    return got, live


@pytest.mark.parametrize("shape", [A, B], ids=["A", "B"])
def test_verdict_words_are_numpys(shape):
    data = steep(shape)
    got, live = words_case(data, STEEP_ISO[shape], "between")
    written = got[live]
    assert live.any() and not live.all() and (written != 0).any()
    assert ((written & np.uint64(0x5555555555)) != 0).any() and ((written & np.uint64(0xAAAAAAAAAA)) != 0).any()   # blocks below, and above
    for iso in (-1.0, 1e6):          # every sample above / below: no tile is live, no word is written
        got, live = words_case(data, iso, iso)
        assert not live.any() and (got == br.UNWRITTEN).all()
    # an isovalue equal to a block's maximum: that block is live (the comparison is strict), its neighbour below it is not
    blocks = br.numpy_blocks(data, np.float32)
    iso = float(blocks[20, 0, 1, 5, 1])
    got, live = words_case(data, iso, "a block's maximum")
    assert live[20, 0, 1] and (int(got[20, 0, 1]) >> 10) & 3 == 0 and (int(got[20, 0, 1]) >> 8) & 3 == 1


def test_negative_zero_against_a_block_of_zeros():
    data = np.zeros((6, 20, 300), np.float32)
    data[2, 5:8, 40:44] = 1.0
    g = grid_of(to_device(data))
    for rep in range(3):
        g.extract(-0.0)
    assert (words_of(g) == 0).all()   # -0.0 == 0.0: neither strictly below nor above - every tile and every block is live
    g.close()
    # (+0.0 on the same samples: the cells around the bump have corners equal to the isovalue, and alias_cells counts them - what
    # test_block_checkerboard relies on when it finds none)
    g = grid_of(to_device(data))
    for rep in range(3):
        g.extract(0.0)
    assert (words_of(g) == 0).all() and alias_cells(g) > 0
    g.close()


# ---- 3. the block checkerboard: every tile live, every block dead ---------------------------------------------------------------------

def test_block_checkerboard(reflibs):
    data = br.checkerboard(B)
    blocks = br.numpy_blocks(data, np.float32)
    assert (blocks[..., 0] == blocks[..., 1]).all(), "a block of the checkerboard is not constant"
    ref = reference(reflibs, ("blocks", "checkerboard"), "f32", data, 0.0)
    assert ref.nV > 100000
    g = grid_of(to_device(data))
    g.set_timing(1)
    for rep in range(3):
        same(g.extract(0.0), ref, ("checkerboard", rep))
    live = live_mask(g, data, 0.0)
    assert live.all()
    n, below, above = left_out(g)
    assert n == br.BLOCKS * live.size and below + above == n and below > 0 and above > 0, (n, below, above)
    assert (n, below, above) == br.left_out(blocks, 0.0, live)
    assert alias_cells(g) == 0   # no sample put in the place of a load that was left out counts as equal to the isovalue 0.0
    g.close()


# ---- 4. surfaces of sweeps with blocks left out ---------------------------------------------------------------------------------------

SURFACES = {
    "steep A": (lambda: steep(A), STEEP_ISO[A], ("steep", A), 0),
    "steep B": (lambda: steep(B), STEEP_ISO[B], ("steep", B), 0),
    "mixed": (mixed_whole, 0.5, ("pack", "mixed whole"), 2),
}


@pytest.mark.parametrize("case", list(SURFACES))
def test_surface_with_blocks_left_out(reflibs, monkeypatch, case):
    make, iso, key, rz = SURFACES[case]
    if rz:
        monkeypatch.setenv("MC33_HIP_RZ", str(rz))
        monkeypatch.setenv("MC33_HIP_MIN_DEPTH", str(rz))
    data = make()
    ref = reference(reflibs, key, "f32", data, iso)
    g = grid_of(to_device(data))
    g.set_timing(1)
    for rep in range(3):
        same(g.extract(iso), ref, (case, rep))
    live = live_mask(g, data, iso)
    want = br.left_out(br.numpy_blocks(data, np.float32), iso, live)
    assert left_out(g) == want, (case, left_out(g), want)
    if case != "mixed":
        assert want[1] > 0 and want[2] > 0
    else:
        assert want[1] > 0
    g.close()


def test_sub_range_with_a_ghost_plane(reflibs):
    """the upper z-slab of B as a window with plane0 > 0 and a ghost slice; the two slabs together are the whole surface"""
    iso = STEEP_ISO[B]

    def blocks_were_left_out(g, window, lo_plane, zs, cnts):
        live = live_mask(g, window, iso, zs, lo_plane)
        want = br.left_out(br.numpy_blocks(window, np.float32), iso, live)
        assert left_out(g) == want and want[1] > 0 and want[2] > 0, (lo_plane, left_out(g), want)
    two_slab_case(reflibs, blocks_were_left_out, timing=1)


# ---- 5. the switch, and samples that change ------------------------------------------------------------------------------------------

def test_blocks_off_gives_the_same_bytes(reflibs, monkeypatch):
    data = steep(B)
    iso = STEEP_ISO[B]
    ref = reference(reflibs, ("steep", B), "f32", data, iso)
    t = to_device(data)
    g = grid_of(t)
    g.set_timing(1)
    for rep in range(3):
        on = g.extract(iso)
    assert left_out(g)[1] > 0
    monkeypatch.setenv("MC33_HIP_BLOCKS", "0")
    g0 = grid_of(t)
    g0.set_timing(1)
    for rep in range(3):
        off = g0.extract(iso)
    same(off, ref, "MC33_HIP_BLOCKS=0")
    same_arrays(on, off, "with and without blocks left out")
    assert left_out(g0) == (0, 0, 0) and blocks_of(g0, "f32") is None and table_of(g0, "f32") is not None
    g.close(); g0.close()


def test_a_write_into_a_block_that_was_left_out(reflibs):
    data = steep(A).copy()
    iso = STEEP_ISO[A]
    t = to_device(data)
    g = grid_of(t)
    for rep in range(3):
        same(g.extract(iso), reference(reflibs, ("steep", A), "f32", data, iso), ("before", rep))
    w = words_of(g)
    # a block below the isovalue inside a strip that a live tile reads
    p, yt, seg = [int(x) for x in np.argwhere((w != br.UNWRITTEN) & ((w & np.uint64(0x55555555)) != 0))[0]]
    j = next(j for j in range(16) if (int(w[p, yt, seg]) >> (2 * j)) & 3 == 1)
    rows, cols = br.block_index(A, yt, seg, j)
    y, x = int(rows[3]), int(cols[5])
    assert data[p, y, x] < iso
    v = t._version
    t[p, y, x] = 5000.0
    assert t._version != v
    data[p, y, x] = 5000.0
    ref1 = reflibs["f32"].isosurface(data, iso)
    assert ref1.nV > reference(reflibs, ("steep", A), "f32", steep(A), iso).nV
    for rep in range(3):
        same(g.extract(iso), ref1, ("after the write", rep))
    assert np.array_equal(words(blocks_of(g, "f32")), words(br.numpy_blocks(data, np.float32)))
    g.close()


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------------------

def test_three_extractions_leave_the_same_bytes(reflibs):
    data = mixed_whole()
    g = grid_of(to_device(data))
    g.extract(0.5)
    g.extract(0.5)
    runs = []
    for rep in range(3):
        V, N, T, cnt = g.extract(0.5)
        runs.append((V.cpu().numpy().tobytes(), N.cpu().numpy().tobytes(), T.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2] and len(runs[0][2]) > 0
    same(g.extract(0.5), reference(reflibs, ("pack", "mixed whole"), "f32", data, 0.5), "mixed whole")
    g.close()
