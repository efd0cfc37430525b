"""GPU tests of the sized plan cut by what a wave's life costs: the plan of a single-isovalue sweep that leaves dead
blocks out shares its tiles out by batches + the weight of a plane, every other plan by batches alone as before; a lane keeps the
weight of its plan beside the target; and at the device's own residency such a plan goes by a fill and a band of its own.

Every surface is compared with the unmodified reference's (oracle/_ref) on the dense numpy array, bit for bit, with the fields,
helpers and comparison of tests/sweep_harness.py.  There is no tolerance in this file.  The plans are held to the numpy restatement of the share rule (tests/sweep_plan_rules.py)."""
import numpy as np
import pytest

import sweep_pack_rules as pr
import sweep_plan_rules as sp
from sweep_harness import (A, B, BIG, HIGH, LOW, STEEP_ISO, banded, by_the_rule, check_packed, check_plan, grid_of, live_everywhere,  # noqa: F401
                           live_list_always, numpy_table, packed_of, plan_of, reference, same, steep, table_of, to_device, two_slab_case,
                           weight_of, words_of)   # (live_list_always: the module's fixture)

pytestmark = pytest.mark.gpu


# ---- 1. the plan of a sweep that leaves blocks out, sized twice --------------------------------------------------------------------

def test_sized_plans_are_cut_by_the_weight(reflibs, monkeypatch):
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    data = banded(96)
    refs = {iso: reference(reflibs, ("pack", "banded 96"), "f32", data, iso) for iso in (LOW[0], HIGH)}
    g = grid_of(to_device(data))
    seen = []
    for iso in (LOW[0], HIGH):
        for rep in range(6):   # (a count is published by one call, asks for a size in the next, and is obeyed when the one after agrees)
            same(g.extract(iso), refs[iso], ("balance", iso, rep))
        by_the_rule(g, ("balance", iso))                        # packed blocks in the band of a forced residency: 0.62 - 0.72
        weight, chunks = check_plan(g, BIG, ("balance", iso))
        assert weight > 0.0, "a sized plan of a sweep that leaves blocks out is cut with a weight"
        # the short last y tile (one batch per plane) is (16 + w) / (1 + w) times as deep as the others, no longer sixteen times
        full, short = chunks[0], chunks[-2]
        assert (full - 1.0) / (short + 1.0) <= (16.0 + weight) / (1.0 + weight) <= (full + 1.0) / max(short - 1.0, 0.5), chunks
        seen.append((len(plan_of(g)[0]), chunks))
    assert seen[1][0] >= 1.2 * seen[0][0], seen
    assert words_of(g).shape == (BIG[0], 3, 5)   # blocks were left out: mc33hip_block_words has words to give
    g.close()


def test_no_weight_without_the_block_skip(reflibs, monkeypatch):
    """MC33_HIP_BLOCKS=0: the sweeps stream every block of a live tile, and the sized plan is the one it always was"""
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("MC33_HIP_BLOCKS", "0")
    data = banded(96)
    refs = {iso: reference(reflibs, ("pack", "banded 96"), "f32", data, iso) for iso in (LOW[0], HIGH)}
    g = grid_of(to_device(data))
    for iso in (LOW[0], HIGH):
        for rep in range(6):
            same(g.extract(iso), refs[iso], ("no skip", iso, rep))
        n = by_the_rule(g, ("no skip", iso))
        weight, chunks = check_plan(g, BIG, ("no skip", iso))   # (weight 0: check_plan restates the rule by batches alone)
        assert weight == 0.0 and n > 4 * plan_of(g)[1]
        assert chunks[0] >= 12 * max(chunks[-2], 2), chunks       # the short y tile as many batches deep as a full one
    g.close()


# ---- 2. a weighted plan on blocks that are not grouped ------------------------------------------------------------------------------

def test_weighted_plan_on_a_narrow_grid(reflibs, monkeypatch):
    """A is three segments wide: no block of its plans is a whole group, and blocks are left out only with MC33_HIP_BLOCKS=1.  Its
    plans are below one round of any device, so a size is asked for by MC33_HIP_TABLE_TILES."""
    monkeypatch.setenv("MC33_HIP_TABLE_TILES", "150")
    data = steep(A)
    iso = STEEP_ISO[A]
    ref = reference(reflibs, ("steep", A), "f32", data, iso)
    chunks = {}
    for blocks in ("1", None):
        if blocks:
            monkeypatch.setenv("MC33_HIP_BLOCKS", blocks)
        else:
            monkeypatch.delenv("MC33_HIP_BLOCKS")
        g = grid_of(to_device(data))
        for rep in range(3):
            same(g.extract(iso), ref, ("narrow", blocks, rep))
        weight, chunks[blocks] = check_plan(g, A, ("narrow", blocks), asked=150)
        assert plan_of(g)[2] == 1 and (weight > 0.0) == (blocks == "1"), (blocks, weight)
        tiles, dead, grouped, e = check_packed(g, numpy_table(data, "f32"), (iso,), ("narrow", blocks))
        assert not grouped.any() and dead.any() and not dead.all()
        g.close()
    assert chunks["1"] != chunks[None] and chunks["1"][-1] > chunks[None][-1], chunks   # the last y tile (12 sample rows) gets more, shallower tiles


# ---- 3. a sub-range with a ghost plane ---------------------------------------------------------------------------------------------------

def test_sub_range_with_a_ghost_plane_under_a_weighted_plan(reflibs, monkeypatch):
    """the upper z-slab of B as a window with plane0 > 0 and a ghost slice, each slab by a sized, weighted plan; the two slabs
    together are the whole surface"""
    monkeypatch.setenv("MC33_HIP_TABLE_TILES", "90")

    def the_plan_is_weighted(g, window, lo_plane, zs, cnts):
        weight, chunks = check_plan(g, B, ("slab", lo_plane), asked=90)
        assert weight > 0.0 and plan_of(g)[2] == 1
        check_packed(g, table_of(g, "f32"), (STEEP_ISO[B],), ("slab", lo_plane), zs=zs, plane0=lo_plane)
    two_slab_case(reflibs, the_plan_is_weighted)


# ---- 4. a re-target under swept lanes -------------------------------------------------------------------------------------------------

def test_retarget_to_weighted_plans_under_swept_lanes(reflibs, monkeypatch):
    """lanes swept by the default plan (no weight), then single calls that size a weighted plan and size it again, then the lanes
    emitted in reverse: each tail asks for the plan of its lane by slot, target AND weight"""
    monkeypatch.setenv("MC33_HIP_SWEEP_BLOCKS_PER_CU", "1")
    data = banded(96)
    refs = [reference(reflibs, ("pack", "banded 96"), "f32", data, iso) for iso in LOW]
    ref_high = reference(reflibs, ("pack", "banded 96"), "f32", data, HIGH)
    ref_one = reference(reflibs, ("pack", "banded 96"), "f32", data, LOW[0] + 1.0)
    g = grid_of(to_device(data))
    g.sweep_many(LOW)
    assert table_of(g, "f32") is not None and weight_of(g) == 0.0   # passes over several isovalues: by batches alone
    n1 = len(plan_of(g)[0])
    for rep in range(4):
        same(g.extract(LOW[0] + 1.0), ref_one, ("re-target", rep))
    n2, w2 = len(plan_of(g)[0]), weight_of(g)
    for rep in range(4):
        same(g.extract(HIGH), ref_high, ("re-target again", rep))
    n3, w3 = len(plan_of(g)[0]), weight_of(g)
    assert n2 != n1 and n3 != n2 and plan_of(g)[2] == 1 and w2 > 0.0 and w3 == w2, (n1, n2, n3, w2, w3)
    for k in reversed(range(8)):
        same(g.extract(LOW[k]), refs[k], ("lane", k))
        if k >= 4:   # (lanes 7 .. 4 were swept by the default plan with the table: the tail put that plan back in force)
            assert weight_of(g) == 0.0 and len(plan_of(g)[0]) == n1, k
    same(g.extract(HIGH), ref_high, "the sized plan again")
    assert weight_of(g) == w2
    g.close()


# ---- 5. the fill and band of weighted plans at the device's own residency ---------------------------------------------------------------

def test_weighted_plans_fill_the_device_at_its_own_residency(reflibs, monkeypatch):
    """nobody forces the residency: the sized plan of a sweep that leaves blocks out goes by the second fill and band, right below
    one round.  The grid is the smallest that lets the rule show on the cross-section of BIG: with MC33_HIP_MIN_DEPTH=1 a sized
    plan may be as fine as one plane per tile, `unit` tiles, and at a live share of 0.8 the rule asks for fill x 4 x resident / 0.8
    tiles - so nzc is the least for which that is no more than unit (about 250 MB of float at 256 compute units), and the field
    is live below 0.85 of its planes: above 0.8, below the 0.9 that sends sweeps back to the coarse plan."""
    monkeypatch.setenv("MC33_HIP_MIN_DEPTH", "1")
    small = grid_of(to_device(steep(B)))
    small.extract(STEEP_ISO[B])
    resident = plan_of(small)[1]
    small.close()
    per_slice = pr.unit_of((2,) + BIG[1:])                       # tiles of one slice at one plane per tile
    nzc = int(np.ceil(sp.FILL_BALANCED * 4 * resident / 0.8 / per_slice))
    shape = (nzc + 1,) + BIG[1:]
    z0 = int(round(0.85 * nzc))
    data = live_everywhere(shape)
    data[z0:] += 1000.0
    iso = LOW[0]
    ref = reference(reflibs, ("balance", "own residency", shape, z0), "f32", data, iso)
    assert ref.nV > 1000
    g = grid_of(to_device(data))
    for rep in range(6):   # (no table, table and count, a size asked for, agreed and made, and two sweeps by it)
        same(g.extract(iso), ref, ("own residency", rep))
    tiles, res, which = plan_of(g)
    e, live, ntiles = packed_of(g)
    weight, chunks = check_plan(g, shape, "own residency")
    print("own residency: %d resident, %d planes, %d tiles, %d live, %d packed blocks (%.3f)" % (res, nzc, ntiles, live, len(e), len(e) / res))
    assert res == resident and which == 1 and weight == sp.PLANE_WEIGHT and ntiles == len(tiles) > 4 * resident
    assert 0.8 * ntiles <= live < 0.9 * ntiles
    assert sp.BAND_BALANCED_LO * resident <= len(e) <= sp.BAND_BALANCED_HI * resident, (len(e), resident)
    assert not pr.keeps(live, resident)                          # ... which is outside the band of a forced residency
    same(g.extract(iso), ref, ("own residency", "kept"))
    assert len(plan_of(g)[0]) == ntiles, "a plan inside its band was replaced"
    g.close()
