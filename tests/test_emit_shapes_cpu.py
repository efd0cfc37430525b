"""The work split of the emit passes (tests/emit_shapes.py restates XcdBatchWalk and XcdWalk of mc33_emit.hip.h word for word):
for every grid the host launches - a multiple of 8 - the walks of all waves / blocks partition the work exactly; for a grid
that is no multiple of 8 the triangle pass's walk has a hole, which is why the host rounds MC33_HIP_EMIT_BLOCKS and
MC33_HIP_EMIT_V_BLOCKS; and the shape list of tests/test_gpu_emit_shapes.py reaches walk lengths 1, 2, 3 and >= 4 on the
batch counts its grids have.  No GPU, no library."""
import pytest

import emit_cases as ec
import emit_shapes as es

BLOCKS = (8, 16, 24, 64, 768, 1024)


def flat(walks):
    return sorted(x for w in walks for x in w)


def test_batch_walks_partition_the_batches():
    for nbatch in list(range(301)) + [1000, 13812]:
        for blocks in BLOCKS:
            walks = es.batch_walk(nbatch, blocks)
            assert len(walks) == 4 * blocks
            assert flat(walks) == list(range(nbatch)), (nbatch, blocks)  # every batch once: none left out, none twice
            for w in walks:  # a wave's batches ascend by the same stride, inside one XCD's eighth
                assert all(b - a == (blocks >> 3) * 4 for a, b in zip(w, w[1:])), (nbatch, blocks, w)


def test_record_walks_partition_the_chunks():
    sizes = list(range(0, 2600, 37)) + [255, 256, 257, 2047, 2048, 2049, 8012, 14708, 24806, 65536, 69999, 70000]
    for n in sizes:
        for blocks in BLOCKS:
            walks = es.record_walk(n, blocks)
            assert len(walks) == blocks
            assert flat(walks) == list(range((n + 255) // 256)), (n, blocks)


@pytest.mark.parametrize("blocks", [12, 20])
def test_a_grid_that_is_no_multiple_of_8_leaves_chunks_unwalked(blocks):
    """XCDs 4..7 of 12 (20) blocks own one slot (two) but stride by ceil(blocks / 8): chunks of theirs are never taken.  A
    record_walk 'mended' to cover them would not be the kernel's."""
    for n in (8012, 24806, 70000):
        chunks = (n + 255) // 256
        got = flat(es.record_walk(n, blocks))
        assert len(set(got)) == len(got)  # (nothing twice)
        missing = sorted(set(range(chunks)) - set(got))
        assert missing, (n, blocks)
        per_xcd = (chunks + 7) // 8
        assert all(c // per_xcd >= 4 for c in missing), (n, blocks, missing)  # the XCDs with the fewer blocks
        assert flat(es.record_walk(n, es.round8(blocks))) == list(range(chunks))  # what the host launches instead
    # 12 blocks over the 32 chunks of cos_field(48): XCDs 0..3 walk their four chunks with two blocks, XCDs 4..7 take chunks 0 and 2 of theirs
    assert sorted(set(range(32)) - set(flat(es.record_walk(8012, 12)))) == [17, 19, 21, 23, 25, 27, 29, 31]
    assert es.round8(12) == 16 and es.round8(20) == 24 and es.round8(8) == 8 and es.round8(1) == 8


def test_slow_rounds():
    assert es.slow_rounds(0, 1, False) == (0, False) and es.slow_rounds(256, 1, False) == (1, False) and es.slow_rounds(257, 1, False) == (2, False)
    assert es.slow_rounds(32, 1, True) == (2, False) and es.slow_rounds(33, 1, True) == (1, True) and es.slow_rounds(16, 1, True) == (1, False)
    # MC33_HIP_SLOW_BLOCKS = ceil(n / 32), the "two rounds" shape of the GPU test: exactly two rounds of the lane-per-slot loop from 17 records on
    for n in list(range(17, 2000)) + [8800, 34000, 100000]:
        assert es.slow_rounds(n, (n + 31) // 32, True) == (2, False), n


# record batches of the small grids of the GPU test as the CPU model has them (sum over slots of ceil(cut cells / 64)): cos_field(48)
# at 0.1 - the grid every sample type and the inclined store take -, cos_field(64) at 0, noise_quant(32, 2) at 1
SMALL = (145, 255, 402)
# ... and of its rough (9, 66, 258) grids, and of the full-size noise grid that is not needed: every wave walks at least 4
LARGE = (2082, 13812)


def band(nbatch):
    """the device's number may differ from the model: any count within 25 % of it"""
    return range(nbatch - nbatch // 4, nbatch + nbatch // 4 + 1)


def test_the_shape_list_reaches_every_walk_length():
    """Walk lengths 1, 2, 3 and >= 4 all occur over MC33_HIP_EMIT_V_BLOCKS in {8, 16, 32, 64} for any batch count within 25 % of
    the small grids' - except a count of exactly 8 * 16 or 8 * 32, where every XCD's share is a power of two and the waves of an
    XCD, a multiple of four, walk 4, 2 or 1 batches each and never 3 (128 is 12 % below the model's 145: the GPU test's own
    closing assertion is what decides).  The rough grids have batches enough for every wave to walk at least 4 under every shape
    of the list; the short walks are the small grids' part."""
    assert es.VERTEX_SHAPES == tuple(int(ec.SHAPES[k]["MC33_HIP_EMIT_V_BLOCKS"]) for k in ("v8", "v16", "v32", "v64"))
    never_three = {128, 256}
    for model in SMALL:
        for nbatch in band(model):
            got = set().union(*[es.walk_lengths(nbatch, b) for b in es.VERTEX_SHAPES])
            assert got >= ({1, 2, 4} if nbatch in never_three else {1, 2, 3, 4}), (model, nbatch, sorted(got))
    assert es.walk_lengths(145, 16) == {1, 2, 3} and es.walk_lengths(145, 8) == {3, 4}
    assert {len(w) for w in es.batch_walk(145, 8)} == {3, 4, 5}
    assert es.walk_lengths(145, 768) == {1}  # the default grid of a 256-CU part: what the suite reached before
    for model in LARGE:
        for nbatch in band(model):
            for b in es.VERTEX_SHAPES:
                assert es.walk_lengths(nbatch, b) == {4}, (model, nbatch, b)
    # the triangle pass: cos_field(48)'s 8 012 records make 4 rounds with 8 blocks, 2 with 16 - and with 12, once rounded
    assert [es.triangle_rounds(8012, b) for b in (8, 16, es.round8(12))] == [4, 2, 2]
    assert es.triangle_rounds(8012, 16384) == 1


def test_the_cases_name_every_switch_they_set():
    assert all(set(s) <= set(ec.SWITCHES) for s in ec.SHAPES.values())
    assert all(k in ec.SWITCHES for c in ec.CASES for k, _ in c.env)
    assert len(ec.CASES) == len(ec.BY_NAME) and {c.dtype for c in ec.CASES} == set(ec.NP)
