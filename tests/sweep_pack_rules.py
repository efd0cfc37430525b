"""numpy restatements of the two device-free rules of the sweep with a range table: the order of the packed live
list (mc33_c_library_amd/csrc/mc33_sweep_pack.h), and the size of the plan (mc33_sweep_plan.h).  Written from the rules as DESIGN.md states them, not
from the header's code: tests/test_sweep_pack_cpu.py holds the header to them, tests/test_gpu_sweep_pack.py the device."""
import numpy as np

NONE, GROUP = 0xFFFFFFFF, 0x80000000
FILL, BAND_LO, BAND_HI, MIN_DEPTH, DEFAULT_DEPTH = 0.68, 0.62, 0.72, 3.0, 5.0


def packed_entries(dead, grouped):
    """the packed list [entries][4] of a plan whose tiles have the verdicts dead[tile]; grouped[block]: the plan made the block of
    four neighbouring segments over the same rows and planes.
    A block with four live tiles stays one entry, at W(b) + ceil(L(b) / 4); the live tiles of all other blocks go four at a time, in
    plan order, quad q at q + W(block of its first tile) - W(b) whole blocks, L(b) leftover tiles before block b."""
    n = len(dead)
    nb = (n + 3) // 4
    d = np.ones(nb * 4, bool)
    d[:n] = dead
    d = d.reshape(nb, 4)
    whole = ~d.any(axis=1)
    left = ~d & ~whole[:, None]
    W = np.concatenate([[0], np.cumsum(whole)])
    L = np.concatenate([[0], np.cumsum(left.sum(axis=1))])
    tiles = np.flatnonzero(left.reshape(-1))
    out = np.full((int(whole.sum()) + (len(tiles) + 3) // 4, 4), NONE, np.uint32)
    taken = np.zeros(len(out), bool)
    for b in np.flatnonzero(whole):
        at = int(W[b] + (L[b] + 3) // 4)
        assert not taken[at]
        taken[at] = True
        out[at] = 4 * b + np.arange(4)
        if grouped[b]:
            out[at, 0] |= GROUP
    for q in range((len(tiles) + 3) // 4):
        quad = tiles[4 * q:4 * q + 4]
        at = int(q + W[quad[0] // 4])
        assert not taken[at]
        taken[at] = True
        out[at, :len(quad)] = quad
    assert taken.all()
    return out


def check_entries(entries, dead):
    """what any packed list has to be: every live tile once, no dead tile, first tiles ascending in plan order, only the last quad short"""
    e = np.asarray(entries, np.uint32).reshape(-1, 4).copy()
    if len(e) == 0:
        assert np.asarray(dead).all()
        return
    e[:, 0] &= ~np.uint32(GROUP)
    idx = e[e != NONE]
    assert len(np.unique(idx)) == len(idx), "a tile twice"
    assert (idx < len(dead)).all() and not np.asarray(dead)[idx].any(), "a dead tile"
    assert len(idx) == int((~np.asarray(dead)).sum()), "a live tile is missing"
    assert (np.diff(e[:, 0].astype(np.int64)) > 0).all(), "first tiles do not ascend"
    short = np.flatnonzero((e == NONE).any(axis=1))
    assert len(short) <= 1 and (e[:, 0] != NONE).all(), "more than one short entry"
    for at in short:   # the last quad: only whole blocks of the plan come behind it
        k = int((e[at] != NONE).sum())
        assert (e[at, :k] != NONE).all()
        later = e[at + 1:].astype(np.int64)
        assert (later[:, 0] % 4 == 0).all() and (later == later[:, :1] + np.arange(4)).all(), "a quad behind the short one"
    for r in e:  # within an entry too
        v = r[r != NONE].astype(np.int64)
        assert (np.diff(v) > 0).all()


def grouped_blocks(tiles):
    """per block of four consecutive tiles {seg, yt, z_lo, z_hi}: the segments seg .. seg + 3 of one y tile over the same planes"""
    n = len(tiles)
    out = np.zeros((n + 3) // 4, bool)
    for b in range(n // 4):
        q = np.asarray(tiles[4 * b:4 * b + 4], np.int64)
        out[b] = (q[:, 0] == q[0, 0] + np.arange(4)).all() and (q[:, 1] == q[0, 1]).all() and (q[:, 2] == q[0, 2]).all() and (q[:, 3] == q[0, 3]).all()
    return out


def target(live, tiles, resident, unit, min_depth=MIN_DEPTH, fill=FILL):
    """tiles to ask the plan for: the packed blocks of a plan of that size, at the live share live / tiles, are fill of the resident
    blocks; never more tiles than unit / min_depth (tiles min_depth planes deep), never fewer than one round; 0: nothing to go by"""
    if not live or not tiles or not resident:
        return 0
    t = min(fill * 4.0 * resident * tiles / live, unit / (min_depth if min_depth > 0 else 1.0))
    t = min(max(t, 4.0 * resident), 1073741823.0)   # never fewer tiles than one round: such a plan gets no list, and no count again
    return 1 if t < 1.0 else int(t)


def keeps(live, resident, lo=BAND_LO, hi=BAND_HI):
    return lo * resident <= (live + 3) // 4 <= hi * resident


def unit_of(shape, nzc=None, rows_per_batch=4):
    """the tiles the slices of a grid (points z, y, x) make at one plane per tile: sample rows in whole batches x segments x slices / 64"""
    ny, nx = shape[1] - 1, shape[2] - 1
    nseg, nyt = (nx + 255) // 256, (ny + 62) // 63
    rb = rows_per_batch
    W = sum((min(64, ny + 1 - 63 * yt) + rb - 1) // rb * rb for yt in range(nyt)) * nseg
    return W * float(shape[0] - 1 if nzc is None else nzc) / 64.0


def floor_depth(unit, resident, env_min_depth=0):
    """the smallest depth sizing goes to, None: the grid's plan is below one round and is left alone"""
    if unit / DEFAULT_DEPTH >= 4.0 * resident:
        return MIN_DEPTH
    d = float(max(1, env_min_depth))
    return d if unit / d >= 4.0 * resident else None
