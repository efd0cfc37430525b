"""numpy restatement of how a sweep's plan shares its tiles out among its columns (mc33_c_library_amd/csrc/mc33_sweep_plan.h,
DESIGN.md 21 "The cost of a wave's life"), and of which fill and band a sized plan goes by.  Written from the rule as DESIGN.md
states it, not from the header's code: tests/test_sweep_plan_cpu.py holds the header to it, tests/test_gpu_sweep_balance.py the
device.

The rule.  A column is a group of up to four neighbouring row segments (256 cells each) x a y tile (63 cell rows); it has one wave
per segment.  The work of one of its waves per plane is w = batches + weight: the y tile's sample rows in whole batches of four,
and the weight of a plane in batches (0: batches alone).  Of a plan of B tiles, column i gets the share B w[i] / W of the chunks,
W = sum of w[i] x waves[i]; rounded down, at least 1, at most nzc (one plane per chunk); then, in the order of the largest
fractions, one chunk more per column that is not at nzc until the tiles - chunks x waves, summed - are at least B.  Which of two
columns with the same fraction comes first is not part of the rule."""
import numpy as np

import sweep_pack_rules as pr

# the measured weight of a plane in batches for sweeps that leave dead blocks out, and the fill and band of plans cut with a weight
# at the device's own residency (tests/test_sweep_plan_cpu.py holds the library's constants to them)
PLANE_WEIGHT = 3.0
FILL_BALANCED, BAND_BALANCED_LO, BAND_BALANCED_HI = 0.987, 0.978, 0.997


def columns(shape, rows_per_batch=4):
    """(y tile, segment group, waves, batches per plane) of every column of a grid of points (z, y, x), y tile major"""
    ny, nx = shape[1] - 1, shape[2] - 1
    nseg, nyt = (nx + 255) // 256, (ny + 62) // 63
    out = []
    for yt in range(nyt):
        rows = min(64, ny + 1 - 63 * yt)
        for xg in range((nseg + 3) // 4):
            out.append((yt, xg, min(4, nseg - 4 * xg), (rows + rows_per_batch - 1) // rows_per_batch))
    return out


def shares(cols, B, nzc, weight=0.0, unit=1.0):
    """(floor part of the chunks [col], fraction [col], waves [col]); unit: what a batch counts (the old rule counted sample rows,
    4 to a batch - the shares are the same numbers up to rounding in the last place, which the floor can see)"""
    w = [(c[3] + weight) * unit for c in cols]
    waves = np.array([c[2] for c in cols], np.int64)
    W = 0.0
    for k in range(len(cols)):
        W += w[k] * int(waves[k])
    share = np.array([float(B) * x / W for x in w])
    base = np.minimum(np.maximum(1.0, np.floor(share)), float(nzc)).astype(np.int64)
    return base, share - np.floor(share), waves


def check_chunks(chunks, cols, B, nzc, weight=0.0, unit=1.0):
    """chunks [col] is what the rule gives, up to the order of equal fractions"""
    chunks = np.asarray(chunks, np.int64)
    base, frac, waves = shares(cols, B, nzc, weight, unit)
    extra = chunks - base
    assert ((extra == 0) | (extra == 1)).all() and (chunks >= 1).all() and (chunks <= nzc).all(), (chunks, base)
    got = extra == 1
    room = base < nzc
    assert not (got & ~room).any()
    if got.any() and (room & ~got).any():
        assert frac[got].min() >= frac[room & ~got].max(), "a chunk went to a smaller fraction"
    total = int((chunks * waves).sum())
    # dealing stops when the tiles have reached B, or when every column with room has had its chunk - and not before
    assert total >= B or not (room & ~got).any(), (total, B)
    if got.any():
        smallest = got & (frac == frac[got].min())
        assert total - int(waves[smallest].max()) < B, "a chunk was dealt after the tiles had reached B"
    else:
        assert int((base * waves).sum()) >= B or not room.any()
    return total


def band(weight, forced_residency, balanced):
    """(fill, lo, hi) a sized plan goes by: the second set only for a weighted plan at the device's own residency"""
    if weight > 0 and not forced_residency:
        return (balanced[0], balanced[1], min(balanced[2], 1.0))
    return (pr.FILL, pr.BAND_LO, pr.BAND_HI)


def plan_chunks(tiles, shape):
    """chunks per column of a plan {seg, yt, z_lo, z_hi}[tiles], in the order of columns(shape)"""
    t = np.asarray(tiles, np.int64)
    out = []
    for yt, xg, waves, _ in columns(shape):
        m = (t[:, 1] == yt) & (t[:, 0] == 4 * xg)
        out.append(int(m.sum()))
    return out
