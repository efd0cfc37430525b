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


# ---- the policy of the sweeps with a range table ("The size of the plan", "A field with a table and little dead
# goes back to the one-round plan") -------------------------------------------------------------------------------------------------

def word(live, tiles, plan):
    """what k_live_compact publishes: live tiles << 32 | tiles << 1 | plan; 0: nothing yet"""
    return (live << 32) | (tiles << 1) | plan


class Facts:
    """what the policy is told of the context and of the range about to be swept (TableFacts, in the order of the struct)"""

    def __init__(self, unit, resident, min_depth=0, weight=0.0, forced=False, rz=0, rz_table=0, table_tiles=0, live=-1, plan_tiles=0, plan_sized=False):
        self.unit, self.resident, self.min_depth, self.weight, self.forced = float(unit), resident, min_depth, float(weight), forced
        self.rz, self.rz_table, self.table_tiles, self.live, self.plan_tiles, self.plan_sized = rz, rz_table, table_tiles, live, plan_tiles, plan_sized

    def line(self):
        return "%r %d %d %r %d %d %d %d %d %d %d" % (self.unit, self.resident, self.min_depth, self.weight, int(self.forced), self.rz, self.rz_table,
                                                    self.table_tiles, self.live, self.plan_tiles, int(self.plan_sized))


class Policy:
    """the state the sweeps with a table go by, as DESIGN.md states the rules; every method returns the decision"""

    def __init__(self):
        self.coarse, self.coarse_sweeps, self.target, self.pending = False, 0, 0, 0

    def state(self):
        return (int(self.coarse), self.coarse_sweeps, self.target, self.pending)

    def plan(self, w):
        """a sweep by the finer plan that found more than 90 % of its tiles live sends the following ones to plan 0; a sweep by
        plan 0 that found fewer than 75 % live sends them back; the one-in-16 counter starts when the stand-in does"""
        tiles, live = (w & 0xFFFFFFFF) >> 1, w >> 32
        if tiles:
            if (w & 1) and 100 * live > 90 * tiles:
                if not self.coarse:
                    self.coarse_sweeps = 0
                self.coarse = True
            elif not (w & 1) and 100 * live < 75 * tiles:
                self.coarse = False
        return 0 if self.coarse else 1

    def retarget(self, w, f):
        """precedence: MC33_HIP_TABLE_TILES, then an explicit depth (left alone), then the sizing by a count of plan 1"""
        if f.table_tiles:
            self.target = f.table_tiles
            return
        tiles, live = (w & 0xFFFFFFFF) >> 1, w >> 32
        if f.rz or f.rz_table or not f.resident or not (w & 1) or not tiles or not live:
            return
        depth = pr.floor_depth(f.unit, f.resident, f.min_depth)
        if depth is None:   # less than one round at the smallest depth
            return
        fill, lo, hi = band(f.weight, f.forced, (FILL_BALANCED, BAND_BALANCED_LO, BAND_BALANCED_HI))
        now = f.plan_tiles if f.plan_tiles else tiles   # the live share scaled to the plan in force
        if pr.keeps(live * now // tiles, f.resident, lo, hi):
            self.pending = 0
            return
        t = pr.target(live, tiles, f.resident, f.unit, depth, fill)
        if not t or t == self.target:
            self.pending = 0
        elif not self.pending or abs(t - self.pending) > 0.05 * self.pending:
            self.pending = t   # a second call has to agree
        else:
            self.pending, self.target = 0, t

    def wants_list(self, f):
        """a plan of at least one round, or a sized plan; while plan 0 stands in, one sweep in 16, the first at once; MC33_HIP_LIVE
        overrides either way (the sweeps are still counted)"""
        want = f.plan_tiles >= 4 * f.resident or f.plan_sized
        if self.coarse:
            want = self.coarse_sweeps % 16 == 0
            self.coarse_sweeps += 1
        return f.live > 0 or (f.live < 0 and want)

    def forget(self):
        """new samples: the finer plan, at its default depth, nothing pending"""
        self.coarse, self.target, self.pending = False, 0, 0
