"""CPU tests of how a sweep's plan shares its tiles out among its columns, of which fill and band a sized plan goes by, of the
whole planner (plan_slot, plan_tiles) and of the policy of the sweeps with a range table (TablePolicy):
mc33_c_library_amd/csrc/mc33_sweep_plan.h compiled into a stand-alone host program (tests/sweep_plan_host.cpp) and held to the
numpy restatement (tests/sweep_plan_rules.py) and to the plans recorded on the device (tests/golden/sweep_plans.json), and once
more under ASan and UBSan.

Geometries (points z, y, x): BIG = 160 x 130 x 1030 (y tiles of 16, 16 and 1 batches per plane; a group of four segments and a
fifth), the flagship 1024^3 (16 y tiles of 16 batches and one of 4), a grid with a single y tile, and a shallow one whose columns
are asked for more chunks than it has planes.  Targets: one round of the device, the size the fill rule asks for in mid-band, and
the cap at the smallest depth."""
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_pack_rules as pr
import sweep_plan_rules as sp
from host_program import HERE, SANITIZE, build_host_program

BIG, FLAGSHIP, ONE_YT, SHALLOW = (160, 130, 1030), (1024, 1024, 1024), (40, 60, 520), (12, 130, 1030)
WEIGHTS = (0.0, 1.0, 3.5, 4.0, 16.0)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "sweep_plan_host.cpp", [])


@pytest.fixture(scope="module")
def host_program_sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: stand-alone, with its own main"""
    return build_host_program(tmp_path_factory, "sweep_plan_host.cpp", SANITIZE)


def run(program, *args):
    r = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    return r.stdout.split()


def run_shares(program, shape, nzc, B, weight):
    out = [int(x) for x in run(program, "shares", shape[0], shape[1], shape[2], nzc, B, repr(float(weight)))]
    return out[0], out[1:]


def run_old(program, shape, nzc, B):
    out = [int(x) for x in run(program, "old", shape[0], shape[1], shape[2], nzc, B)]
    return out[0], out[1:]


def targets(shape, resident):
    """(one round, mid-band at 0.36 of the tiles live, the cap at the rule's smallest depth) for the whole grid"""
    unit = pr.unit_of(shape)
    depth = pr.floor_depth(unit, resident, 1)
    assert depth is not None, (shape, resident)
    tiles = int(unit / pr.DEFAULT_DEPTH)
    mid = pr.target(int(0.36 * tiles), tiles, resident, unit, depth)
    return (4 * resident, mid, int(unit / depth))


CASES = [(BIG, 256), (FLAGSHIP, 1024), (ONE_YT, 16)]


@pytest.mark.parametrize("shape,resident", CASES, ids=["BIG", "1024^3", "one y tile"])
def test_shares_are_the_rules(host_program, shape, resident):
    cols = sp.columns(shape)
    nzc = shape[0] - 1
    ts = targets(shape, resident)
    assert ts[0] <= ts[1] <= ts[2], ts
    for B in ts:
        old_total, old = run_old(host_program, shape, nzc, B)
        for weight in WEIGHTS:
            total, chunks = run_shares(host_program, shape, nzc, B, weight)
            assert len(chunks) == len(cols) and total == sum(c * col[2] for c, col in zip(chunks, cols))
            assert sp.check_chunks(chunks, cols, B, nzc, weight, unit=4.0) == total
            if weight == 0.0:   # the rule as it stood, chunk for chunk
                assert (total, chunks) == (old_total, old), (shape, B)
            # no column is asked for more chunks than there are planes here (the cap is the grid at one plane per tile, counted in
            # batches, and a weight only moves chunks from the full y tiles to the short one, which is the deepest): the tiles reach
            # the target and overshoot by less than the waves of the last column dealt to
            assert max(chunks) <= nzc and B <= total <= B + 4 * len(cols), (shape, B, weight, total)


@pytest.mark.parametrize("shape,resident,short", [(BIG, 256, 1), (FLAGSHIP, 1024, 4)], ids=["BIG", "1024^3"])
def test_the_short_y_tile_is_no_shallower_than_a_full_one(host_program, shape, resident, short):
    """depth = planes / chunks, so depth of the short y tile / depth of a full one = chunks of a full one / chunks of the short
    one = (16 + w) / (short + w), give or take a chunk of rounding in either"""
    cols = sp.columns(shape)
    nzc = shape[0] - 1
    assert cols[0][3] == 16 and cols[-1][3] == short
    for B in targets(shape, resident):
        for weight in WEIGHTS:
            chunks = run_shares(host_program, shape, nzc, B, weight)[1]
            full, last = chunks[0], chunks[-2 if shape == BIG else -1]   # (BIG: the group of four segments of the last y tile)
            assert last <= full, (shape, B, weight)
            want = (16.0 + weight) / (short + weight)
            lo = (full - 1.0) / (last + 1.0)
            hi = (full + 1.0) / (last - 1.0) if last > 1 else float("inf")   # (a column has at least one chunk)
            assert lo <= want <= hi, (shape, B, weight, full, last, want)
            if weight == 0.0 and last > 1:
                assert full >= 3 * last   # batches alone: the short tile many times as deep
    # the flagship at the size of the fill rule: 35 planes deep by batches alone, about 22 with the measured weight
    t = pr.target(4408, 12288, 1024, pr.unit_of(FLAGSHIP))
    d0 = 1023.0 / run_shares(host_program, FLAGSHIP, 1023, t, 0.0)[1][-1]
    d1 = 1023.0 / run_shares(host_program, FLAGSHIP, 1023, t, 3.5)[1][-1]
    assert 33.0 <= d0 <= 36.0 and 20.0 <= d1 <= 24.0, (d0, d1)


def test_more_chunks_than_planes(host_program):
    """a target above what the grid makes at one plane per tile (MC33_HIP_TABLE_TILES can ask for one; the fill rule's cap
    cannot): columns stop at one chunk per plane, the full y tiles first and, with a weight, the short one too, and the tiles
    fall short of the target"""
    cols = sp.columns(SHALLOW)
    nzc = SHALLOW[0] - 1
    unit = pr.unit_of(SHALLOW)
    for B in (int(1.2 * unit), int(3 * unit), 100000):
        for weight in WEIGHTS:
            total, chunks = run_shares(host_program, SHALLOW, nzc, B, weight)
            assert sp.check_chunks(chunks, cols, B, nzc, weight, unit=4.0) == total
            assert max(chunks) == nzc and total <= sum(nzc * c[2] for c in cols)
            if weight == 0.0:
                assert (total, chunks) == run_old(host_program, SHALLOW, nzc, B)
        assert run_shares(host_program, SHALLOW, nzc, 100000, 3.5)[1] == [nzc] * len(cols)
    # 1.2 units: the full y tiles stop at one chunk per plane, and the chunks they cannot take are NOT handed to the short one,
    # which gets its own share and at most one chunk more - with any weight it stays the deepest
    for weight in WEIGHTS:
        chunks = run_shares(host_program, SHALLOW, nzc, int(1.2 * unit), weight)[1]
        assert chunks[:4] == [nzc] * 4 and max(chunks[4:]) < nzc, (weight, chunks)
    # three units with a weight: the short y tile is asked for more chunks than planes as well (3 x 11 x 17 / 32 > 11)
    assert run_shares(host_program, SHALLOW, nzc, int(3 * unit), 16.0)[1] == [nzc] * len(cols)
    assert max(run_shares(host_program, SHALLOW, nzc, int(3 * unit), 0.0)[1][4:]) < nzc


def library_constants():
    text = open(os.path.join(HERE, "..", "mc33_c_library_amd", "csrc", "mc33_sweep_plan.h")).read()
    m = re.search(r"TABLE_FILL_BALANCED = ([0-9.]+), TABLE_BAND_BALANCED_LO = ([0-9.]+), TABLE_BAND_BALANCED_HI = ([0-9.]+);", text)
    w = re.search(r"PLANE_WEIGHT_BLOCKS = ([0-9.]+);", text)
    assert m and w
    return tuple(float(x) for x in m.groups()), float(w.group(1))


def test_fill_and_band_choice(host_program):
    balanced, weight = library_constants()
    assert weight == sp.PLANE_WEIGHT and balanced == (sp.FILL_BALANCED, sp.BAND_BALANCED_LO, sp.BAND_BALANCED_HI)
    assert weight > 0.0 and balanced[1] < balanced[0] < balanced[2] <= 1.0   # a band never ends above one round
    plain = (pr.FILL, pr.BAND_LO, pr.BAND_HI)
    for second in (balanced, (0.9, 0.8, 1.3)):
        for w in (0.0, weight, 7.0):
            for forced in (0, 1):
                got = tuple(float(x) for x in run(host_program, "band", repr(w), forced, *[repr(x) for x in plain], *[repr(x) for x in second]))
                assert got == sp.band(w, forced, second), (w, forced, second)
                if forced or w == 0.0:   # forced residency, unweighted plans: the constants every sized plan went by
                    assert got == plain
                else:
                    assert got == (second[0], second[1], min(second[2], 1.0))


def test_under_the_sanitizers(host_program_sanitized):
    for shape, resident in CASES:
        cols = sp.columns(shape)
        for B in targets(shape, resident):
            for weight in (0.0, 3.5):
                total, chunks = run_shares(host_program_sanitized, shape, shape[0] - 1, B, weight)
                assert sp.check_chunks(chunks, cols, B, shape[0] - 1, weight, unit=4.0) == total
            assert run_old(host_program_sanitized, shape, shape[0] - 1, B) == run_shares(host_program_sanitized, shape, shape[0] - 1, B, 0.0)
    assert run_shares(host_program_sanitized, SHALLOW, 11, 100000, 3.5)[0] == 11 * 5 * 3
    assert [float(x) for x in run(host_program_sanitized, "band", "3.5", 0, "0.68", "0.62", "0.72", "0.9", "0.8", "1.3")] == [0.9, 0.8, 1.0]


# ---- the planner: plan_slot and plan_tiles ---------------------------------------------------------------------------------------------

GOLDEN = os.path.join(HERE, "golden", "sweep_plans.json")
A_SHAPE = (48, 200, 520)


def run_plan(program, shape, zs, ze, table, target, weight, rz, rz_table, resident, min_depth, rows_per_batch=4):
    """((slot, zs, ze, depth, target, weight), total, tiles [n][4], boundaries [m][5]) - total None: too large for one launch"""
    out = run(program, "plan", shape[1] - 1, (shape[2] - 1 + 255) // 256, rows_per_batch, zs, ze, int(table), target, repr(float(weight)), rz, rz_table, resident, min_depth)
    key = tuple(int(x) for x in out[:5]) + (float(out[5]),)
    if out[6] == "large":
        return key, None, None, None
    total, nt, nb = (int(x) for x in out[6:9])
    v = np.array([int(x) for x in out[9:]], np.int64)
    assert len(v) == 4 * nt + 5 * nb
    return key, total, v[:4 * nt].reshape(nt, 4), v[4 * nt:].reshape(nb, 5)


def check_plan_properties(tiles, bounds, shape, zs, ze, what):
    """what any plan has to be, whatever its size"""
    nseg = (shape[2] - 1 + 255) // 256
    assert (np.diff(tiles[:, 2]) >= 0).all(), (what, "z_lo descends in launch order")
    pairs = []
    for yt, xg, waves, _ in sp.columns(shape):
        cuts = None
        for seg in range(4 * xg, 4 * xg + waves):
            at = np.flatnonzero((tiles[:, 0] == seg) & (tiles[:, 1] == yt))
            mine = tiles[at]
            assert mine[0, 2] == zs and mine[-1, 3] == ze and (mine[1:, 2] == mine[:-1, 3]).all() and (mine[:, 3] > mine[:, 2]).all(), (what, yt, seg, "no partition of the range")
            assert cuts is None or np.array_equal(cuts, mine[:, 2:]), (what, yt, seg, "the segments of a group are cut differently")
            cuts = mine[:, 2:]
            pairs += [(at[k], at[k + 1], mine[k + 1, 2], yt, seg) for k in range(len(at) - 1)]
            if seg > 4 * xg:   # the segments of a group at one chunk are neighbours in the list
                assert np.array_equal(at, prev + 1), (what, yt, seg)
            prev = at
    assert len(tiles) == sum(c * col[2] for c, col in zip(sp.plan_chunks(tiles, shape), sp.columns(shape)))
    assert sorted(pairs) == sorted(tuple(int(x) for x in b) for b in bounds), (what, "boundaries")
    assert (tiles[:, 0] < nseg).all()


def golden_cases():
    import json
    import sweep_plan_sequences as sq
    with open(GOLDEN) as f:
        g = json.load(f)
    seen = set()
    for rec in g["sequences"]:
        shape = sq.BIG if rec["shape"] == "banded 96" else tuple(rec["shape"])
        for at in rec["steps"]:
            if (at, rec["name"]) not in seen:
                seen.add((at, rec["name"]))
                yield rec["name"], shape, rec["env"], g["plans"][at]


def test_planner_makes_the_recorded_plans(host_program):
    """every recorded plan, from the inputs the library had: the recorded resident blocks, the switches of the sequence, the plan
    bit; the target is MC33_HIP_TABLE_TILES where that is set, and otherwise - the count a sweep published is not recorded -
    some target no more than a block of waves per column below the tiles there are (none at all: the plan by its depth)"""
    n = 0
    for name, shape, env, plan in golden_cases():
        want = np.array(plan["tiles"], np.int64).reshape(-1, 4)
        ntiles, resident, bit = plan["info"]
        zs, ze = int(want[:, 2].min()), int(want[:, 3].max())
        rz, rz_table, forced = int(env.get("MC33_HIP_RZ", 0)), int(env.get("MC33_HIP_RZ_TABLE", 0)), int(env.get("MC33_HIP_TABLE_TILES", 0))
        assert bit == 0 or not (rz and not rz_table)
        targets = [forced] if forced and bit else [0] + list(range(max(1, ntiles - 4 * len(sp.columns(shape))), ntiles + 1))
        hit = None
        for target in targets if bit else [0]:
            key, total, tiles, bounds = run_plan(host_program, shape, zs, ze, bit, target, plan["weight"] if target else 0.0, rz, rz_table, resident, 0)
            if total is not None and np.array_equal(tiles, want):
                hit = (key, bounds)
                break
        assert hit, (name, plan["info"], plan["weight"], "the planner does not make this plan")
        key, bounds = hit
        assert key[0] == (0 if not bit else 2 if key[4] else 1) and key[5] == plan["weight"], (name, key)
        assert key[3] == ((rz_table or 5) if bit else (rz or 16))
        check_plan_properties(want, bounds, shape, zs, ze, name)
        n += 1
    assert n >= 20


def by_depth(unit, depth, resident, min_depth=1):
    """the tiles a plan without a target is asked for: whole rounds of the device, or on a small grid one round at most, tiles
    down to min_depth planes deep"""
    pref, one = unit / depth, 4 * resident
    return one * int(pref / one + 0.5) if pref >= one else max(1, min(one, int(unit / min_depth)))


PLAN_CASES = [(BIG, 256, 0, 159), (FLAGSHIP, 1024, 0, 1023), (ONE_YT, 16, 0, 39), (SHALLOW, 256, 0, 11), (A_SHAPE, 1024, 10, 11), (BIG, 256, 16, 159)]


@pytest.mark.parametrize("shape,resident,zs,ze", PLAN_CASES, ids=["BIG", "1024^3", "one y tile", "shallow", "one slice", "sub-range"])
def test_plans_are_the_rule(host_program, shape, resident, zs, ze):
    cols = sp.columns(shape)
    nzc = ze - zs
    unit = pr.unit_of(shape, nzc)
    for weight in (0.0, 3.0):
        for table, target in ((0, 0), (1, 0), (1, 4 * resident), (1, max(1, int(unit / 3.0))), (1, int(3 * unit) + 1)):
            key, total, tiles, bounds = run_plan(host_program, shape, zs, ze, table, target, weight, 0, 0, resident, 0)
            assert key == (2 if target else table, zs, ze, 5 if table else 16, target, weight if target else 0.0)
            assert total == len(tiles) <= 0x3FFFFFFF
            check_plan_properties(tiles, bounds, shape, zs, ze, (shape, table, target, weight))
            B = target if target else by_depth(unit, key[3], resident)
            assert sp.check_chunks(sp.plan_chunks(tiles, shape), cols, B, nzc, key[5], unit=4.0) == total


def test_plan_slot_and_the_launch_limit(host_program):
    # MC33_HIP_RZ alone: one plan, number 0, whatever is asked; with MC33_HIP_RZ_TABLE two again; a weight only with a target
    assert run_plan(host_program, ONE_YT, 0, 39, 1, 77, 3.0, 2, 0, 16, 0)[0] == (0, 0, 39, 2, 0, 0.0)
    assert run_plan(host_program, ONE_YT, 0, 39, 1, 77, 3.0, 2, 1, 16, 0)[0] == (2, 0, 39, 1, 77, 3.0)
    assert run_plan(host_program, ONE_YT, 0, 39, 1, 0, 3.0, 0, 7, 16, 0)[0] == (1, 0, 39, 7, 0, 0.0)
    assert run_plan(host_program, ONE_YT, 0, 39, 0, 77, 3.0, 9, 7, 16, 0)[0] == (0, 0, 39, 9, 0, 0.0)
    assert run_plan(host_program, ONE_YT, 0, 39, 1, 77, -1.0, 0, 0, 16, 0)[0] == (2, 0, 39, 5, 77, 0.0)
    # MC33_HIP_MIN_DEPTH on a small grid: tiles no shallower than that
    t1 = run_plan(host_program, ONE_YT, 0, 39, 0, 0, 0.0, 0, 0, 1024, 1)[1]
    t4 = run_plan(host_program, ONE_YT, 0, 39, 0, 0, 0.0, 0, 0, 1024, 4)[1]
    u = pr.unit_of(ONE_YT)   # (the tiles reach what was asked and overshoot by less than the waves of a column: three here)
    assert int(u) <= t1 < int(u) + 3 and int(u / 4.0) <= t4 < int(u / 4.0) + 3 and t4 < t1
    # more tiles than one launch takes: 2^21 x 2^21 cells a plane, one plane per tile
    wide = (20001, 63 * 4096 + 1, 256 * 4096 + 1)
    assert run_plan(host_program, wide, 0, 20000, 1, 0x3FFFFFFF + 5, 0.0, 0, 0, 1024, 0)[1] is None
    # packed samples: batches of 8 and 16 rows
    for rb in (8, 16):
        key, total, tiles, bounds = run_plan(host_program, BIG, 0, 159, 1, 0, 0.0, 0, 0, 256, 0, rows_per_batch=rb)
        cols = sp.columns(BIG, rb)
        assert sp.check_chunks(sp.plan_chunks(tiles, BIG), cols, by_depth(pr.unit_of(BIG, rows_per_batch=rb), 5, 256), 159, 0.0, unit=float(rb)) == total


# ---- the policy ------------------------------------------------------------------------------------------------------------------------

def run_policy(program, tmp_path, steps):
    """steps: (op, word, Facts); every step through the host program and through the restatement - (decision, state) must agree"""
    path = str(tmp_path / "policy.txt")
    with open(path, "w") as f:
        for op, w, facts in steps:
            f.write("%s %d %s\n" % (op, w, facts.line()))
    out = run(program, "policy", path)
    assert len(out) == 5 * len(steps)
    p = sp.Policy()
    got = []
    for k, (op, w, facts) in enumerate(steps):
        d = {"plan": lambda: p.plan(w), "retarget": lambda: p.retarget(w, facts), "list": lambda: int(p.wants_list(facts)), "forget": p.forget}[op]()
        mine = ("-" if d is None else str(d),) + tuple(str(x) for x in p.state())
        assert tuple(out[5 * k:5 * k + 5]) == mine, (k, op, out[5 * k:5 * k + 5], mine)
        got.append((d, p.state()))
    return got


def test_policy(host_program, host_program_sanitized, tmp_path):
    unit, res = pr.unit_of(FLAGSHIP), 1024
    F = lambda **kw: sp.Facts(unit, res, **kw)   # noqa: E731
    w = sp.word
    for program in (host_program, host_program_sanitized):
        # which plan: plan-1 counts at 91, 90, 89 %; plan-0 counts at 74, 75, 76 %; between the thresholds a field stays where it was sent
        r = run_policy(program, tmp_path, [("plan", w(9000, 10000, 1), F()), ("plan", w(8900, 10000, 1), F()), ("plan", w(9100, 10000, 1), F()),
                                           ("plan", w(7600, 10000, 0), F()), ("plan", w(7500, 10000, 0), F()), ("plan", w(8000, 10000, 1), F()),
                                           ("plan", w(8900, 10000, 0), F()), ("plan", w(7400, 10000, 0), F()), ("plan", w(8000, 10000, 1), F()),
                                           ("plan", 0, F()), ("plan", w(9100, 10000, 0), F())])
        assert [d for d, _ in r] == [1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1]
        # retarget: inside the band a pending size is cleared; outside, the first call only sets pending, a second within 5 % adopts,
        # one beyond 5 % replaces pending and adopts nothing; a target equal to the present one clears pending
        inside, out1, out2, far = w(2785, 4096, 1), w(1474, 4096, 1), w(1500, 4096, 1), w(800, 4096, 1)
        t1, t2, tf = pr.target(1474, 4096, res, unit), pr.target(1500, 4096, res, unit), pr.target(800, 4096, res, unit)
        assert pr.keeps(2785, res) and not pr.keeps(1474, res) and abs(t2 - t1) <= 0.05 * t1 < abs(tf - t2)
        r = run_policy(program, tmp_path, [("retarget", out1, F()), ("retarget", inside, F()), ("retarget", out1, F()), ("retarget", far, F()),
                                           ("retarget", out1, F()), ("retarget", out2, F()), ("retarget", far, F(plan_tiles=4096)),
                                           ("retarget", out2, F())])   # (... and a count that asks for the present target)
        assert [s[2:] for _, s in r] == [(0, t1), (0, 0), (0, t1), (0, tf), (0, t1), (t2, 0), (t2, tf), (t2, 0)]
        # a count of the plan in force inside the band keeps it, whatever plan the word counted
        assert run_policy(program, tmp_path, [("retarget", out1, F(plan_tiles=int(4096 * 2785 / 1474)))])[0][1] == (0, 0, 0, 0)
        # the second fill and band: a weighted plan at the device's own residency
        tb = pr.target(1474, 4096, res, unit, fill=sp.FILL_BALANCED)
        assert run_policy(program, tmp_path, [("retarget", out1, F(weight=3.0))])[0][1][3] == tb != t1
        assert run_policy(program, tmp_path, [("retarget", out1, F(weight=3.0, forced=True))])[0][1][3] == t1
        # left alone: rz, rz_table, no word yet, a plan-0 word, no resident blocks, a grid below one round at the smallest depth
        small = pr.unit_of(ONE_YT)
        for facts, word in ((F(rz=2), out1), (F(rz_table=1), out1), (F(), 0), (F(), w(1474, 4096, 0)), (sp.Facts(unit, 0), out1),
                            (sp.Facts(small, res, 1), out1), (F(), w(0, 4096, 1))):
            assert run_policy(program, tmp_path, [("retarget", word, facts)])[0][1] == (0, 0, 0, 0)
        # ... while a grid that makes one round only at MC33_HIP_MIN_DEPTH is sized down to that depth
        u2 = 4.5 * res * 4
        assert run_policy(program, tmp_path, [("retarget", w(300, 4096, 1), sp.Facts(u2, res, 1))])[0][1][3] == int(u2)
        assert run_policy(program, tmp_path, [("retarget", w(300, 4096, 1), sp.Facts(u2, res, 2))])[0][1][3] == int(u2 / 2)
        # MC33_HIP_TABLE_TILES forces the target, before everything else
        assert run_policy(program, tmp_path, [("retarget", 0, F(table_tiles=777, rz_table=3))])[0][1] == (0, 0, 777, 0)
        # list: at least one round yes, below no unless the plan is sized; MC33_HIP_LIVE overrides
        r = run_policy(program, tmp_path, [("list", 0, F(plan_tiles=4096)), ("list", 0, F(plan_tiles=4095)), ("list", 0, F(plan_tiles=4095, plan_sized=True)),
                                           ("list", 0, F(plan_tiles=4095, live=1)), ("list", 0, F(plan_tiles=8192, live=0))])
        assert [d for d, _ in r] == [1, 0, 1, 1, 0]
        # while coarse exactly sweeps 0, 16, 32 get a list, the first at once; the counter starts over with the next stand-in
        steps = [("plan", w(9100, 10000, 1), F())] + [("list", 0, F(plan_tiles=4096))] * 40 + [("plan", w(7000, 10000, 0), F()), ("plan", w(9100, 10000, 1), F()),
                                                                                             ("list", 0, F(plan_tiles=4096))]
        r = run_policy(program, tmp_path, steps)
        assert [k for k in range(40) if r[1 + k][0]] == [0, 16, 32] and r[40][1][1] == 40 and r[-1] == (1, (1, 1, 0, 0))
        # reset on new samples: the finer plan, target 0, pending 0
        r = run_policy(program, tmp_path, [("plan", w(9100, 10000, 1), F()), ("retarget", 0, F(table_tiles=500)), ("retarget", out1, F()), ("forget", 0, F()), ("plan", 0, F())])
        assert r[2][1] == (1, 0, 500, t1) and r[3][1] == (0, 0, 0, 0) and r[4][0] == 1


def test_planner_under_the_sanitizers(host_program, host_program_sanitized):
    """the same plans from the program built with ASan and UBSan: the vectors of plan_tiles are exactly as long as the plan"""
    for shape, resident, zs, ze in PLAN_CASES[:1] + PLAN_CASES[2:]:
        for table, target, weight in ((0, 0, 0.0), (1, 0, 0.0), (1, 4 * resident, 3.0), (1, 100000, 3.0)):
            args = (shape, zs, ze, table, target, weight, 0, 0, resident, 1)
            a, b = run_plan(host_program, *args), run_plan(host_program_sanitized, *args)
            assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), args
    assert run_plan(host_program_sanitized, (20001, 63 * 4096 + 1, 256 * 4096 + 1), 0, 20000, 1, 0x3FFFFFFF + 5, 0.0, 0, 0, 1024, 0)[1] is None
