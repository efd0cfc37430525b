"""CPU tests of the two device-free rules of the sweep with a range table: mc33_c_library_amd/csrc/mc33_sweep_pack.h compiled into a
stand-alone host program (tests/sweep_pack_host.cpp) and held to the numpy restatement (tests/sweep_pack_rules.py) - the order of
the packed live list, block after block and as k_live_compact makes it from two prefix sums over its threads, and the size of the
plan - over random verdict patterns and live counts, and once more under ASan and UBSan."""
import os
import subprocess

import numpy as np
import pytest

import sweep_pack_rules as pr
from host_program import HERE, SANITIZE, build_host_program


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "sweep_pack_host.cpp", [])


@pytest.fixture(scope="module")
def host_program_sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: stand-alone, with its own main"""
    return build_host_program(tmp_path_factory, "sweep_pack_host.cpp", SANITIZE)


def verdict_bytes(dead, grouped):
    n = len(dead)
    nb = (n + 3) // 4
    d = np.ones(nb * 4, bool)
    d[:n] = dead
    v = (d.reshape(nb, 4) * (1 << np.arange(4))).sum(axis=1).astype(np.uint8)
    return v | (np.asarray(grouped, bool)[:nb].astype(np.uint8) << 4)


def run_pack(program, tmp, dead, grouped, threads):
    path = os.path.join(tmp, "verdicts.bin")
    verdict_bytes(dead, grouped).tofile(path)
    r = subprocess.run([program, "pack", path, str(threads)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    n, live = (int(x) for x in lines[0].split())
    e = np.array([[int(x) for x in ln.split()] for ln in lines[1:1 + n]], np.uint32).reshape(n, 4)
    return e, live


def patterns():
    """(name, dead[tiles], grouped[blocks])"""
    rng = np.random.default_rng(33)
    out = []
    for n, p in ((4408, 0.64), (1000, 0.5), (1001, 0.1), (1002, 0.9), (1003, 0.99), (37, 0.5), (4, 0.5), (3, 0.3), (1, 0.0), (12288, 0.641)):
        dead = rng.random(n) < p
        out.append(("random %d %.2f" % (n, p), dead, rng.random((n + 3) // 4) < 0.5))
    # runs, as a smooth field leaves them: whole stretches of blocks dead, live, and mixed ones between
    dead = np.repeat(rng.random(700) < 0.6, 6)[:4093]
    out.append(("runs", dead, np.ones(1024, bool)))
    out.append(("all dead", np.ones(517, bool), np.zeros(130, bool)))
    out.append(("all live", np.zeros(516, bool), np.arange(129) % 3 != 0))
    out.append(("all live, a short last block", np.zeros(518, bool), np.ones(130, bool)))
    one = np.ones(999, bool)
    one[613] = False
    out.append(("one live tile", one, np.ones(250, bool)))
    five = np.ones(64, bool)
    five[[3, 17, 18, 40, 63]] = False
    out.append(("five live tiles", five, np.zeros(16, bool)))
    whole_in_quad = np.ones(32, bool)   # a whole block between the tiles of one quad
    whole_in_quad[[1, 2, 8, 9, 10, 11, 13, 20]] = False
    out.append(("a whole block inside a quad", whole_in_quad, np.ones(8, bool)))
    return out


PATTERNS = patterns()


@pytest.mark.parametrize("case", range(len(PATTERNS)), ids=[p[0] for p in PATTERNS])
def test_packed_order_is_the_rules(host_program, tmp_path, case):
    name, dead, grouped = PATTERNS[case]
    want = pr.packed_entries(dead, grouped)
    pr.check_entries(want, dead)
    for threads in (0, 1, 7, 64, 1024):
        got, live = run_pack(host_program, str(tmp_path), dead, grouped, threads)
        assert live == int((~dead).sum()) and len(got) == (live + 3) // 4, (name, threads)
        assert np.array_equal(got, want), (name, threads)


def test_a_whole_block_comes_behind_the_quad_that_has_begun():
    name, dead, grouped = PATTERNS[-1]
    e = pr.packed_entries(dead, grouped)
    assert e.tolist() == [[1, 2, 13, 20], [8 | pr.GROUP, 9, 10, 11]]
    assert pr.packed_entries(np.ones(8, bool), np.ones(2, bool)).shape == (0, 4)


def run_target(program, live, tiles, resident, unit, min_depth, live_now=None):
    r = subprocess.run([program, "target", str(live), str(tiles), str(resident), repr(float(unit)), repr(float(min_depth)), repr(pr.FILL),
                        repr(pr.BAND_LO), repr(pr.BAND_HI), str(live if live_now is None else live_now)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    t, k = (int(x) for x in r.stdout.split())
    return t, bool(k)


def test_plan_size_is_the_rules(host_program):
    rng = np.random.default_rng(7)
    unit1024 = pr.unit_of((1024, 1024, 1024))
    cases = [(4408, 12288, 1024, unit1024, pr.MIN_DEPTH),   # the flagship's count
             (0, 12288, 1024, unit1024, pr.MIN_DEPTH),      # live = 0: nothing to go by
             (12288, 12288, 1024, unit1024, pr.MIN_DEPTH),  # live = tiles
             (100, 219, 1024, pr.unit_of((40, 70, 1030)), 1.0),  # tiles < one round
             (300, 12288, 1024, unit1024, pr.MIN_DEPTH),    # a target that hits the minimum depth
             (3, 1024, 256, pr.unit_of((160, 130, 1030)), 1.0),
             (5, 0, 1024, unit1024, pr.MIN_DEPTH), (5, 7, 0, unit1024, pr.MIN_DEPTH)]
    for k in range(300):
        tiles = int(rng.integers(1, 200000))
        cases.append((int(rng.integers(0, tiles + 1)), tiles, int(rng.integers(1, 2049)), float(rng.uniform(10.0, 1e6)), float(rng.choice([1.0, 2.0, 3.0, 5.5]))))
    for live, tiles, resident, unit, min_depth in cases:
        t, k = run_target(host_program, live, tiles, resident, unit, min_depth)
        assert t == pr.target(live, tiles, resident, unit, min_depth), (live, tiles, resident, unit, min_depth)
        assert k == pr.keeps(live, resident), (live, resident)
    # the flagship: 4 408 of 12 288 tiles live on 1 024 resident blocks - about 7 760 tiles, whose packed blocks are 0.68 of a round
    t, k = run_target(host_program, 4408, 12288, 1024, unit1024, pr.MIN_DEPTH)
    assert not k and 7720 <= t <= 7800, t
    live_then = round(t * 4408 / 12288)
    assert 0.67 * 1024 <= (live_then + 3) // 4 <= 0.69 * 1024 and run_target(host_program, 4408, 12288, 1024, unit1024, pr.MIN_DEPTH, live_then)[1]
    # the minimum depth: never more tiles than unit / depth, and then fewer packed blocks than a round, never more
    t, _ = run_target(host_program, 300, 12288, 1024, unit1024, pr.MIN_DEPTH)
    assert t == int(unit1024 / pr.MIN_DEPTH) and (round(t * 300 / 12288) + 3) // 4 < pr.BAND_LO * 1024
    # more than the fill live: one round, never less
    assert run_target(host_program, 9830, 12288, 1024, unit1024, pr.MIN_DEPTH)[0] == 4096 and pr.target(9830, 12288, 1024, unit1024) == 4096
    # the band never ends above one round
    assert pr.BAND_HI <= 1.0 and pr.BAND_LO < pr.FILL < pr.BAND_HI
    top = 4 * int(pr.BAND_HI * 1024)
    assert run_target(host_program, 1, 1, 1024, 1.0, 1.0, top)[1] and not run_target(host_program, 1, 1, 1024, 1.0, 1.0, top + 1)[1]


def test_the_librarys_constants_are_the_rules():
    """the constants of table_retarget (mc33_sweep_plan.h) are the ones the restatement and the GPU tests go by"""
    import re
    text = open(os.path.join(HERE, "..", "mc33_c_library_amd", "csrc", "mc33_sweep_plan.h")).read()
    m = re.search(r"TABLE_FILL = ([0-9.]+), TABLE_BAND_LO = ([0-9.]+), TABLE_BAND_HI = ([0-9.]+), TABLE_MIN_DEPTH = ([0-9.]+);", text)
    assert m and tuple(float(x) for x in m.groups()) == (pr.FILL, pr.BAND_LO, pr.BAND_HI, pr.MIN_DEPTH)
    assert re.search(r"SWEEP_DEPTH_TABLE = %du" % int(pr.DEFAULT_DEPTH), text)


def test_under_the_sanitizers(host_program_sanitized, tmp_path):
    for name, dead, grouped in PATTERNS:
        want = pr.packed_entries(dead, grouped)
        for threads in (0, 5, 1024):
            got, live = run_pack(host_program_sanitized, str(tmp_path), dead, grouped, threads)
            assert np.array_equal(got, want), (name, threads)
    assert run_target(host_program_sanitized, 4408, 12288, 1024, pr.unit_of((1024, 1024, 1024)), pr.MIN_DEPTH)[0] > 0
