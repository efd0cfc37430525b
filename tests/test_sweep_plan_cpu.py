"""CPU tests of how a sweep's plan shares its tiles out among its columns and of which fill and band a sized plan goes by:
mc33_c_library_amd/csrc/mc33_sweep_plan.h compiled into a stand-alone host program (tests/sweep_plan_host.cpp) and held to the
numpy restatement (tests/sweep_plan_rules.py), and once more under ASan and UBSan.

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

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

BIG, FLAGSHIP, ONE_YT, SHALLOW = (160, 130, 1030), (1024, 1024, 1024), (40, 60, 520), (12, 130, 1030)
WEIGHTS = (0.0, 1.0, 3.5, 4.0, 16.0)


def build(tmp_path_factory, name, flags):
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++"] + HOST_FLAGS + flags + [os.path.join(HERE, "sweep_plan_host.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build(tmp_path_factory, "sweep_plan_host", [])


@pytest.fixture(scope="module")
def host_program_sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: stand-alone, with its own main"""
    return build(tmp_path_factory, "sweep_plan_host_san", SANITIZE)


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
    text = open(os.path.join(HERE, "..", "mc33_c_library_amd", "csrc", "mc33_extract.hip.h")).read()
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
