"""CPU tests of the walk of the block sweep over the live blocks of a plane: mc33_c_library_amd/csrc/mc33_sweep_blocks.h compiled
into a stand-alone host program (tests/sweep_blocks_host.cpp) and held to the restatement below, written from the rules as
DESIGN.md 21 states them, and once more under ASan and UBSan.

The word of a plane of a tile (k_block_verdicts): bits 2 j, 2 j + 1 the code of block j = 4 g + k (row group g, quarter k), j < 16;
bits 32 + 2 g, 33 + 2 g the code of the halo block of row group g.  0: live, 1: all samples below the isovalue, 2: all above.  Code 3
is never written; the header takes it as "not live": below for a block, above for a halo block, and so does the restatement.

Cases: all 4^5 code combinations of one row group (four quarters and the halo block), in every row group, with every number of
row groups and both halo modes, the other groups' bits random; and a few thousand random words, the unused upper bits included."""
import subprocess

import numpy as np
import pytest

from host_program import SANITIZE, build_host_program

NONE = 16
NEG_INF, POS_INF = 0xFF800000, 0x7F800000


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory, "sweep_blocks_host.cpp", [])


@pytest.fixture(scope="module")
def host_program_sanitized(tmp_path_factory):
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer: stand-alone, with its own main"""
    return build_host_program(tmp_path_factory, "sweep_blocks_host.cpp", SANITIZE)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------

def code(w, g, k):
    return (w >> (8 * g + 2 * k)) & 3


def halo_code(w, g):
    return (w >> (32 + 2 * g)) & 3


def live_mask(w, groups, own):
    m = 0
    for g in range(groups):
        for k in range(4):
            if code(w, g, k) == 0:
                m |= 1 << (4 * g + k)
        if own and halo_code(w, g) == 0:   # the halo load rides on the batch of quarter 3
            m |= 1 << (4 * g + 3)
    return m


def next_block(mask, j):
    for b in range(j, 16):
        if (mask >> b) & 1:
            return b
    return NONE


def expected(w, groups, own):
    m = live_mask(w, groups, own)
    out = [m, m, NONE] + [next_block(m, j) for j in range(17)]   # (the walk visits exactly the blocks of the mask and ends with "none")
    for g in range(4):
        out.append(sum(1 << k for k in range(4) if code(w, g, k) == 2))
        out.append({0: 0, 1: NEG_INF}.get(halo_code(w, g), POS_INF))
    return out


# ---- the program ------------------------------------------------------------------------------------------------------------------------

def run(program, tmp_path, cases):
    path = str(tmp_path / "words.txt")
    with open(path, "w") as f:
        for w, groups, own in cases:
            f.write("%x %d %d\n" % (w, groups, own))
    r = subprocess.run([program, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    got = []
    for line in lines:
        t = line.split()
        assert len(t) == 3 + 17 + 8
        got.append([int(t[0], 16), int(t[1], 16)] + [int(x) for x in t[2:20]] + [int(x, 16) for x in t[20:]])
    return got


def check(program, tmp_path, cases):
    got = run(program, tmp_path, cases)
    for c, g in zip(cases, got):
        assert g == expected(*c), ("%x" % c[0], c[1:], g, expected(*c))


def one_group_cases(rng):
    """all 4^5 combinations of the five codes of row group g, for every g; the rest of the word random"""
    cases = []
    for g in range(4):
        for combo in range(4 ** 5):
            w = int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2))
            w &= ~((0xFF << (8 * g)) | (3 << (32 + 2 * g)))
            w |= (combo & 0xFF) << (8 * g) | (combo >> 8) << (32 + 2 * g)
            cases.append((w, 1 + (combo + g) % 4, (combo >> 3) & 1))
    return cases


def test_every_combination_of_one_row_group(host_program, tmp_path):
    rng = np.random.default_rng(20140)
    cases = one_group_cases(rng)
    check(host_program, tmp_path, cases)
    # ... and the same combinations in group 0 of a word with nothing else in it, every row-group count and both halo modes
    plain = [((c & 0xFF) | (c >> 8) << 32, groups, own) for c in range(4 ** 5) for groups in (1, 2, 3, 4) for own in (0, 1)]
    check(host_program, tmp_path, plain)


def test_whole_words(host_program, tmp_path):
    rng = np.random.default_rng(20141)
    words = [0, 0xFFFFFFFFFFFFFFFF, 0x5555555555, 0xAAAAAAAAAA, 0x55555555, 0xAA00000000, 0x00000000AAAAAAAA, 0x40000000, 0x80000001]
    # every block dead but one, at every position; every block live but one
    words += [0x5555555555 & ~(3 << (2 * j)) for j in range(20)] + [1 << (2 * j) for j in range(20)] + [2 << (2 * j) for j in range(20)]
    # words of codes 0 .. 2 only, as k_block_verdicts writes them, at several shares of dead blocks
    for p_dead in (0.1, 0.5, 0.74, 0.95):
        for rep in range(600):
            c = np.where(rng.random(20) < p_dead, rng.integers(1, 3, 20), 0)
            words.append(sum(int(v) << (2 * j) for j, v in enumerate(c)))
    # any 64 bits
    words += [int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2)) for rep in range(2000)]
    cases = [(w, groups, own) for w in words for groups in (1, 2, 3, 4) for own in (0, 1)]
    assert len(cases) > 30000
    check(host_program, tmp_path, cases)
    # the rules themselves, on a word read by hand: group 0 = {live, below, above, below}, halo live; group 1 all above, halo below
    w = (0 | 1 << 2 | 2 << 4 | 1 << 6) | 0xAA << 8 | 1 << 34
    assert expected(w, 2, 0)[0] == 0x1 and expected(w, 2, 1)[0] == 0x9 and expected(w, 1, 1)[0] == 0x9
    assert expected(w, 2, 1)[20:24] == [0x4, 0, 0xF, NEG_INF]
    # the blocks of the row groups the tile does not have are never streamed, whatever their codes
    assert expected(0, 1, 1)[0] == 0xF and expected(0, 3, 0)[0] == 0xFFF


def test_under_the_sanitizers(host_program_sanitized, tmp_path):
    rng = np.random.default_rng(20142)
    check(host_program_sanitized, tmp_path, one_group_cases(rng)[::3])
    words = [0, 0xFFFFFFFFFFFFFFFF] + [int(rng.integers(0, 1 << 63)) << 1 | int(rng.integers(0, 2)) for rep in range(500)]
    check(host_program_sanitized, tmp_path, [(w, groups, own) for w in words for groups in (1, 2, 3, 4) for own in (0, 1)])
