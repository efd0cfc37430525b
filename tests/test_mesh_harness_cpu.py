"""tests/mesh_harness.py held to its own job, without a GPU: a stand-in pass on CPU tensors with made-up counts.  The canary
check is what the GPU tests of the mesh passes rely on to see a kernel write behind its counted rows, so here every kind of
output gets one byte changed at its first and at its last spare row, and the check must say so."""
import ctypes as C

import numpy as np
import pytest
import torch

from mesh_harness import SPARE, CanariedCall

SIZES = (0, 1, 17)
KINDS = ("oV", "oN", "oT", "attribute", "oMap")


class Args(C.Structure):
    _fields_ = [("oV", C.c_void_p), ("nV", C.c_ulonglong), ("mode", C.c_int), ("plane", C.c_double * 4), ("attr", C.c_void_p * 2), ("attr_mode", C.c_int * 2)]


class Context:
    """what a call needs of a DeviceGrid: ctx, and a library that keeps the last message"""
    ctx = None

    def __init__(self):
        self.lib, self.said = self, b""

    def mc33hip_last_error(self):
        return self.said

    def entry(self, ctx, ref):
        self.said = b"mode %d" % ref._obj.mode
        return -ref._obj.mode


class Stand(CanariedCall):
    """n input vertices; n vertices and n triangles counted; the counted rows are written unless write is False"""

    def __init__(self, n, v=torch.float32, without=(), write=True, change=None):
        super().__init__(Context(), device="cpu")
        self.nV = n
        self.oV, self.oT = self.room(n, 3, v), self.room(n, 3, torch.int32)
        self.oN = None if "oN" in without else self.room(n, 3, torch.float32)
        self.oMap = None if "oMap" in without else self.room(n, 0, torch.int32)
        self.oA = [self.room(n, 0, torch.int32) for _ in range(2)]
        a = Args(self.oV.data_ptr(), n, 0, (C.c_double * 4)(0.0, 0.0, 1.0, 0.0))
        self.call(self.g.entry, a, change)
        self.counts = (n, n)
        if write:
            for t, used in self.outputs():
                if t is not None:
                    t[:used] = 1
        self.of = {"oV": self.oV, "oN": self.oN, "oT": self.oT, "attribute": self.oA[1], "oMap": self.oMap}


def flip(t, row, byte):
    t.view(torch.uint8).reshape(t.shape[0], -1)[row, byte] ^= 0xFF


def refused(call, **kw):
    with pytest.raises(AssertionError) as e:
        call.spare_intact(**kw)
    return str(e.value)


@pytest.mark.parametrize("n", SIZES)
def test_untouched_outputs_pass(n):
    Stand(n).spare_intact()
    Stand(n, v=torch.float64).spare_intact()
    Stand(n, write=False).spare_intact(written=False)
    call = Stand(n)
    assert all(t.shape[0] == n + SPARE for t, _ in call.outputs()) and len(call.all_bytes()) == 6


@pytest.mark.parametrize("kind", KINDS)
def test_one_byte_behind_the_counted_rows_fails_with_the_count(kind):
    for n in SIZES:
        for row, byte in ((n, 0), (n + SPARE - 1, -1)):  # the first spare row - exactly row `used` - and the last
            call = Stand(n)
            flip(call.of[kind], row, byte)
            assert refused(call).startswith("1 bytes behind the output rows"), (kind, n, row)
        two = Stand(n)
        flip(two.of[kind], n, 0)
        flip(two.of[kind], n + 3, 1)
        assert refused(two).startswith("2 bytes ")
    # the last counted row is the call's to write: FILL there is no finding, and neither is anything else
    call = Stand(17)
    call.of[kind][16] = 0
    call.spare_intact()


def test_written_false_checks_from_row_0():
    call = Stand(17, write=False)
    call.spare_intact(written=False)
    flip(call.oT, 0, 0)
    call.spare_intact()  # (row 0 is a counted row)
    assert refused(call, written=False).startswith("1 bytes ")
    full = Stand(1)  # its one row of every output is written
    assert refused(full, written=False).startswith("12 bytes ")  # (oV comes first: three floats 1.0, no byte of them 0x55)


def test_an_output_that_is_none_is_passed_over_and_hides_no_other():
    call = Stand(17, without=("oN", "oMap"))
    assert call.oN is None and call.oMap is None and len(call.all_bytes()) == 4
    call.spare_intact()
    for kind in ("oV", "oT", "attribute"):  # those before and those behind the missing ones in outputs()
        call = Stand(17, without=("oN", "oMap"))
        flip(call.of[kind], 17, 0)
        assert refused(call).startswith("1 bytes ")


@pytest.mark.parametrize("real,word", [(np.float32, np.uint32), (np.float64, np.uint64)])
def test_equal_bits_compares_bits(real, word):
    call = Stand(1)
    nan = np.array([np.nan], real).view(word)[0]
    want = np.array([[0.0, 1.5, 0.0], [-0.0, 2.5, 0.0]], real)
    want.view(word)[:, 2] = (nan, nan | word(1))  # two NaNs of different payload
    same = torch.from_numpy(want.copy())
    call.equal_bits("equal", same, want)
    call.equal_bits("no rows", same[:0], want[:0])
    for row, col, other in ((1, 0, 0.0), (0, 0, -0.0)):  # -0.0 against 0.0, either way round
        got = want.copy()
        got[row, col] = other
        assert np.array_equal(got[:, :2], want[:, :2])  # (as numbers they are equal)
        with pytest.raises(AssertionError, match="zero: 1 rows differ"):
            call.equal_bits("zero", torch.from_numpy(got), want)
    got = want.copy()
    got.view(word)[0, 2] = nan | word(1)
    with pytest.raises(AssertionError, match="payload: 1 rows differ"):
        call.equal_bits("payload", torch.from_numpy(got), want)
    with pytest.raises(AssertionError, match="short"):
        call.equal_bits("short", same[:1], want)
    # indices: the device's int32 rows against the oracle's uint32
    T = np.array([[0, 1, 0xFFFFFFFF]], np.uint32)
    call.equal_bits("oT", torch.from_numpy(T.view(np.int32).copy()), T)


def test_all_bytes_sees_every_byte_of_every_output():
    for n in (1, 17):
        base = Stand(n).all_bytes()
        assert Stand(n).all_bytes() == base
        for kind in KINDS:
            t = Stand(n).of[kind]
            rows, width = t.shape[0], t.view(torch.uint8).reshape(t.shape[0], -1).shape[1]
            where = [(r, b) for r in range(rows) for b in range(width)] if n == 1 else [(0, 0), (n - 1, width - 1), (n, 0), (rows - 1, width - 1)]
            for row, byte in where:
                call = Stand(n)
                flip(call.of[kind], row, byte)
                assert call.all_bytes() != base, (kind, row, byte)


def test_change_reaches_scalars_arrays_and_indexed_members():
    plain = Stand(1)
    assert (plain.rc, plain.message, plain.a.nV, list(plain.a.plane)) == (0, "mode 0", 1, [0.0, 0.0, 1.0, 0.0])
    assert plain.a.oV == plain.oV.data_ptr() and list(plain.a.attr) == [None, None]
    call = Stand(1, change=dict(mode=22, nV=1 << 32, oV=None, plane=(1.0, -2.0, float("inf"), 4.0), attr0=1234, attr_mode1=-1))
    a = call.a
    assert (call.rc, call.message) == (-22, "mode 22")  # the struct was changed BEFORE the call
    assert (a.mode, a.nV, a.oV) == (22, 1 << 32, None) and list(a.plane) == [1.0, -2.0, float("inf"), 4.0]
    assert list(a.attr) == [1234, None] and list(a.attr_mode) == [0, -1]
    assert Stand(1, change=dict(attr1=77)).a.attr[1] == 77
    with pytest.raises(AttributeError):
        Stand(1, change=dict(no_such_member=1))
