"""What the GPU tests of the passes over a finished mesh share (measure, topology, filter, smooth, simplify, clip, and property
beside them): arrays to the device and back as bits, a context on a grid, and ONE statement of the canaried
call - every output of a device call sits in a larger tensor whose SPARE rows behind the counted ones are filled with FILL and
must still hold it afterwards.  That check is the suite's only guard against a kernel writing behind its counted rows;
tests/test_mesh_harness_cpu.py holds it to its job on CPU tensors.  The CPU-side helpers of the same tests are in
tests/mesh_checks.py."""
import ctypes as C

import numpy as np
import pytest

SPARE = 16  # canaried rows behind every output
FILL = 0x55


def to_device(a, device="cuda"):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:  # (the shared fixtures are read-only; torch wants to own what it wraps)
        a = a.copy()
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(device)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def words(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def device_grid(data, r0=(0.0, 0.0, 0.0), d=(1.0, 1.0, 1.0), prop=None, **kw):
    from mc33_c_library_amd import DeviceGrid
    g = DeviceGrid(to_device(data), r0=r0, d=d, **kw)
    if prop is not None:
        g.attach_property(to_device(prop))
    return g


def tiny_grid():
    """a context for meshes that come from no grid"""
    return device_grid(np.zeros((4, 4, 4), np.float32))


@pytest.fixture(scope="module")
def ctx():
    """one such context per test module that imports this fixture by name"""
    g = tiny_grid()
    yield g
    g.close()


def once_per_key(make):
    """make(reflibs, *key) is called once per key.  The cache belongs to the function this returns, so to the test module that
    defines it: what a module uploaded lives as long as that module, and no module sees another's tensors."""
    cache = {}

    def cached(reflibs, *key):
        if key not in cache:
            cache[key] = make(reflibs, *key)
        return cache[key]
    cached.__doc__ = make.__doc__
    return cached


class CanariedCall:
    """One device call whose outputs sit inside larger, canaried tensors.  A subclass fills its argument struct, takes its
    outputs from room(), makes the call through call(), and names in outputs() what it allocated; its check() compares with its
    oracle through equal_bits() and ends in spare_intact().  device: "cuda", or "cpu" for a stand-in entry point."""

    def __init__(self, g, device="cuda"):
        self.g, self.device = g, device

    def room(self, rows, width, dtype):
        """rows + SPARE rows of width elements (0: a flat array), every byte at FILL"""
        import torch
        t = torch.empty((rows + SPARE, width) if width else (rows + SPARE,), dtype=dtype, device=self.device)
        t.view(torch.uint8).fill_(FILL)
        return t

    def outputs(self):
        """[(tensor or None, rows the call counted in it)]: here the outputs of a pass that returns a mesh - oV, oN and the
        attributes hold counts[0] rows, oT counts[1], oMap one word per INPUT vertex"""
        nV2, nT2 = self.counts[0], self.counts[1]
        return [(self.oV, nV2), (self.oN, nV2), (self.oT, nT2), (self.oMap, self.nV)] + [(x, nV2) for x in self.oA]

    @staticmethod
    def override(a, change):
        """members of the struct set to something else (the refused calls): a scalar or pointer member by its name, an array
        member (plane, cell) by its name from a sequence, one element of an array member by name + index (attr0, attr_mode1)"""
        for name, value in (change or {}).items():
            if not hasattr(a, name) and name[-1].isdigit():
                getattr(a, name[:-1])[int(name[-1])] = value
            elif isinstance(getattr(a, name), C.Array):
                setattr(a, name, type(getattr(a, name))(*value))
            else:
                setattr(a, name, value)

    def call(self, entry, a, change=None):
        """entry(ctx, &a) with the members in change overridden first; rc and the context's message are kept"""
        self.override(a, change)
        self.a = a
        self.rc = entry(self.g.ctx, C.byref(a))
        self.message = self.g.lib.mc33hip_last_error().decode(errors="replace")

    def host(self, t):
        return t.cpu().numpy()

    def spare_intact(self, written=True):
        """the canaries behind the rows the call may write - behind row 0 when it must write nothing"""
        for t, used in self.outputs():
            if t is not None:
                tail = self.host(t[used if written else 0:]).view(np.uint8)
                assert np.all(tail == FILL), "%d bytes behind the output rows were written" % np.count_nonzero(tail != FILL)

    def all_bytes(self):
        return [self.host(t).tobytes() for t, _ in self.outputs() if t is not None]

    def equal_bits(self, label, got_rows, want):
        """the counted rows of an output against the oracle's array, bit for bit: -0.0 is not 0.0, a NaN equals only itself"""
        got, want = bits(self.host(got_rows)), bits(want)
        assert got.shape == want.shape, "%s: shape %r, oracle %r" % (label, got.shape, want.shape)
        assert np.array_equal(got, want), "%s: %d rows differ" % (label, np.count_nonzero((got != want).reshape(got.shape[0], -1).any(axis=1)))
