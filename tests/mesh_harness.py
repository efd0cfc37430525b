"""What the GPU tests of the passes over a finished mesh share (measure, topology, filter, smooth, simplify, clip, and property
beside them): arrays to the device and back as bits, a context on a grid, and ONE statement of the canaried
call - every output of a device call sits in a larger tensor whose SPARE rows behind the counted ones are filled with FILL and
must still hold it afterwards.  That check is the suite's only guard against a kernel writing behind its counted rows;
tests/test_mesh_harness_cpu.py holds it to its job on CPU tensors.  The CPU-side helpers of the same tests are in
tests/mesh_checks.py."""
import ctypes as C

import numpy as np
import pytest

import clip_oracle as co
import simplify_oracle as sp
import smooth_oracle as so
from mc33_capi import MC33Lib, product_path

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


def capi(dtype="f32", nneg=False):
    """a sample type's product library through the C API of marching_cubes_33.h, every prototype declared (tests/mc33_capi.py)"""
    return MC33Lib(product_path(dtype, nneg=nneg), dtype)


def palette(n):
    """n distinct 0xAABBGGRR words, some with the top bit set"""
    return [int((0xff000000 if k % 2 else 0x7f000000) | ((k * 2654435761) & 0xffffff)) for k in range(n)]


def as_i32(words):
    return np.array([w & 0xFFFFFFFF for w in words], np.uint32).view(np.int32)


def c_palette(words):
    return (C.c_int * len(words))(*[int(x) for x in as_i32(words)])


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


class ClipCall(CanariedCall):
    """one mc33hip_clip_surface call; the default capacities are the ones that are always enough: nV + 2 nT rows, 2 nT triangles"""

    def __init__(self, g, V, N, T, plane, attrs=(), modes=(), capV=None, capT=None, with_map=True, with_normals=True, change=None):
        import torch
        from mc33_c_library_amd.api import Clipping
        super().__init__(g)
        self.nV, self.nT = V.shape[0], T.shape[0]
        self.capV = self.nV + 2 * self.nT if capV is None else capV
        self.capT = 2 * self.nT if capT is None else capT
        with_normals = with_normals and N is not None
        self.oV, self.oT = self.room(self.capV, 3, V.dtype), self.room(self.capT, 3, torch.int32)
        self.oN = self.room(self.capV, 3, torch.float32) if with_normals else None
        self.oA = [self.room(self.capV, 0, torch.int32) for _ in attrs]
        self.oMap = self.room(self.nV, 0, torch.int32) if with_map else None
        a = Clipping()
        a.V, a.N, a.T, a.nV, a.nT = V.data_ptr(), (N.data_ptr() if N is not None else None), T.data_ptr(), self.nV, self.nT
        for k, x in enumerate(attrs):
            a.attr[k], a.oAttr[k] = x.data_ptr(), self.oA[k].data_ptr()
            a.attr_mode[k] = int(modes[k]) if k < len(modes) else co.COPY
        a.n_attr = len(attrs)
        a.plane = (C.c_double * 4)(*plane)
        a.oV, a.oT, a.capV, a.capT = self.oV.data_ptr(), self.oT.data_ptr(), self.capV, self.capT
        a.oN = self.oN.data_ptr() if with_normals else None
        a.oMap = self.oMap.data_ptr() if with_map else None
        self.keep = (V, N, T, attrs)
        self.call(g.lib.mc33hip_clip_surface, a, change)
        self.counts = tuple(int(getattr(a, n)) for n in co.Clipped.COUNTS)

    def check(self, want):
        """bit for bit against the oracle"""
        assert self.counts == want.counts(), (self.counts, want.counts())
        nV2, nT2 = want.nV_out, want.nT_out
        self.equal_bits("oV", self.oV[:nV2], want.V)
        self.equal_bits("oT", self.oT[:nT2], want.T)
        if self.oN is not None:
            self.equal_bits("oN", self.oN[:nV2], want.N)
        assert len(self.oA) == len(want.attrs)
        for k, x in enumerate(self.oA):
            self.equal_bits("attribute %d" % k, x[:nV2], want.attrs[k])
        if self.oMap is not None:
            self.equal_bits("oMap", self.oMap[:self.nV], want.vmap)
        self.spare_intact()


class CompactCall(CanariedCall):
    """one mc33hip_compact_components call"""

    def __init__(self, g, V, N, T, labels, roots, invert=False, attrs=(), capV=None, capT=None, with_map=True):
        import torch
        from mc33_c_library_amd.api import Compaction
        super().__init__(g)
        self.nV, self.nT = V.shape[0], T.shape[0]
        self.capV = self.nV if capV is None else capV
        self.capT = self.nT if capT is None else capT
        self.oV, self.oN, self.oT = self.room(self.capV, 3, V.dtype), self.room(self.capV, 3, torch.float32), self.room(self.capT, 3, torch.int32)
        self.oA = [self.room(self.capV, 0, torch.int32) for _ in attrs]
        self.oMap = self.room(self.nV, 0, torch.int32) if with_map else None
        roots = np.ascontiguousarray(np.asarray(roots).reshape(-1), dtype=np.uint32)
        a = Compaction()
        a.V, a.N, a.T, a.label, a.nV, a.nT = V.data_ptr(), N.data_ptr(), T.data_ptr(), labels.data_ptr(), self.nV, self.nT
        for k, x in enumerate(attrs):
            a.attr[k], a.oAttr[k] = x.data_ptr(), self.oA[k].data_ptr()
        a.n_attr, a.invert = len(attrs), int(bool(invert))
        a.roots, a.n_roots = (roots.ctypes.data if roots.size else None), roots.size
        a.oV, a.oN, a.oT, a.capV, a.capT = self.oV.data_ptr(), self.oN.data_ptr(), self.oT.data_ptr(), self.capV, self.capT
        a.oMap = self.oMap.data_ptr() if with_map else None
        self.keep = (V, N, T, labels, attrs, roots)
        self.call(g.lib.mc33hip_compact_components, a)
        self.counts = (int(a.nV_out), int(a.nT_out), int(a.components_kept))

    def check(self, want):
        """bit for bit against the oracle"""
        assert self.counts == (want.nV_out, want.nT_out, want.components_kept), (self.counts, (want.nV_out, want.nT_out, want.components_kept))
        nV2, nT2 = want.nV_out, want.nT_out
        self.equal_bits("oV", self.oV[:nV2], want.V)
        self.equal_bits("oN", self.oN[:nV2], want.N)
        self.equal_bits("oT", self.oT[:nT2], want.T)
        for k, x in enumerate(self.oA):
            self.equal_bits("attribute %d" % k, x[:nV2], want.attrs[k])
        if self.oMap is not None:
            self.equal_bits("oMap", self.oMap[:self.nV], want.vmap)
        self.spare_intact()


def normals_of(want):
    return so.vertex_normals(want.V, want.T) if want.nV_out else np.zeros((0, 3), np.float32)


class SimplifyCall(CanariedCall):
    """one mc33hip_simplify_surface call"""

    def __init__(self, g, V, T, cell, origin=(0.0, 0.0, 0.0), mode=sp.MEAN, drop=True, attrs=(), capV=None, capT=None, with_map=True, with_normals=True, change=None):
        import torch
        from mc33_c_library_amd.api import Simplification
        super().__init__(g)
        self.nV, self.nT = V.shape[0], T.shape[0]
        self.capV = self.nV if capV is None else capV
        self.capT = self.nT if capT is None else capT
        self.oV, self.oT = self.room(self.capV, 3, V.dtype), self.room(self.capT, 3, torch.int32)
        self.oN = self.room(self.capV, 3, torch.float32) if with_normals else None
        self.oA = [self.room(self.capV, 0, torch.int32) for _ in attrs]
        self.oMap = self.room(self.nV, 0, torch.int32) if with_map else None
        a = Simplification()
        a.V, a.T, a.nV, a.nT = V.data_ptr(), T.data_ptr(), self.nV, self.nT
        for k, x in enumerate(attrs):
            a.attr[k], a.oAttr[k] = x.data_ptr(), self.oA[k].data_ptr()
        a.n_attr = len(attrs)
        a.origin, a.cell = (C.c_double * 3)(*origin), (C.c_double * 3)(*cell)
        a.mode, a.drop_duplicates = int(mode), int(bool(drop))
        a.oV, a.oT, a.capV, a.capT = self.oV.data_ptr(), self.oT.data_ptr(), self.capV, self.capT
        a.oN = self.oN.data_ptr() if with_normals else None
        a.oMap = self.oMap.data_ptr() if with_map else None
        self.keep = (V, T, attrs)
        self.call(g.lib.mc33hip_simplify_surface, a, change)
        self.counts = tuple(int(getattr(a, n)) for n in sp.Simplified.COUNTS)

    def check(self, want, attrs=()):
        """bit for bit against the oracle; attrs: the input words on the host"""
        assert self.counts == want.counts(), (self.counts, want.counts())
        nV2, nT2 = want.nV_out, want.nT_out
        self.equal_bits("oV", self.oV[:nV2], want.V)
        self.equal_bits("oT", self.oT[:nT2], want.T)
        if self.oN is not None:
            self.equal_bits("oN", self.oN[:nV2], normals_of(want))
        for k, x in enumerate(self.oA):
            self.equal_bits("attribute %d" % k, x[:nV2], np.asarray(attrs[k])[want.keep])
        if self.oMap is not None:
            self.equal_bits("oMap", self.oMap[:self.nV], want.vmap)
        self.spare_intact()


def check_python(got, want):
    """what DeviceGrid.compact_components returned against the oracle, bit for bit"""
    V2, N2, T2, attrs2, vmap, kept = got
    assert (V2.shape[0], T2.shape[0], kept) == (want.nV_out, want.nT_out, want.components_kept)
    assert np.array_equal(bits(V2.cpu().numpy()), bits(want.V)) and np.array_equal(bits(N2.cpu().numpy()), bits(want.N))
    assert np.array_equal(T2.cpu().numpy().view(np.uint32), want.T) and np.array_equal(vmap.cpu().numpy().view(np.uint32), want.vmap)
    for x, w in zip(attrs2, want.attrs):
        assert np.array_equal(bits(x.cpu().numpy()), bits(w))


def info_of(A):
    """the four counts mc33hip_smooth_surface fills"""
    return (A.max_degree, A.isolated_vertices, A.boundary_vertices, A.invalid_triangles)
