"""GPU tests of the FACE records (cells on the grid's x / y / z = 0 faces finished by k_cells) and of the tails that
leave the slow kernels out when the last extraction had no cell with a corner equal to the isovalue (a miss repeats the tail with
them): every result bit-identical to the unmodified reference (oracle/_ref)."""
import ctypes as C

import numpy as np
import pytest

from parity import assert_surface_parity

pytestmark = pytest.mark.gpu


def face_field(nx=33, ny=65, nz=17):
    """A smooth field whose surface crosses all three 0-faces (and the far ones) many times."""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.sin(0.61 * x + 0.3) + np.sin(0.37 * y + 1.1) + np.sin(0.83 * z + 0.7) + 0.05 * np.cos(0.29 * x * y / 7.0)


def scaled(f, dtype):
    if dtype == "u16":
        return np.round((f + 3.2) * 9000.0).astype(np.uint16), 28800.5
    if dtype == "f64":
        return f.astype(np.float64), 0.1
    return f.astype(np.float32), 0.1


@pytest.mark.parametrize("dtype", ["f32", "u16", "f64"])
def test_face_heavy_grid_bit_identical(products, reflibs, dtype):
    if dtype not in reflibs:
        pytest.skip("no reference build for %s" % dtype)
    data, iso = scaled(face_field(), dtype)
    got = products[dtype].isosurface(data, iso)
    ref = reflibs[dtype].isosurface(data, iso)
    assert got.nT > 1000
    assert_surface_parity(got, ref, 65.0, "face grid %s" % dtype, bit_exact=True)
    # the surface does reach every 0-face
    V = ref.V.astype(np.float64)
    for ax in range(3):
        assert np.any(V[:, ax] < 1.0), "axis %d: no vertex next to the 0-face" % ax


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 5), (5, 9, 2), (17, 3, 4)])
def test_tiny_grids_all_faces(products, reflibs, shape):
    """Grids so small that every cell is a face cell (or nearly)."""
    nx, ny, nz = shape
    rng = np.random.default_rng(nx * 100 + ny * 10 + nz)
    data = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    got = products["f32"].isosurface(data, 0.05)
    ref = reflibs["f32"].isosurface(data, 0.05)
    assert_surface_parity(got, ref, 20.0, "tiny %s" % (shape,), bit_exact=True)


def uchar_grid():
    """uchar samples around 100: at isovalue 100.0 many corners equal it (slow cells with aliases), at 100.5 none do."""
    z, y, x = np.meshgrid(np.arange(40), np.arange(36), np.arange(44), indexing="ij")
    f = 100.0 + 6.0 * np.sin(0.3 * x + 0.2) * np.cos(0.27 * y) + 4.0 * np.sin(0.41 * z + 0.5)
    return np.clip(np.round(f), 0, 255).astype(np.uint8)


class OneContext:
    """create_MC33 once, then any sequence of size_of_isosurface / calculate_isosurface on it (the reference's C API)."""

    def __init__(self, lib, data):
        self.lib = lib
        self.G, self.keep = lib.make_grid(data)
        self.M = lib.lib.create_MC33(self.G)
        assert self.M

    def size(self, iso):
        nV, nT = C.c_uint(0), C.c_uint(0)
        self.lib.lib.size_of_isosurface(self.M, self.lib.real(iso), C.byref(nV), C.byref(nT))
        return nV.value, nT.value

    def surface(self, iso):
        S = self.lib.lib.calculate_isosurface(self.M, self.lib.real(iso))
        assert S
        try:
            return self.lib.copy_surface(S)
        finally:
            self.lib.lib.free_surface_memory(S)

    def close(self):
        self.lib.lib.free_MC33(self.M)
        self.lib.lib.free_memory_grd(self.G)


def test_alias_flip_on_one_context(products, reflibs):
    """100.5 (no corner equal to it: the tails after the first leave the slow kernels out) -> 100.0 (many: a miss, the tail again
    with them) -> 100.5 -> 100.0 -> 100.5, a count and an extraction each, all on ONE context."""
    if "u8" not in reflibs:
        pytest.skip("no reference build for u8")
    data = uchar_grid()
    assert np.any(data == 100)
    seq = [100.5, 100.5, 100.0, 100.5, 100.0, 100.0, 100.5]
    got_ctx, ref_ctx = OneContext(products["u8"], data), OneContext(reflibs["u8"], data)
    try:
        for k, iso in enumerate(seq):
            assert got_ctx.size(iso) == ref_ctx.size(iso), "step %d iso %g: sizes" % (k, iso)
            got, ref = got_ctx.surface(iso), ref_ctx.surface(iso)
            assert got.nT > 0
            assert_surface_parity(got, ref, 64.0, "flip step %d iso %g" % (k, iso), bit_exact=True)
            # an extraction without a count before it
            got, ref = got_ctx.surface(iso), ref_ctx.surface(iso)
            assert_surface_parity(got, ref, 64.0, "flip step %d iso %g (again)" % (k, iso), bit_exact=True)
    finally:
        got_ctx.close()
        ref_ctx.close()


def test_alias_flip_device_extract(reflibs):
    """The same flip through the device-level call (mc33hip_extract on torch memory) on one DeviceGrid."""
    if "u8" not in reflibs:
        pytest.skip("no reference build for u8")
    import torch
    from mc33_c_library_amd import DeviceGrid
    data = uchar_grid()
    g = DeviceGrid(torch.from_numpy(data).to("cuda:0"))
    for k, iso in enumerate([100.5, 100.5, 100.0, 100.5, 100.0, 100.5]):
        V, N, T, cnt = g.extract(iso)
        ref = reflibs["u8"].isosurface(data, iso)
        assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT), "step %d iso %g" % (k, iso)
        assert np.array_equal(T.cpu().numpy().view(np.uint32).reshape(-1, 3), ref.T), "step %d iso %g: triangles" % (k, iso)
        assert np.array_equal(V.cpu().numpy().reshape(-1, 3).view(np.uint32), ref.V.view(np.uint32)), "step %d iso %g: vertices" % (k, iso)
