"""The halo column of k_sweep - the first sample of the next row segment, one per row - is loaded under a lane condition by the
waves that need it and not at all by the three waves of a grouped block that take its bits from the wave to their right
(mc33_sweep.hip.h, single-isovalue forms).  Grids with a grouped block and an ungrouped segment behind it (1030 wide), with the
grouped block alone (1024) and with ungrouped segments only (300), two y tiles of 63 + 7 rows; fields whose surface lies on a
segment border and whose halo-column sample equals the isovalue.  Bit for bit against the reference built into oracle/_ref."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY, NZ = 70, 20
WIDTHS = (1030, 1024, 300)


def cos_f32(nx):
    x, y, z = np.cos(np.linspace(-20.0, 20.0, nx)), np.cos(np.linspace(-4.0, 4.0, NY)), np.cos(np.linspace(-2.0, 2.0, NZ))
    return ((x[None, None, :] + y[None, :, None]) + z[:, None, None]).astype(np.float32)


def ramp_f32(nx, at):
    """x - at: the surface is the plane x = at"""
    return np.broadcast_to((np.arange(nx, dtype=np.float64) - at).astype(np.float32), (NZ, NY, nx)).copy()


def cos_u16(nx):
    f = cos_f32(nx).astype(np.float64)
    return np.rint(32768.0 + 10000.0 * f).astype(np.uint16)


def ramp_u16(nx):
    return np.broadcast_to(np.arange(nx, dtype=np.uint16), (NZ, NY, nx)).copy()


def f32_cases():
    for nx in WIDTHS:
        yield pytest.param("f32", lambda nx=nx: cos_f32(nx), 0.0, id="f32-cos-%d" % nx)
        for at in (255.5, 256.0, 1023.0):
            if at < nx - 1 or (at == 1023.0 and nx >= 1024):
                yield pytest.param("f32", lambda nx=nx, at=at: ramp_f32(nx, at), 0.0, id="f32-x-%g-%d" % (at, nx))


def u16_cases():
    for nx in WIDTHS:
        yield pytest.param("u16", lambda nx=nx: cos_u16(nx), 32768.5, id="u16-cos-%d" % nx)
        for at in (255.5, 256.0, 1023.0):
            if at < nx - 1 or (at == 1023.0 and nx >= 1024):
                yield pytest.param("u16", lambda nx=nx: ramp_u16(nx), at, id="u16-x-%g-%d" % (at, nx))


def narrow_and_wide_cases():
    """the other two sample types whose single-isovalue sweep has the lane condition: uchar (four samples per load) and uint, on the
    grid with a grouped block and an ungrouped segment behind it.  A column of steps along x - the surface on the border of the
    first two segments, then with the halo-column sample equal to the isovalue - and a smooth field"""
    nx = 1030
    step = lambda dt: np.broadcast_to(np.where(np.arange(nx) < 256, 10, 20).astype(dt), (NZ, NY, nx)).copy()
    for dt, name in ((np.uint8, "u8"), (np.uint32, "u32")):
        yield pytest.param(name, lambda dt=dt: step(dt), 15.5, id="%s-step-15.5-%d" % (name, nx))
        yield pytest.param(name, lambda dt=dt: step(dt), 20.0, id="%s-step-20-%d" % (name, nx))
        yield pytest.param(name, lambda dt=dt: np.rint(128.0 + 40.0 * cos_f32(nx).astype(np.float64)).astype(dt), 128.5, id="%s-cos-%d" % (name, nx))


@pytest.mark.parametrize("dtype,make,iso", list(f32_cases()) + list(u16_cases()) + list(narrow_and_wide_cases()))
def test_halo_column(dtype, make, iso, reflibs):
    import torch
    from mc33_c_library_amd import DeviceGrid
    data = make()
    ref = reflibs[dtype].isosurface(data, iso)
    t = torch.from_numpy(data.view({"u16": np.int16, "u32": np.int32}.get(dtype, data.dtype))).cuda()
    g = DeviceGrid(t)
    V, N, T, cnt = g.extract(iso)
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
    assert np.array_equal(T.cpu().numpy().view(np.uint32), ref.T)
    assert np.array_equal(V.cpu().numpy().view(np.uint32), ref.V.view(np.uint32))
    n, nan = N.cpu().numpy(), np.isnan(ref.N)
    assert np.array_equal(np.isnan(n), nan) and np.array_equal(n[~nan].view(np.uint32), ref.N[~nan].view(np.uint32))
    g.close()
