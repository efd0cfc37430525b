"""k_cells with ONE block (MC33_HIP_CELLS_BLOCKS=1): its four waves walk the whole list of slices with cut cells, each taking
slice after slice, so every hand-over of a wave from one slice to the next - its LDS record written again, header, record range
and plane rows of another slot - is exercised, which the default grid (as many blocks as the device holds, times four) hardly
does on a test-sized grid.  Smooth slices (compact planes), noise (raw planes: the second round trip), the two alternating
along z (the two planes of a slice differ in format), and a list of one slice.  Every array is compared bit for bit with the
reference built into oracle/_ref."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

NX, NY, NZ = 300, 130, 24


def smooth():
    x, y, z = np.cos(np.linspace(-7.0, 7.0, NX)), np.cos(np.linspace(-4.0, 4.0, NY)), np.cos(np.linspace(-2.0, 2.0, NZ))
    return ((x[None, None, :] + y[None, :, None]) + z[:, None, None]).astype(np.float32)


def noise():
    return fx.noise_f32(0, 11, shape=(NZ, NY, NX))


def halves():
    """smooth and noise planes in turn: the two planes of a slice differ in format, from slice to slice the other way round"""
    d = smooth()
    d[1::2] = noise()[1::2]
    return d


def one_slice():
    """one sample above the isovalue, in the grid's first plane: the cut cells lie in one slice of one row segment"""
    d = np.full((NZ, NY, NX), -1.0, dtype=np.float32)
    d[0, 70, 280] = 1.0
    return d


@pytest.mark.parametrize("make", [smooth, noise, halves, one_slice], ids=lambda f: f.__name__)
def test_one_block_walks_every_slice(make, reflibs, monkeypatch):
    import torch
    from mc33_c_library_amd import DeviceGrid
    monkeypatch.setenv("MC33_HIP_CELLS_BLOCKS", "1")  # (read when the context is created)
    data = make()
    ref = reflibs["f32"].isosurface(data, 0.0)
    assert ref.nT > 0
    g = DeviceGrid(torch.from_numpy(data).cuda())
    for _ in range(2):  # (the second extraction: the list, the headers and the record arrays of the first are still there)
        V, N, T, cnt = g.extract(0.0)
        assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
        assert np.array_equal(T.cpu().numpy().view(np.uint32), ref.T)
        assert np.array_equal(V.cpu().numpy().view(np.uint32), ref.V.view(np.uint32))
        n, nan = N.cpu().numpy(), np.isnan(ref.N)
        assert np.array_equal(np.isnan(n), nan) and np.array_equal(n[~nan].view(np.uint32), ref.N[~nan].view(np.uint32))
    g.close()
