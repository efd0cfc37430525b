"""What the CPU and the GPU tests of the smoothing share (tests/test_smooth_cpu.py, tests/test_gpu_smooth.py): the figures of
the fixture rows and the reference's surface of a row with its adjacency and smoothed copies, made once."""
import smooth_oracle as so
from mesh_checks import reference_mesh

# fixture -> max_degree, isolated, boundary_vertices, area before, after 10 iterations (0.5, -0.53) pinned, not pinned
TABLE = {
    "sphere": (9, 0, 0, 12.5617, 12.5646, 12.5646),
    "blobs": (9, 0, 0, 759.1933, 761.8437, 761.8437),
    "sheet": (9, 0, 720, 150.2069, 150.2014, 148.4636),
    "noise": (13, 0, 5778, 328.3539, 282.8174, 271.7802),
    "quant": (17, 25, 2543, 13919.5392, 11875.7812, 11193.6348),
}

_meshes = {}


def mesh(reflibs, name):
    """the reference's surface of a fixture row, its adjacency and both smoothed copies, computed once and left unchanged"""
    if name not in _meshes:
        data, r0, d, iso, s = reference_mesh(reflibs, name)
        A = so.adjacency(s.T, s.nV)
        P = {pin: so.smooth(s.V, s.T, 10, 0.5, -0.53, pin, A=A)[0] for pin in (True, False)}
        for a in (P[True], P[False]):
            a.setflags(write=False)
        _meshes[name] = (data, r0, d, iso, s, A, P)
    return _meshes[name]
