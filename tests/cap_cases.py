"""The tiny grids of the cap tests (tests/test_cap_cpu.py, tests/test_gpu_cap.py).  Every builder checks on the CPU
that no sample on a face of its box equals the isovalue - the cells a cap skips - except where the case is about exactly that.
numpy only."""
import types

import numpy as np

NAMES = ("dome", "corner", "saddle", "noise", "one", "flat", "full", "none", "spaced", "sub", "quant", "hole")
VARIANTS = ("dome_f64", "dome_u8", "dome_u16")  # dome in the other sample types
OPEN = ("quant", "hole")  # the cases whose result keeps boundary edges
ALL = NAMES + VARIANTS
LARGE = ("big",)  # for the device: more face cells and box points than a tile of the scans, more triangles than a block

NP = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16}

# 3 x 3 x 3, written by hand around the isovalue 0: the eight corner cells are all ambiguous somewhere, and the faces hold diagonal
# cells that the reference's face test joins (a hexagon) and ones it separates (two triangles)
SADDLE = [[[3.5, -2.5, 1.5], [-1.5, 2.5, -3.5], [2.5, -0.5, 4.5]],
          [[-4.5, 1.5, -2.5], [3.5, -1.5, 0.5], [-0.5, 3.5, -1.5]],
          [[1.5, -3.5, 2.5], [-2.5, 0.5, -4.5], [4.5, -1.5, 3.5]]]


def ball(shape, c, R):
    """R^2 - |x - c|^2 at the grid points, float64: above the isovalue 0 inside the ball"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return R * R - (((x - c[0]) ** 2 + (y - c[1]) ** 2) + (z - c[2]) ** 2)


def dome_field():
    return ball((9, 11, 13), (6.3, 5.2, 4.4), 7.1)


def case(name):
    """data [nz, ny, nx], dtype, iso, r0, d, zr: the z range of the extraction (cell slices) or None, lo / hi: the box"""
    c = types.SimpleNamespace(name=name, dtype="f32", iso=0.0, r0=(0.0, 0.0, 0.0), d=(1.0, 1.0, 1.0), zr=None)
    if name in ("dome", "spaced", "sub", "hole"):
        data = dome_field()
        if name == "spaced":
            c.r0, c.d = (-3.5, 2.0, 10.0), (0.5, 1.0, 2.0)
        if name == "sub":
            c.zr = (2, 6)
        if name == "hole":  # a sample next to the surface, away from every face (the mesh: without_nonfinite)
            data[2, 2, 2] = np.nan
    elif name == "dome_f64":
        c.dtype, data = "f64", dome_field()
    elif name in ("dome_u8", "dome_u16"):  # the same ball in integers around 100.5
        c.dtype, c.iso = name[5:], 100.5
        data = np.clip(np.rint(100.0 + 3.0 * dome_field()), 0, 255 if name == "dome_u8" else 65535)
    elif name == "big":
        data = ball((35, 37, 40), (19.3, 18.2, 17.4), 22.1)
    elif name == "corner":
        data = ball((6, 7, 8), (-0.3, -0.4, -0.2), 4.3)
    elif name == "saddle":
        data = np.array(SADDLE, np.float64)
    elif name == "noise":
        data = np.random.default_rng(33).standard_normal((12, 12, 12)) + np.pi / 100.0
    elif name == "one":
        data = np.array([[[1.5, -1.0], [-2.0, 0.5]], [[-1.5, -0.5], [2.5, -3.0]]])
    elif name == "flat":
        data = ball((7, 9, 2), (0.4, 4.3, 3.2), 3.9)
    elif name == "full":
        data = np.ones((3, 4, 5))
    elif name == "none":
        data = -np.ones((3, 4, 5))
    elif name == "quant":  # integers 0 .. 11 against the isovalue 2: a twelfth of the face samples equals it (the seed: one whose
        c.dtype, c.iso = "u8", 2.0  # surface the extractor leaves edge-manifold, so that what the caps add can be told)
        data = np.random.default_rng(35).integers(0, 12, (6, 7, 8))
    else:
        raise KeyError(name)
    c.data = np.ascontiguousarray(data.astype(NP[c.dtype]))
    nz, ny, nx = c.data.shape
    c.lo, c.hi = (0, 0, c.zr[0] if c.zr else 0), (nx - 1, ny - 1, c.zr[1] if c.zr else nz - 1)
    real = np.float64 if c.dtype == "f64" else np.float32
    box = c.data[c.lo[2]:c.hi[2] + 1]
    faces = np.concatenate([box[0].ravel(), box[-1].ravel(), box[:, 0].ravel(), box[:, -1].ravel(), box[:, :, 0].ravel(), box[:, :, -1].ravel()]).astype(real)
    c.on_faces = int(np.count_nonzero(real(c.iso) - faces == 0))
    assert (c.on_faces > 0) == (name == "quant"), (name, c.on_faces)
    assert not np.isnan(faces).any()
    c.data.setflags(write=False)
    return c


def extraction(c):
    """what an extractor without a z range is given so that it makes the surface of c's box: the planes of the box and their origin"""
    if c.zr is None:
        return c.data, c.r0
    return np.ascontiguousarray(c.data[c.zr[0]:c.zr[1] + 1]), (c.r0[0], c.r0[1], c.r0[2] + c.zr[0] * c.d[2])


def without_nonfinite(V, T):
    """T without the triangles that name a vertex with a coordinate that is not finite.  The extractor puts NaN vertices on the
    grid edges of a NaN sample and leaves no hole of its own; a caller who drops those triangles has one, and its rim lies on no
    face of the box: the `hole` case."""
    bad = ~np.isfinite(np.asarray(V, np.float64)).all(axis=1)
    T = np.asarray(T)
    return np.ascontiguousarray(T[~bad[T.astype(np.int64)].any(axis=1)])
