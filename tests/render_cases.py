"""The views, tiny grids and made-up meshes of the rendering tests (tests/test_render_cpu.py, tests/test_gpu_render.py; DESIGN.md
24).  The matrices here are built by hand in numpy - not by MC33_view_fit, which has tests of its own - with the conventions of
include/mc33_hip.h: row major, clip = m (x, y, z, 1), x to the right, y up, depth 0 .. 1 away from the eye.  numpy only."""
import types

import numpy as np

import fixtures as fx
import render_oracle as ro


def frame(direction, up):
    """(right, up, forward) of a camera that looks along `direction`: right-handed, so the image is not mirrored"""
    f = np.asarray(direction, np.float64)
    f = f / np.sqrt((f * f).sum())
    r = np.cross(f, np.asarray(up, np.float64))
    r = r / np.sqrt((r * r).sum())
    return r, np.cross(r, f), f


def perspective(eye, target, up, fov_degrees, width, height, near, far):
    eye = np.asarray(eye, np.float64)
    r, u, f = frame(np.asarray(target, np.float64) - eye, up)
    th = np.tan(np.radians(fov_degrees) / 2.0)
    a, b = far / (far - near), -far * near / (far - near)
    rows = [r / (th * width / height), u / th, a * f, f]
    off = [0.0, 0.0, b, 0.0]
    return np.array([list(rows[k]) + [off[k] - float(rows[k] @ eye)] for k in range(4)]).reshape(16)


def orthographic(centre, direction, up, half_height, width, height, near, far):
    """near, far: signed distances from `centre` along `direction`"""
    c = np.asarray(centre, np.float64)
    r, u, f = frame(direction, up)
    rows = [r / (half_height * width / height), u / half_height, f / (far - near), np.zeros(3)]
    off = [0.0, 0.0, -near / (far - near), 1.0]
    return np.array([list(rows[k]) + [off[k] - float(rows[k] @ c)] for k in range(4)]).reshape(16)


def pixels(width, height):
    """x, y of a vertex are pixel coordinates (x to the right, y DOWN, pixel (i, j) has its centre at (i + 0.5, j + 0.5)), z is its depth"""
    return np.array([2.0 / width, 0, 0, -1.0, 0, -2.0 / height, 0, 1.0, 0, 0, 1.0, 0, 0, 0, 0, 1.0])


def ball(shape, c, R):
    """R^2 - |x - c|^2: the field falls outwards, so the stored normals point outwards"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    return R * R - (((x - c[0]) ** 2 + (y - c[1]) ** 2) + (z - c[2]) ** 2)


SPHERE_C, SPHERE_R = (11.3, 11.6, 11.4), 8.2
SPHERE_EYE = (41.0, 33.0, 29.0)
GRID_CASES = ("sphere", "noise16", "inside", "f64")


def case(name):
    """data [nz, ny, nx], dtype, iso, and the view of the case (cull 0, two-sided: the tests vary both)"""
    c = types.SimpleNamespace(name=name, dtype="f32", iso=0.0, r0=(0.0, 0.0, 0.0), d=(1.0, 1.0, 1.0))
    light = (0.3, 0.5, 0.8)
    if name in ("sphere", "f64"):
        c.dtype = "f64" if name == "f64" else "f32"
        data = ball((24, 24, 24), SPHERE_C, SPHERE_R)
        c.eye = SPHERE_EYE
        c.view = ro.view(perspective(c.eye, SPHERE_C, (0.0, 0.0, 1.0), 28.0, 96, 64, 30.0, 60.0), 96, 64, light=light, background=0xFF201008)
    elif name == "noise16":
        data = fx.noise_f32(16, 3)
        c.eye = (44.0, 31.0, 27.0)
        c.view = ro.view(perspective(c.eye, (7.5, 7.5, 7.5), (0.0, 0.0, 1.0), 30.0, 128, 128, 25.0, 75.0), 128, 128, light=light)
    elif name == "inside":  # the eye inside the grid, next to the surface: corners behind it, fragments before the near plane
        data = ball((24, 24, 24), SPHERE_C, SPHERE_R)
        c.eye = (SPHERE_C[0] + 7.6, SPHERE_C[1], SPHERE_C[2])
        c.view = ro.view(perspective(c.eye, (SPHERE_C[0] + 6.0, SPHERE_C[1] + 6.0, SPHERE_C[2] + 1.0), (0.0, 0.0, 1.0), 100.0, 64, 48, 2.5, 30.0), 64, 48, light=light)
    else:
        raise KeyError(name)
    c.data = np.ascontiguousarray(data.astype(np.float64 if c.dtype == "f64" else np.float32))
    c.data.setflags(write=False)
    return c


def colour_words(n, seed=11):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def normals(n, seed=12):
    x = np.random.default_rng(seed).standard_normal((n, 3))
    return (x / np.sqrt((x * x).sum(axis=1))[:, None]).astype(np.float32)


def mesh(V, T, seed=0, dtype=np.float32):
    V = np.ascontiguousarray(np.asarray(V, np.float64).astype(dtype))
    T = np.ascontiguousarray(np.asarray(T, np.int64).astype(np.uint32).reshape(-1, 3))
    return types.SimpleNamespace(V=V, N=normals(V.shape[0], 12 + seed), T=T, C=colour_words(V.shape[0], 11 + seed))


def lattice(seed):
    """A planar lattice of quads in pixel coordinates whose vertices lie on pixel centres and corners (steps of 0.5, 1 or 1.5 pixels
    from a start on the half-pixel lattice), every quad cut along a random diagonal, every triangle wound at random, partly outside
    the viewport.  Returns (mesh, view, inside): inside - the pixel centres in the outline by the top-left rule, x0 <= cx < x1 and
    y0 <= cy < y1, inside the viewport."""
    rng = np.random.default_rng(seed)
    width, height = int(rng.integers(5, 40)), int(rng.integers(5, 40))
    nx, ny = int(rng.integers(1, 14)), int(rng.integers(1, 14))
    sx, sy = 0.5 * rng.integers(1, 4), 0.5 * rng.integers(1, 4)
    x0, y0 = 0.5 * rng.integers(-6, 2 * width - 4), 0.5 * rng.integers(-6, 2 * height - 4)
    xs, ys = x0 + sx * np.arange(nx + 1), y0 + sy * np.arange(ny + 1)
    V = np.array([[x, y, 0.5] for y in ys for x in xs])
    T = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            for t in ([(a, b, c), (a, c, d)] if rng.integers(2) else [(a, b, d), (b, c, d)]):
                T.append(t if rng.integers(2) else (t[0], t[2], t[1]))
    cx, cy = np.arange(width) + 0.5, np.arange(height) + 0.5
    inside = int(((cx >= xs[0]) & (cx < xs[-1])).sum()) * int(((cy >= ys[0]) & (cy < ys[-1])).sum())
    return mesh(V, T, seed), ro.view(pixels(width, height), width, height), inside


def quad(width, height, z=(0.2, 0.4, 0.9, 0.6)):
    """two triangles over the whole viewport"""
    V = [[0, 0, z[0]], [width, 0, z[1]], [width, height, z[2]], [0, height, z[3]]]
    return mesh(V, [[0, 1, 2], [0, 2, 3]], 3), ro.view(pixels(width, height), width, height, light=(0.2, -0.3, 0.9))


def guard():
    """4096 x 4096: one triangle with two corners ON the guard band's limit (X, Y = +2^23) that covers the whole viewport, one with a
    corner two steps of 1/256 pixel beyond it (rejected), one with a corner on the limit -2^23 whose box holds no pixel of the viewport"""
    far, step = 32768.0, 1.0 / 128.0
    V = [[0, 0, 0.25], [far, 0, 0.5], [0, far, 0.75], [-far - step, 0, 0.5], [-far, 0, 0.5], [0, -far, 0.5]]
    return mesh(V, [[0, 2, 1], [0, 3, 2], [0, 4, 5]], 4), ro.view(pixels(4096, 4096), 4096, 4096)


def with_bad_indices(m):
    nV = m.V.shape[0]
    T = np.concatenate([m.T[:3], np.array([[0, 1, nV], [0xFFFFFFFF, 2, 3]], np.uint32), m.T[3:], np.array([[nV + 7, nV, 0]], np.uint32)])
    return types.SimpleNamespace(V=m.V, N=m.N, T=np.ascontiguousarray(T), C=m.C)


def with_nonfinite(m):
    V = m.V.copy()
    V[1, 0], V[V.shape[0] // 2, 2], V[-1, 1] = np.nan, np.inf, -np.inf
    return types.SimpleNamespace(V=V, N=m.N, T=m.T, C=m.C)


def tiny(width=32, height=24):
    """triangles smaller than 1/256 pixel around a few points - their corners round to one or two lattice points - beside
    triangles a few steps of 1/256 pixel wide that hold no pixel centre, and some that hold exactly one"""
    rng = np.random.default_rng(21)
    V, T = [], []
    for k in range(60):
        p = np.array([rng.uniform(1, width - 1), rng.uniform(1, height - 1)])
        if k % 3 == 2:
            p = np.floor(p) + 0.5  # on a pixel centre
        size = (1e-4, 1.0 / 256.0, 3.0 / 256.0)[k % 3]
        for _ in range(3):
            V.append([p[0] + rng.uniform(-size, size), p[1] + rng.uniform(-size, size), rng.uniform(0.1, 0.9)])
        T.append([3 * k, 3 * k + 1, 3 * k + 2])
    return mesh(V, T, 5), ro.view(pixels(width, height), width, height)
