"""The definition of property sampling (include/mc33_hip.h: mc33hip_sample_property / mc33hip_color_vertices) restated in
numpy float64, one operation per line.  It is the yardstick of tests/test_property_cpu.py and tests/test_gpu_property.py and
never calls the product.

For a vertex v, with N[a] cells along axis a, origin r0, spacing d (doubles) and the property array P[z][y][x]:
  1. g[a] = ((double)v[a] - r0[a]) / d[a]
  2. i[a] = floor(g[a]) clamped to [0, N[a]]; f[a] = g[a] - i[a] clamped to [0, 1]; f[a] = 0 where i[a] == N[a]
  3. lerp(p, q, f) = p where f == 0 (q is not read there), else p * (1 - f) + q * f
  4. samples as doubles; lerp along x on the four rows, then along y, then along z
  5. the value is that double rounded to float
  6. s = ((double)value - lo) / (hi - lo) clamped to [0, 1]; color = palette[(int)floor(s * (n - 1) + 0.5)]; a NaN value
     gets the default colour.
numpy evaluates every binary operation by itself in IEEE double: nothing here is fused into a*b+c.
"""
import numpy as np

DEFAULT_COLOR = np.uint32(0xff5c5c5c).view(np.int32)  # DefaultColorMC


def grid_coordinates(V, r0, d, shape):
    """Steps 1 and 2: (i, f) per axis, i as int64 [n, 3] (x, y, z), f as float64 [n, 3]; and g itself."""
    v = np.asarray(V).astype(np.float64)
    n_cells = (shape[2] - 1, shape[1] - 1, shape[0] - 1)
    g = np.empty_like(v)
    i = np.empty(v.shape, np.int64)
    f = np.empty_like(v)
    with np.errstate(invalid="ignore"):
        for a in range(3):
            ga = v[:, a] - np.float64(r0[a])
            ga = ga / np.float64(d[a])
            fl = np.floor(ga)
            top = np.float64(n_cells[a])
            ic = np.where(~(fl >= 0.0), 0.0, np.where(fl > top, top, fl))
            fa = ga - ic
            fa = np.where(fa < 0.0, 0.0, np.where(fa > 1.0, 1.0, fa))
            ia = ic.astype(np.int64)
            fa = np.where(ia == n_cells[a], 0.0, fa)
            g[:, a], i[:, a], f[:, a] = ga, ia, fa
    return g, i, f


def _lerp(p, q, f):
    with np.errstate(invalid="ignore", over="ignore"):
        one_minus = 1.0 - f
        left = p * one_minus
        right = q * f
        both = left + right
    return np.where(f == 0.0, p, both)


def planes_needed(V, r0, d, shape):
    """(lowest, highest) z plane any vertex reads: i_z, and i_z + 1 where f_z != 0."""
    _, i, f = grid_coordinates(V, r0, d, shape)
    return int(i[:, 2].min()), int((i[:, 2] + (f[:, 2] != 0.0)).max())


def sample_property(V, r0, d, P):
    """Steps 1 - 5: float32 [n]."""
    P = np.asarray(P)
    _, i, f = grid_coordinates(V, r0, d, P.shape)
    x0, y0, z0 = i[:, 0], i[:, 1], i[:, 2]
    # where f == 0 the second operand is not read: its index is the first operand's (there may be no sample at i + 1)
    x1 = x0 + (f[:, 0] != 0.0)
    y1 = y0 + (f[:, 1] != 0.0)
    z1 = z0 + (f[:, 2] != 0.0)

    def s(z, y, x):
        return P[z, y, x].astype(np.float64)

    r00 = _lerp(s(z0, y0, x0), s(z0, y0, x1), f[:, 0])
    r01 = _lerp(s(z0, y1, x0), s(z0, y1, x1), f[:, 0])
    r10 = _lerp(s(z1, y0, x0), s(z1, y0, x1), f[:, 0])
    r11 = _lerp(s(z1, y1, x0), s(z1, y1, x1), f[:, 0])
    p0 = _lerp(r00, r01, f[:, 1])
    p1 = _lerp(r10, r11, f[:, 1])
    with np.errstate(over="ignore", invalid="ignore"):
        return _lerp(p0, p1, f[:, 2]).astype(np.float32)


def color_values(p, palette, lo, hi, default=DEFAULT_COLOR):
    """Step 6 from the float values of step 5: int32 [n]."""
    pal = np.array([int(x) & 0xFFFFFFFF for x in palette], np.uint32).view(np.int32)
    n = len(pal)
    assert 2 <= n <= 256 and lo < hi
    p = np.asarray(p, np.float32)
    nan = np.isnan(p)
    pd = np.where(nan, 0.0, p.astype(np.float64))
    s = pd - np.float64(lo)
    s = s / (np.float64(hi) - np.float64(lo))
    s = np.where(s < 0.0, 0.0, np.where(s > 1.0, 1.0, s))
    k = s * np.float64(n - 1)
    k = k + 0.5
    k = np.floor(k).astype(np.int64)
    return np.where(nan, np.int32(default), pal[k]).astype(np.int32)


def color_vertices(V, r0, d, P, palette, lo, hi, default=DEFAULT_COLOR):
    return color_values(sample_property(V, r0, d, P), palette, lo, hi, default)
