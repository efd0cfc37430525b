"""The definition of the curvature pass (include/mc33_hip.h: mc33hip_curvature_vertices) restated in numpy float64, one operation
per line.  It is the yardstick of tests/test_curvature_cpu.py and tests/test_gpu_curvature.py and never calls the product.

Grid: N[a] cells, points 0 .. N[a], spacing d[a], origin r0[a]; S(i, j, k) the sample F[k][j][i] as a double; N[a] >= 2.
Per node, for node index n along axis a (the other two indices the node's own):
  p = min(n + 1, N[a]); m = max(n - 1, 0); c = clamp(n, 1, N[a] - 1)
  g_a  = (S(p) - S(m)) / ((double)(p - m) * d[a])
  H_aa = ((S(c + 1) - S(c)) - (S(c) - S(c - 1))) / (d[a] * d[a])
  H_ab = ((S(pa, pb) - S(pa, mb)) - (S(ma, pb) - S(ma, mb))) / (((double)(pa - ma) * d[a]) * ((double)(pb - mb) * d[b])),  a < b
Per vertex:
  1. g, i, f: steps 1 - 2 of tests/property_oracle.py
  2. the nine node quantities interpolated with that oracle's lerp along x, then y, then z; where f == 0 the second node is
     not read (its index is the first node's)
  3. g2 = (gx*gx + gy*gy) + gz*gz; gl = sqrt(g2); tr = (hxx + hyy) + hzz
  4. gHg = (((gx*gx)*hxx + (gy*gy)*hyy) + (gz*gz)*hzz) + 2.0 * ((((gx*gy)*hxy) + ((gx*gz)*hxz)) + ((gy*gz)*hyz))
  5. mean = sign * ((gHg - g2*tr) / ((2.0*g2) * gl))
  6. the adjugate of H;  7. gAg = step 4 on it; gauss = gAg / (g2*g2)
  8. disc = mean*mean - gauss; r = sqrt(disc < 0 ? 0 : disc); k1 = mean + r; k2 = mean - r
  9. the four doubles rounded to float.
numpy evaluates every binary operation by itself in IEEE double: nothing here is fused into a*b+c."""
import collections

import numpy as np

import property_oracle as po

NAMES = ("mean", "gauss", "k1", "k2")
Summary = collections.namedtuple("Summary", "lo hi finite undefined")


def _node(F, ix, iy, iz, d):
    """the nine quantities at the nodes (ix, iy, iz) (int64 arrays): a list of float64 arrays"""
    F = np.asarray(F)
    n_cells = (F.shape[2] - 1, F.shape[1] - 1, F.shape[0] - 1)
    assert min(n_cells) >= 2
    idx = (ix, iy, iz)

    def S(x, y, z):
        return F[z, y, x].astype(np.float64)

    def at(axis, value):
        j = list(idx)
        j[axis] = value
        return S(*j)

    def at2(a, va, b, vb):
        j = list(idx)
        j[a] = va
        j[b] = vb
        return S(*j)

    p = [np.minimum(idx[a] + 1, n_cells[a]) for a in range(3)]
    m = [np.maximum(idx[a] - 1, 0) for a in range(3)]
    c = [np.clip(idx[a], 1, n_cells[a] - 1) for a in range(3)]
    span = []
    for a in range(3):
        w = (p[a] - m[a]).astype(np.float64)
        w = w * np.float64(d[a])
        span.append(w)
    q = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(3):
            t = at(a, p[a]) - at(a, m[a])
            q.append(t / span[a])
        for a in range(3):
            up = at(a, c[a] + 1) - at(a, c[a])
            dn = at(a, c[a]) - at(a, c[a] - 1)
            t = up - dn
            dd = np.float64(d[a]) * np.float64(d[a])
            q.append(t / dd)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            hi = at2(a, p[a], b, p[b]) - at2(a, p[a], b, m[b])
            lo = at2(a, m[a], b, p[b]) - at2(a, m[a], b, m[b])
            t = hi - lo
            den = span[a] * span[b]
            q.append(t / den)
    return q


def _form(g, hxx, hyy, hzz, hxy, hxz, hyz):
    gx, gy, gz = g
    a = (gx * gx) * hxx
    b = (gy * gy) * hyy
    c = (gz * gz) * hzz
    diag = (a + b) + c
    e = (gx * gy) * hxy
    f = (gx * gz) * hxz
    h = (gy * gz) * hyz
    off = (e + f) + h
    return diag + 2.0 * off


def interpolated(V, r0, d, F):
    """steps 1 - 2: the nine interpolated quantities as float64 arrays"""
    F = np.asarray(F)
    _, i, f = po.grid_coordinates(V, r0, d, F.shape)
    x0, y0, z0 = i[:, 0], i[:, 1], i[:, 2]
    x1 = x0 + (f[:, 0] != 0.0)
    y1 = y0 + (f[:, 1] != 0.0)
    z1 = z0 + (f[:, 2] != 0.0)
    n = {}
    for kz, z in ((0, z0), (1, z1)):
        for ky, y in ((0, y0), (1, y1)):
            for kx, x in ((0, x0), (1, x1)):
                n[kz, ky, kx] = _node(F, x, y, z, d)
    out = []
    for k in range(9):
        r00 = po._lerp(n[0, 0, 0][k], n[0, 0, 1][k], f[:, 0])
        r01 = po._lerp(n[0, 1, 0][k], n[0, 1, 1][k], f[:, 0])
        r10 = po._lerp(n[1, 0, 0][k], n[1, 0, 1][k], f[:, 0])
        r11 = po._lerp(n[1, 1, 0][k], n[1, 1, 1][k], f[:, 0])
        p0 = po._lerp(r00, r01, f[:, 1])
        p1 = po._lerp(r10, r11, f[:, 1])
        out.append(po._lerp(p0, p1, f[:, 2]))
    return out


def curvature64(V, r0, d, F, sign=1):
    """steps 1 - 8: (mean, gauss, k1, k2) as float64 arrays"""
    assert sign in (1, -1)
    gx, gy, gz, hxx, hyy, hzz, hxy, hxz, hyz = interpolated(V, r0, d, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g2 = (gx * gx + gy * gy) + gz * gz
        gl = np.sqrt(g2)
        tr = (hxx + hyy) + hzz
        gHg = _form((gx, gy, gz), hxx, hyy, hzz, hxy, hxz, hyz)
        num = gHg - g2 * tr
        den = (2.0 * g2) * gl
        mean = np.float64(sign) * (num / den)
        axx = hyy * hzz - hyz * hyz
        ayy = hxx * hzz - hxz * hxz
        azz = hxx * hyy - hxy * hxy
        axy = hxz * hyz - hxy * hzz
        axz = hxy * hyz - hxz * hyy
        ayz = hxy * hxz - hxx * hyz
        gAg = _form((gx, gy, gz), axx, ayy, azz, axy, axz, ayz)
        gauss = gAg / (g2 * g2)
        disc = mean * mean - gauss
        r = np.sqrt(np.where(disc < 0.0, 0.0, disc))
        k1 = mean + r
        k2 = mean - r
    return mean, gauss, k1, k2


def curvature(V, r0, d, F, sign=1):
    """steps 1 - 9: (mean, gauss, k1, k2) as float32 arrays"""
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple(x.astype(np.float32) for x in curvature64(V, r0, d, F, sign))


def summary(values):
    """lo, hi: extremes of the finite floats of each output as doubles (+inf / -inf for none); finite: the vertices whose four
    floats are all finite; undefined: the others"""
    lo, hi = [], []
    all_finite = np.ones(values[0].shape, bool)
    for v in values:
        fin = np.isfinite(v)
        lo.append(float(v[fin].min()) if fin.any() else float("inf"))
        hi.append(float(v[fin].max()) if fin.any() else float("-inf"))
        all_finite &= fin
    n = int(np.count_nonzero(all_finite))
    return Summary(tuple(lo), tuple(hi), n, int(all_finite.size) - n)


def total(V, T, r0, d, shape, P):
    """(sum, bound): the sum over the triangles of area_i * ((P0 + P1) + P2) / 3 that mc33hip_measure_surface makes of P passed as
    dP, from tests/measure_oracle.py - total_mean / total_gauss of MC33_isosurface_curvature"""
    import measure_oracle as mo
    m = mo.measure(V, T, r0, d, shape, P=P)
    return m.property_integral, m.property_bound
