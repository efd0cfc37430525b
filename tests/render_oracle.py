"""The rendering of include/mc33_hip.h (mc33hip_render_surface) restated in numpy: float64 and int64 (Python
integers where one triangle is set up), vectorised over a triangle's box of pixel centres, a Python loop over the triangles, the
resolve vectorised over the covered pixels.  Every expression keeps the order of operations of the definition; numpy fuses
nothing.  The device is held to this bit for bit (tests/test_gpu_render.py); tests/test_render_cpu.py holds this to facts it does
not compute itself.  numpy only."""
import math
import types

import numpy as np

COUNTS = ("drawn", "culled", "degenerate", "rejected", "offscreen", "invalid_triangles", "fragments", "covered")
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NOTRI = 0xFFFFFFFF
GUARD = float(1 << 23)
BAND = 1 << 20  # pixels of a box handled at once


def view(m, width, height, cull=0, two_sided=1, light=(0.0, 0.0, 1.0), ambient=0.2, diffuse=0.8, background=0xFF000000):
    return types.SimpleNamespace(m=np.asarray(m, np.float64).reshape(16).copy(), width=int(width), height=int(height), cull=int(cull), two_sided=int(two_sided),
                                 light=tuple(float(x) for x in light), ambient=float(ambient), diffuse=float(diffuse), background=int(background))


def screen(V, vw):
    """X, Y (int64, 1/256 pixel), z, cw (float64) and usable per vertex"""
    m = vw.m.reshape(4, 4)
    P = np.asarray(V).astype(np.float64).reshape(-1, 3)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        c = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(4)]
        usable = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2]) & np.isfinite(c[3]) & (c[3] > 0.0)
        cw = np.where(usable, c[3], 1.0)
        ix, iy, zz = c[0] / cw, c[1] / cw, c[2] / cw
        sx, sy = (ix * 0.5 + 0.5) * float(vw.width), (0.5 - iy * 0.5) * float(vw.height)
        fx, fy = np.floor(sx * 256.0 + 0.5), np.floor(sy * 256.0 + 0.5)
        usable = usable & (np.abs(fx) <= GUARD) & (np.abs(fy) <= GUARD)
    X = np.where(usable, fx, 0.0).astype(np.int64)
    Y = np.where(usable, fy, 0.0).astype(np.int64)
    return X, Y, zz, cw, usable


def setup(X, Y, t, vw):
    """the class of one triangle with three valid, usable corners, and what its pixels need: (class, s, box)"""
    x = [int(X[v]) for v in t]
    y = [int(Y[v]) for v in t]
    area2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    if area2 == 0:
        return "degenerate", None
    front = area2 < 0
    if (vw.cull == 1 and not front) or (vw.cull == 2 and front):
        return "culled", None
    x0, x1 = max((min(x) - 128 + 255) >> 8, 0), min((max(x) - 128) >> 8, vw.width - 1)
    y0, y1 = max((min(y) - 128 + 255) >> 8, 0), min((max(y) - 128) >> 8, vw.height - 1)
    if x0 > x1 or y0 > y1:
        return "offscreen", None
    return "drawn", (x, y, area2, x0, x1, y0, y1)


def edges(x, y, area2, Px, Py):
    """E of the three edges at the points (Px, Py) (int64 arrays that broadcast), negated with dx, dy when area2 < 0, and inside"""
    s = -1 if area2 < 0 else 1
    E, inside = [], True
    for e in range(3):
        n = (e + 1) % 3
        dx, dy = s * (x[n] - x[e]), s * (y[n] - y[e])
        Ee = dx * (Py - y[e]) - dy * (Px - x[e])
        E.append(Ee)
        inside = inside & ((Ee > 0) | ((Ee == 0) & bool(dy < 0 or (dy == 0 and dx > 0))))
    return E, inside


def render(V, N, T, C, vw, base_color=0xFFFFFFFF, want_key=False, shade=True):
    """shade False: no colour image (rgba is None) - the depth and id images and the counts do not depend on it"""
    V, T = np.asarray(V), np.asarray(T).astype(np.int64).reshape(-1, 3)
    nV, nT = V.shape[0], T.shape[0]
    W, H = vw.width, vw.height
    X, Y, z, cw, usable = screen(V, vw)
    key = np.full((H, W), NOKEY, np.uint64)
    n = dict.fromkeys(COUNTS, 0)
    for i in range(nT):
        t = T[i]
        if (t >= nV).any() or (t < 0).any():
            n["invalid_triangles"] += 1
            continue
        if not usable[t].all():
            n["rejected"] += 1
            continue
        cls, tri = setup(X, Y, t, vw)
        n[cls] += 1
        if cls != "drawn":
            continue
        x, y, area2, x0, x1, y0, y1 = tri
        Px = (np.arange(x0, x1 + 1, dtype=np.int64) * 256 + 128)[None, :]
        rows = max(1, BAND // (x1 - x0 + 1))
        z0, z1, z2 = (float(z[v]) for v in t)
        for ya in range(y0, y1 + 1, rows):
            yb = min(ya + rows, y1 + 1)
            Py = (np.arange(ya, yb, dtype=np.int64) * 256 + 128)[:, None]
            E, inside = edges(x, y, area2, Px, Py)
            w0, w1, w2 = E[1], E[2], E[0]
            with np.errstate(all="ignore"):
                zf = ((w0.astype(np.float64) * z0 + w1.astype(np.float64) * z1) + w2.astype(np.float64) * z2) / float(abs(area2))
                frag = inside & (zf >= 0.0) & (zf <= 1.0)
                zq = np.floor(np.where(frag, zf, 0.0) * 4294967295.0 + 0.5).astype(np.uint64)
            k = np.where(frag, (zq << np.uint64(32)) | np.uint64(i), NOKEY)
            sub = key[ya:yb, x0:x1 + 1]
            np.minimum(sub, k, out=sub)
            n["fragments"] += int(frag.sum())
    out = resolve(V, N, T, C, vw, base_color, key, (X, Y, z, cw), shade)
    n["covered"] = int((key != NOKEY).sum())
    for k, v in n.items():
        setattr(out, k, v)
    out.counts = lambda: tuple(n[k] for k in COUNTS)
    if want_key:
        out.key = key
    return out


def unit_light(light):
    lx, ly, lz = light
    length = math.sqrt((lx * lx + ly * ly) + lz * lz)
    return lx / length, ly / length, lz / length


def resolve(V, N, T, C, vw, base_color, key, scr, shade=True):
    W, H = vw.width, vw.height
    rgba = np.full(H * W, vw.background & 0xFFFFFFFF, np.uint32)
    depth = np.full(H * W, np.inf, np.float32)
    tri = np.full(H * W, NOTRI, np.uint32)
    flat = key.reshape(-1)
    covered = np.nonzero(flat != NOKEY)[0]
    for a in range(0, covered.size, BAND):
        resolve_pixels(covered[a:a + BAND], flat, N, T, C, vw, base_color, scr, shade, rgba, depth, tri)
    return types.SimpleNamespace(rgba=rgba.reshape(H, W) if shade else None, depth=depth.reshape(H, W), tri=tri.reshape(H, W))


def resolve_pixels(idx, flat, N, T, C, vw, base_color, scr, shade, rgba, depth, tri):
    X, Y, z, cw = scr
    W = vw.width
    ti = (flat[idx] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    t = T[ti]
    Px, Py = (idx % W) * 256 + 128, (idx // W) * 256 + 128
    Xc, Yc = X[t], Y[t]
    area2 = (Xc[:, 1] - Xc[:, 0]) * (Yc[:, 2] - Yc[:, 0]) - (Xc[:, 2] - Xc[:, 0]) * (Yc[:, 1] - Yc[:, 0])
    s = np.where(area2 < 0, -1, 1).astype(np.int64)
    E = []
    for e in range(3):
        k = (e + 1) % 3
        E.append((s * (Xc[:, k] - Xc[:, e])) * (Py - Yc[:, e]) - (s * (Yc[:, k] - Yc[:, e])) * (Px - Xc[:, e]))
    w = [E[1].astype(np.float64), E[2].astype(np.float64), E[0].astype(np.float64)]
    area = np.abs(area2).astype(np.float64)
    zc = z[t]
    with np.errstate(all="ignore"):
        zf = ((w[0] * zc[:, 0] + w[1] * zc[:, 1]) + w[2] * zc[:, 2]) / area
    depth[idx] = zf.astype(np.float32)
    tri[idx] = ti.astype(np.uint32)
    if not shade:
        return
    cwc = cw[t]
    Nd = np.asarray(N).astype(np.float64).reshape(-1, 3)[t]  # [n, corner, component]
    words = (np.asarray(C).astype(np.uint32)[t] if C is not None else np.full(t.shape, base_color & 0xFFFFFFFF, np.uint32))
    lx, ly, lz = unit_light(vw.light)
    with np.errstate(all="ignore"):
        q = [(w[k] / area) / cwc[:, k] for k in range(3)]
        ssum = (q[0] + q[1]) + q[2]
        L = [q[k] / ssum for k in range(3)]
        nx, ny, nz = (((L[0] * Nd[:, 0, a] + L[1] * Nd[:, 1, a]) + L[2] * Nd[:, 2, a]) for a in range(3))
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = np.isfinite(length) & (length != 0.0)
        td = ((nx * lx + ny * ly) + nz * lz) / np.where(ok, length, 1.0)
        td = np.abs(td) if vw.two_sided else np.where(td > 0.0, td, 0.0)
        td = np.where(ok, td, 0.0)
        shade = vw.ambient + vw.diffuse * td
        word = np.full(idx.size, 0xFF000000, np.uint32)
        for shift in (0, 8, 16):
            c = [((words[:, k] >> np.uint32(shift)) & np.uint32(255)).astype(np.float64) for k in range(3)]
            x = shade * ((L[0] * c[0] + L[1] * c[1]) + L[2] * c[2])
            x = np.where(x > 0.0, x, 0.0)
            x = np.where(x < 255.0, x, 255.0)
            word |= np.floor(x + 0.5).astype(np.uint32) << np.uint32(shift)
    rgba[idx] = word
