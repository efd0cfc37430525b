"""GPU tests of the distance between surfaces (include/mc33_hip.h: mc33hip_surface_distance; include/marching_cubes_33.h:
MC33_isosurface_distance, MC33_simplification_error; DeviceGrid.distance / surface_distance / extract_simplified(error=True) /
extract_smoothed(error=True)).

The expected arrays come from tests/distance_oracle.py, the definition in numpy over ALL pairs: oDist, oTri, oPoint, the counts,
max, min, argmax and argmin are compared bit for bit; sum and sum_sq are held to measure_oracle.sum_bound of the oracle's terms and
to identical bits between two calls.  Every made-up case runs on three contexts - MC33_HIP_DISTANCE_CELLS unset, 1 (every point
tests every triangle) and huge (the finest lattice the library allows) - which must return the same bytes.  Every output of every
call is canaried (tests/mesh_harness.py: CanariedCall)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import distance_cases as dc
import distance_oracle as do
import fixtures as fx
import measure_oracle as mo
import mesh_pieces as mp
import simplify_oracle as sp
from mc33_c_library_amd.api import SurfaceDistance, SurfaceSimplification
from mc33_capi import MC33Lib, ref_path
from mesh_checks import reference_mesh as mesh
from mesh_harness import SPARE, CanariedCall, bits, capi, device_grid, once_per_key, tiny_grid, to_device
from simplify_cases import CELLS, simplified

pytestmark = pytest.mark.gpu

KNOBS = (None, "1", "4000000000")
SUMMARY = ("max", "min", "argmax", "argmin")


def context_with(knob, make=tiny_grid):
    """a context created with MC33_HIP_DISTANCE_CELLS = knob (it is read when a context is created)"""
    old = os.environ.pop("MC33_HIP_DISTANCE_CELLS", None)
    if knob is not None:
        os.environ["MC33_HIP_DISTANCE_CELLS"] = knob
    try:
        return make()
    finally:
        os.environ.pop("MC33_HIP_DISTANCE_CELLS", None)
        if old is not None:
            os.environ["MC33_HIP_DISTANCE_CELLS"] = old


@pytest.fixture(scope="module")
def ctxs():
    gs = [context_with(k) for k in KNOBS]
    yield gs
    for g in gs:
        g.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
    return ctxs[0]


class Call(CanariedCall):
    """one mc33hip_surface_distance call"""

    def __init__(self, g, P, V, T, signed=False, want=("dist", "tri", "point"), change=None):
        import torch
        from mc33_c_library_amd.api import Distance
        super().__init__(g)
        self.nP = P.shape[0]
        self.oDist = self.room(self.nP, 0, torch.float32) if "dist" in want else None
        self.oTri = self.room(self.nP, 0, torch.int32) if "tri" in want else None
        self.oPoint = self.room(self.nP, 3, P.dtype) if "point" in want else None
        a = Distance()
        a.P, a.nP, a.V, a.T, a.nV, a.nT = P.data_ptr(), self.nP, V.data_ptr(), T.data_ptr(), V.shape[0], T.shape[0]
        a.signed_distance = int(bool(signed))
        a.oDist, a.oTri, a.oPoint = (x.data_ptr() if x is not None else None for x in (self.oDist, self.oTri, self.oPoint))
        self.keep = (P, V, T)
        self.call(g.lib.mc33hip_surface_distance, a, change)
        self.counts = tuple(int(getattr(a, n)) for n in do.COUNTS)
        self.summary = tuple(getattr(a, n) for n in SUMMARY)
        self.sums = (a.sum, a.sum_sq)
        self.lattice, self.tests = tuple(a.lattice), int(a.triangle_tests)

    def outputs(self):
        return [(self.oDist, self.nP), (self.oTri, self.nP), (self.oPoint, self.nP)]

    def check(self, want):
        """bit for bit against the oracle, the two sums within the bound of their additions"""
        assert self.counts == want.counts(), (self.counts, want.counts())
        if self.oDist is not None:
            self.equal_bits("oDist", self.oDist[:self.nP], want.dist)
        if self.oTri is not None:
            self.equal_bits("oTri", self.oTri[:self.nP], want.tri)
        if self.oPoint is not None:
            self.equal_bits("oPoint", self.oPoint[:self.nP], want.point)
        got, exp = self.summary, (want.max, want.min, want.argmax, want.argmin)
        print("summary", got, exp, "sums", self.sums, "lattice", self.lattice, "tests", self.tests)
        assert np.array_equal(bits(np.array(got[:2])), bits(np.array(exp[:2]))) and got[2:] == exp[2:], (got, exp)
        for s, terms in zip(self.sums, (want.sum_terms, want.sum_sq_terms)):
            assert abs(s - mo.fsum(terms)) <= mo.sum_bound(terms), (s, mo.fsum(terms), mo.sum_bound(terms))
        self.spare_intact()


def run_everywhere(ctxs, P, V, T, want, signed=False):
    """the case on the three contexts: the oracle's bits on each, the same bytes and sums on all; returns the calls"""
    dP, dV, dT = to_device(P), to_device(V), to_device(T)
    calls = []
    for g in ctxs:
        call = Call(g, dP, dV, dT, signed)
        assert call.rc == 0, call.message
        call.check(want)
        calls.append(call)
    again = Call(ctxs[0], dP, dV, dT, signed)
    assert again.all_bytes() == calls[0].all_bytes() and bits(np.array(again.sums)).tolist() == bits(np.array(calls[0].sums)).tolist(), "two calls differ"
    for call in calls[1:]:
        assert call.all_bytes() == calls[0].all_bytes() and call.summary == calls[0].summary
    usable = T.shape[0] - want.invalid_triangles - want.nonfinite_triangles
    if usable:  # MC33_HIP_DISTANCE_CELLS=1: one cell, every matched point tests every usable triangle once
        assert calls[1].lattice == (1, 1, 1) and calls[1].tests == want.matched_points * usable, (calls[1].lattice, calls[1].tests)
    return calls


# ---- 1. the ladder -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nT", dc.LADDER_TRIANGLES)
def test_ladder(ctxs, nT):
    P, V, T = dc.ladder(dc.LADDER_POINTS[-1], nT)
    whole = do.distance(P, V, T)
    for nP in dc.LADDER_POINTS:
        calls = run_everywhere(ctxs, P[:nP], V, T, do.head(whole, nP))
        if nT == 5000:
            assert max(calls[2].lattice) > max(calls[0].lattice) > 1, [c.lattice for c in calls]


# ---- 2. exact ties -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["sheet", "two_equidistant", "doubled"])
def test_exact_ties(ctxs, case):
    P, V, T = getattr(dc, case)()
    want = do.distance(P, V, T)
    run_everywhere(ctxs, P, V, T, want)
    # T permuted: oTri changes exactly as the oracle says, oDist not at all
    perm = np.random.default_rng(3).permutation(T.shape[0]) if T.shape[0] > 2 else np.array([1, 0])
    T2 = np.ascontiguousarray(T[perm])
    want2 = do.distance(P, V, T2)
    assert np.array_equal(bits(want2.dist), bits(want.dist))
    if case == "two_equidistant":  # the other triangle is index 0 now, and wins
        assert np.all(want.tri == 0) and np.all(want2.tri == 0) and not np.array_equal(want2.point, want.point)
    else:
        assert not np.array_equal(want2.tri, want.tri)
    run_everywhere(ctxs, P, V, T2, want2)


# ---- 3. far and edge points, 4. crowded and spanning lists ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["far_and_edge", "far_from_the_origin", "crowded", "spanning"])
def test_far_edge_crowded_spanning(ctxs, case):
    P, V, T = getattr(dc, case)()
    want = do.distance(P, V, T, signed=True)
    calls = run_everywhere(ctxs, P, V, T, want, signed=True)
    if case == "spanning":  # found from an interior cell of a lattice that has one
        assert min(calls[0].lattice) >= 3 and np.all(want.tri[:200] == T.shape[0] - 1)


# ---- 5. hostile input ----------------------------------------------------------------------------------------------------------------

def test_hostile_triangles_and_points(ctxs):
    P, V, T, bad, wild = dc.hostile()
    want = do.distance(P, V, T)
    assert want.counts() == (P.shape[0] - wild, wild, 0, bad.size)
    calls = run_everywhere(ctxs, P, V, T, want)
    got = calls[0]
    tri = got.host(got.oTri[:got.nP]).view(np.uint32)
    assert not np.isin(tri, bad).any() and np.all(tri[-wild:] == do.NONE)
    assert np.all(got.host(got.oDist[got.nP - wild:got.nP]) == np.inf) and np.isnan(got.host(got.oPoint[got.nP - wild:got.nP])).all()
    # no usable triangle at all: the invalid one makes it ERUNTIME, the outputs are complete
    from mc33_c_library_amd.api import ERUNTIME
    P, V, T = dc.all_unusable()
    want = do.distance(P, V, T)
    for g in ctxs:
        call = Call(g, to_device(P), to_device(V), to_device(T))
        assert call.rc == ERUNTIME and "1 triangle " in call.message and call.lattice == (0, 0, 0), (call.rc, call.message)
        call.check(want)
    call = Call(ctxs[0], to_device(P), to_device(V), to_device(T[:2]))  # without it: success, everybody unmatched
    assert call.rc == 0, call.message
    call.check(do.distance(P, V, T[:2]))


def test_invalid_triangles_are_counted_not_read(reflibs, ctxs):
    """mesh_pieces.spoil(..., "invalid"): 300 triangles name row nV.  V is the first nV rows of a tensor with spare rows behind
    them, so that not even a wrong kernel could touch memory this test does not own."""
    import torch
    from mc33_c_library_amd.api import ERUNTIME
    data, r0, d, iso, s = mesh(reflibs, "blobs")
    room = torch.zeros((s.nV + SPARE, 3), dtype=torch.float32, device="cuda")
    room[:s.nV] = to_device(s.V)
    V = room[:s.nV]
    badT = mp.spoil(s.T, s.nV, 3, "invalid")
    P = (s.V[::137].astype(np.float64) + 0.37 * np.asarray(d)).astype(np.float32)
    want = do.distance(P, s.V, badT)
    assert want.invalid_triangles == mp.SPOILED_EACH
    for g in ctxs:
        bad = Call(g, to_device(P), V, to_device(badT))
        assert bad.rc == ERUNTIME and "300 triangles " in bad.message, (bad.rc, bad.message)
        bad.check(want)  # the outputs are the oracle's without those triangles
    good = Call(ctxs[0], to_device(P), V, to_device(s.T))  # the next call on the context succeeds
    assert good.rc == 0, good.message
    good.check(do.distance(P, s.V, s.T))


# ---- 6. whole fixtures without an all-pairs oracle -----------------------------------------------------------------------------------

@once_per_key
def uploaded(reflibs, name):
    data, r0, d, iso, s = mesh(reflibs, name)
    return to_device(s.V), to_device(s.T)


@pytest.mark.parametrize("name", list(mo.FIXTURES))
def test_fixture_against_itself_and_its_simplification(reflibs, ctx, name):
    data, r0, d, iso, s = mesh(reflibs, name)
    V, T = uploaded(reflibs, name)
    zero, first = do.own_vertices(s.V, s.T)
    own = Call(ctx, V, V, T)
    assert own.rc == 0, own.message
    dist, tri = own.host(own.oDist[:s.nV]), own.host(own.oTri[:s.nV]).view(np.uint32)
    assert np.count_nonzero(zero) == s.nV - mo.FIXTURES[name][2][3]  # (every referenced vertex: tests/test_distance_cpu.py)
    assert np.all(bits(dist[zero]) == 0) and np.all(tri[zero] <= first[zero])  # exactly +0.0, and no later than the first incident triangle
    assert own.counts == (s.nV, 0, 0, 0) and own.summary[1] == 0.0 and own.summary[3] == int(np.argmax(dist == 0.0))
    own.spare_intact()
    if name == "sphere":  # the search prunes at all: a working lattice is orders of magnitude below
        assert own.tests * 8 < s.nV * s.nT, (own.tests, s.nV * s.nT, own.lattice)
    # every 41st vertex of the 2x2x2-simplified surface against the full one, bit for bit with the oracle
    simp = simplified(reflibs, name, "2x2x2", "mean", True)
    P = np.ascontiguousarray(simp.V[::41])
    assert P.shape[0] * s.nT <= 2e7
    some = Call(ctx, to_device(P), V, T, signed=True)
    assert some.rc == 0, some.message
    want = do.distance(P, s.V, s.T, signed=True)
    some.check(want)
    # the full query: the summary agrees with the arrays
    full = Call(ctx, to_device(simp.V), V, T)
    assert full.rc == 0 and full.counts == (simp.nV_out, 0, 0, 0), full.message
    dist = full.host(full.oDist[:simp.nV_out])
    # (argmax is the first point that attains the largest D2 as a DOUBLE - the calls checked against the oracle hold it to that;
    # an earlier point may round to the same float)
    assert np.float32(full.summary[0]) == dist.max() and dist[full.summary[2]] == dist.max() and full.summary[2] >= int(np.argmax(dist == dist.max()))
    assert np.array_equal(bits(dist[::41]), bits(np.abs(want.dist)))
    full.spare_intact()


# ---- 7. signed -----------------------------------------------------------------------------------------------------------------------

def test_signed_distance_of_the_pushed_sphere(reflibs, ctxs):
    data, r0, d, iso, s = mesh(reflibs, "sphere")
    P, side = dc.pushed(s.V[::41], s.N[::41], d)
    want = do.distance(P, s.V, s.T, signed=True)
    assert 100 < np.count_nonzero(want.negative) < P.shape[0] - 100
    calls = run_everywhere(ctxs, P, s.V, s.T, want, signed=True)
    got = calls[0].host(calls[0].oDist[:P.shape[0]])
    assert np.array_equal(got < 0, want.negative)


# ---- 8. the other builds -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["u8", "f64"])
def test_other_sample_types(case):
    """MC33_real is double in libMC33_f64: rows of 24 bytes in P, V and oPoint"""
    real = np.float64 if case == "f64" else np.float32
    data = fx.cos_field(8, dtype=np.float64)[0] if case == "f64" else fx.cos_field_int(8, np.uint8, 40.0, 128.0)
    P, V, T = dc.ladder(257, 257, dtype=real)
    assert V.dtype == real and V.strides[0] == (24 if case == "f64" else 12)
    want = do.distance(P, V, T, signed=True)
    assert want.point.dtype == real
    gs = [context_with(k, lambda: device_grid(data)) for k in KNOBS]
    try:
        run_everywhere(gs, P, V, T, want, signed=True)
    finally:
        for g in gs:
            g.close()


# ---- 9. arguments --------------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_and_null_outputs(ctx):
    import itertools
    import torch
    from mc33_c_library_amd.api import EINVAL, Distance
    P, V, T = dc.ladder(257, 64)
    want = do.distance(P, V, T)
    dP, dV, dT = to_device(P), to_device(V), to_device(T)
    for change in (dict(P=None), dict(V=None), dict(T=None), dict(nP=1 << 32), dict(nV=1 << 32), dict(nT=1 << 32)):
        call = Call(ctx, dP, dV, dT, change=change)
        assert call.rc == EINVAL, (change, call.rc, call.message)
        call.spare_intact(written=False)  # every output still at its fill
    L = ctx.lib.mc33hip_surface_distance
    assert L(ctx.ctx, None) == EINVAL and L(None, C.byref(Distance())) == EINVAL
    # null outputs in every combination
    for n in range(4):
        for some in itertools.combinations(("dist", "tri", "point"), n):
            call = Call(ctx, dP, dV, dT, want=some)
            assert call.rc == 0, (some, call.message)
            call.check(want)
    # sizes of zero
    none = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    call = Call(ctx, none, dV, dT)
    assert call.rc == 0 and call.counts == (0, 0, 0, 0) and call.summary == (0.0, 0.0, 0, 0)
    call.spare_intact(written=False)
    call = Call(ctx, dP, dV, none.to(torch.int32))
    assert call.rc == 0, call.message
    call.check(do.distance(P, V, np.zeros((0, 3), np.uint32)))
    assert call.counts == (0, 257, 0, 0)
    # every overlapping pair of ranges: each array gets a place of its own in one buffer, then one output at a time is moved onto
    # the last byte of an input or of another output
    nP, nV, nT = 1000, 900, 300
    size = {"P": nP * 12, "V": nV * 12, "T": nT * 12, "oDist": nP * 4, "oTri": nP * 4, "oPoint": nP * 12}
    buf = torch.zeros((sum(size.values()) + 64 * len(size),), dtype=torch.uint8, device="cuda")
    at, off = {}, 0
    for n, b in size.items():
        at[n] = buf.data_ptr() + off
        off += b + 64

    def struct(moved=None, onto=None, end=True):
        a = Distance()
        p = dict(at)
        if moved:
            p[moved] = at[onto] + size[onto] - 1 if end else at[onto] - size[moved] + 1
        a.P, a.nP, a.V, a.T, a.nV, a.nT = p["P"], nP, p["V"], p["T"], nV, nT
        a.oDist, a.oTri, a.oPoint = p["oDist"], p["oTri"], p["oPoint"]
        return a
    outs, ins = ["oDist", "oTri", "oPoint"], ["P", "V", "T"]
    pairs = [(o, i) for o in outs for i in ins] + [(o, p) for o in outs for p in outs if o != p]
    assert len(pairs) == 9 + 6
    for o, other in pairs:
        for end in (True, False):
            assert L(ctx.ctx, C.byref(struct(o, other, end))) == EINVAL, (o, other, end)
    assert not buf.any().item()  # nothing was written
    a = struct()
    assert L(ctx.ctx, C.byref(a)) == 0 and a.matched_points == nP  # the same arrays side by side: zeros, one point triangle at the origin
    assert Call(ctx, dP, dV, dT).rc == 0  # the context is still good


# ---- 10. Python and the C API --------------------------------------------------------------------------------------------------------

def info_matches(info, want):
    assert tuple(info[n] for n in do.COUNTS) == want.counts()
    assert (info["max"], info["min"], info["argmax"], info["argmin"]) == (want.max, want.min, want.argmax, want.argmin)
    for s, terms in ((info["sum"], want.sum_terms), (info["sum_sq"], want.sum_sq_terms)):
        assert abs(s - mo.fsum(terms)) <= mo.sum_bound(terms)
    n = want.matched_points
    assert info["mean"] == info["sum"] / n and info["rms"] == math.sqrt(info["sum_sq"] / n)


SMALL = 24  # a cosine field of 24^3 samples: 2016 vertices, 3800 triangles - both directions fit the all-pairs oracle in a second or two


def small_surface(reflibs):
    data, r0, d = fx.cos_field(SMALL)
    s = reflibs["f32"].isosurface(data, 0.0, r0, d)
    assert s.nV * s.nT <= 2e7
    return data, r0, d, s


def test_python_methods(reflibs):
    data, r0, d, s = small_surface(reflibs)
    iso = 0.0
    g = device_grid(data, r0, d)
    V, T = to_device(s.V), to_device(s.T)
    simp = sp.simplify(s.V, s.T, tuple(2.0 * x for x in d), r0, sp.MEAN, True)
    P = np.ascontiguousarray(simp.V[::3])
    want = do.distance(P, s.V, s.T, signed=True)
    dist, tri, point, info = g.distance(to_device(P), V, T, signed=True, nearest_point=True)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(want.dist)) and np.array_equal(tri.cpu().numpy().view(np.uint32), want.tri)
    assert np.array_equal(bits(point.cpu().numpy()), bits(want.point))
    info_matches(info, want)
    assert g.distance(to_device(P), V, T)[2] is None
    # both directions
    fwd, bwd = do.distance(simp.V, s.V, s.T), do.distance(s.V, simp.V, simp.T)
    sd = g.surface_distance(to_device(simp.V), to_device(simp.T), V, T)
    info_matches(sd["forward"], fwd)
    info_matches(sd["backward"], bwd)
    assert sd["hausdorff"] == max(fwd.max, bwd.max) > 0.0
    # the product's own extraction: its V, T are the reference's bit for bit, so the error is the same
    V3, N3, T3, info3 = g.extract_simplified(iso, CELLS["2x2x2"], error=True)
    assert np.array_equal(bits(V3.cpu().numpy()), bits(simp.V)) and "error" not in g.extract_simplified(iso, CELLS["2x2x2"])[3]
    assert info3["error"] == sd
    # smoothed: the vertices move, T stays
    assert len(g.extract_smoothed(iso, iterations=3)) == 4
    V4, N4, T4, cnt, info4 = g.extract_smoothed(iso, iterations=3, error=True)
    moved = V4.cpu().numpy()
    assert not np.array_equal(bits(moved), bits(s.V)) and np.array_equal(T4.cpu().numpy().view(np.uint32), s.T)
    mf, mb = do.distance(moved, s.V, s.T), do.distance(s.V, moved, s.T)
    info_matches(info4["error"]["forward"], mf)
    info_matches(info4["error"]["backward"], mb)
    assert info4["error"]["hausdorff"] == max(mf.max, mb.max) > 0.0
    g.close()


def c_matches(out, want):
    """mean and rms within the bound of the sums, the rest exact"""
    assert (out.points, out.unmatched, out.argmax) == (want.matched_points, want.unmatched_points, want.argmax)
    assert np.array_equal(bits(np.array([out.max, out.min])), bits(np.array([want.max, want.min])))
    n = want.matched_points
    assert abs(out.mean - mo.fsum(want.sum_terms) / n) <= mo.sum_bound(want.sum_terms) / n + 1e-15 * out.mean
    ms = mo.fsum(want.sum_sq_terms) / n
    assert abs(out.rms ** 2 - ms) <= mo.sum_bound(want.sum_sq_terms) / n + 1e-14 * ms


def state(M):
    m = M.contents
    return (m.iso, m.nV, m.nT, m.memoryfault, m.T, m.V)


@pytest.mark.parametrize("nneg", [False, True], ids=["plain", "nneg"])
def test_c_api(reflibs, nneg, monkeypatch):
    """the oracle applied to the reference's surfaces - the _nneg reference's for the _nneg flavour: the distances do not depend
    on the winding, the triangle order is the same"""
    monkeypatch.delenv("MC33_HIP_DEVICES", raising=False)
    data, r0, d = fx.cos_field(SMALL)
    iso = 0.0
    ref = MC33Lib(ref_path("f32", nneg=True), "f32") if nneg else reflibs["f32"]
    s0, s1 = ref.isosurface(data, iso, r0, d), ref.isosurface(data, iso + 0.25, r0, d)
    assert 0 < s0.nV * s1.nT <= 2e7
    lib = capi(nneg=nneg)
    L = lib.lib
    G, keep = lib.make_grid(data, r0, d)
    M = L.create_MC33(G)
    assert M
    try:
        out = (SurfaceDistance * 2)()
        assert L.MC33_isosurface_distance(M, lib.real(iso), lib.real(iso + 0.25), out) == 0
        c_matches(out[0], do.distance(s0.V, s1.V, s1.T))
        assert out[0].min > 0.0 and M.contents.memoryfault == 0
        c = tuple(2.0 * x for x in d)
        simp = sp.simplify(s0.V, s0.T, c, r0, sp.MEAN, True)
        sm = SurfaceSimplification((C.c_double * 3)(2, 2, 2), sp.MEAN, 1)
        assert L.MC33_simplification_error(M, lib.real(iso), C.byref(sm), out) == 0
        c_matches(out[0], do.distance(simp.V, s0.V, s0.T))
        c_matches(out[1], do.distance(s0.V, simp.V, simp.T))
        # an empty surface: -2 and zeros
        assert L.MC33_isosurface_distance(M, lib.real(iso), lib.real(1e9), out) == -2 and (out[0].points, out[0].max) == (0, 0.0)
        assert L.MC33_isosurface_distance(M, lib.real(1e9), lib.real(iso), out) == -2
        sm_all = SurfaceSimplification((C.c_double * 3)(1000, 1000, 1000), sp.MEAN, 1)
        assert L.MC33_simplification_error(M, lib.real(iso), C.byref(sm_all), out) == -2 and (out[1].points, out[1].rms) == (0, 0.0)
        # refused calls leave M as it was
        S = L.calculate_isosurface(M, lib.real(iso))
        assert S
        before = state(M)
        nan = float("nan")
        assert L.MC33_isosurface_distance(M, lib.real(iso + 1), lib.real(iso), None) == -1
        assert L.MC33_simplification_error(M, lib.real(iso + 1), None, out) == -1 and L.MC33_simplification_error(M, lib.real(iso + 1), C.byref(sm), None) == -1
        for bad in (SurfaceSimplification((C.c_double * 3)(0, 2, 2), 0, 1), SurfaceSimplification((C.c_double * 3)(nan, 2, 2), 0, 1), SurfaceSimplification((C.c_double * 3)(2, 2, 2), 2, 1)):
            assert L.MC33_simplification_error(M, lib.real(iso + 1), C.byref(bad), out) == -1
        assert state(M) == before
        L.free_surface_memory(S)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_accepts_an_inclined_grid(monkeypatch):
    """V is in world space and the distance is a property of V and T alone: the shell of an inclined grid is measured; the
    simplification error is refused there, as the simplification is"""
    monkeypatch.delenv("MC33_HIP_DEVICES", raising=False)
    data = fx.cos_field(20)[0]
    lib = capi()
    L = lib.lib
    A = [[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    Ai = np.linalg.inv(np.array(A)).tolist()
    G, keep = lib.make_grid(data, inclined=(A, Ai))
    M = L.create_MC33(G)
    assert M
    try:
        out = (SurfaceDistance * 2)()
        assert L.MC33_isosurface_distance(M, lib.real(0.0), lib.real(0.2), out) == 0
        S = L.calculate_isosurface(M, lib.real(0.0))
        a = lib.copy_surface(S)
        L.free_surface_memory(S)
        S = L.calculate_isosurface(M, lib.real(0.2))
        b = lib.copy_surface(S)
        L.free_surface_memory(S)
        c_matches(out[0], do.distance(a.V, b.V, b.T))
        before = state(M)
        sm = SurfaceSimplification((C.c_double * 3)(2, 2, 2), 0, 1)
        assert L.MC33_simplification_error(M, lib.real(0.1), C.byref(sm), out) == -1 and state(M) == before
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep


def test_c_api_refuses_several_slabs(monkeypatch):
    """MC33_HIP_DEVICES is read by create_MC33: an object on two slabs refuses both calls, is left alone, and still extracts"""
    lib = capi()
    L = lib.lib
    data = fx.cos_field(24)[0]
    monkeypatch.setenv("MC33_HIP_DEVICES", "0,0")
    G, keep = lib.make_grid(data)
    M = L.create_MC33(G)
    assert M
    try:
        before = state(M)
        out = (SurfaceDistance * 2)()
        sm = SurfaceSimplification((C.c_double * 3)(2, 2, 2), 0, 1)
        assert L.MC33_isosurface_distance(M, lib.real(0.0), lib.real(0.2), out) == -1
        assert L.MC33_simplification_error(M, lib.real(0.0), C.byref(sm), out) == -1
        assert state(M) == before
        S = L.calculate_isosurface(M, lib.real(0.0))
        assert S and S.contents.nV > 0
        L.free_surface_memory(S)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        del keep
