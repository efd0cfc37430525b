"""GPU tests of the stages that work on a finished mesh - mc33hip_label_components, mc33hip_measure_surface,
mc33hip_measure_components, mc33hip_surface_topology, mc33hip_component_topology (include/mc33_hip.h) - on meshes made up in numpy
(tests/mesh_pieces.py, smooth_oracle.random_mesh): many components whose runs of equal keys have every length around a wave, a
block and a tile, in any order of vertices and triangles, vertex counts at the edges of the tiles and of the top-level scan,
triangle lists that are not manifold, and one context that takes all of it in turn.

The expected values come from tests/measure_oracle.py and tests/topology_oracle.py and, where the mesh is unspoiled, from the
closed forms of tests/mesh_pieces.py as well (tests/test_mesh_pieces_cpu.py holds the two against each other).  Integers and
labels are compared exactly; a double sum S = sum x_i over n terms within (n + 8) * 2^-53 * fsum(|x_i|), the bound of
tests/test_gpu_measure.py, which holds for every order of additions made in double.  No mesh comes from the reference."""
import ctypes as C
import re

import numpy as np
import pytest

import filter_oracle as fo
import fixtures as fx
import measure_oracle as mo
import mesh_pieces as mp
import smooth_oracle as so
import measure_cases as tm
import topology_cases as tt
import topology_oracle as to
from mesh_harness import bits, check_python, device_grid, info_of, to_device

pytestmark = pytest.mark.gpu

SEED = 7
MESH_TILE = 1024  # vertices per block of k_cc_count / k_mesh_place; k_mesh_scan_top takes 256 tiles per round
_mesh, _want, _fresh = {}, {}, {}


@pytest.fixture(autouse=True)
def small_caches():
    """the ladder and the small components are shared between tests; every other mesh and its oracle go when its test is through"""
    yield
    for cache in (_mesh, _want):
        for key in [k for k in cache if isinstance(k, tuple) and k[0] not in ("ladder", "small")]:
            del cache[key]
    _fresh.clear()
    _want.pop("smooth", None)


def field(dtype="f32"):
    return fx.cos_field(16, dtype=np.float64 if dtype == "f64" else np.float32)


def new_grid(dtype="f32"):
    """a context for meshes that come from no grid"""
    return device_grid(*field(dtype))


def mesh(key):
    """(V, T, expected or None) of a key: (set, vertex order, triangle order[, defects]), ("random", nV), ("one",), ("empty",);
    made once and left unchanged"""
    if key not in _mesh:
        if key[0] == "random":
            V, T = so.random_mesh(key[1], 1)
            _mesh[key] = (V, T, None)
        elif key[0] == "one":
            V, T, _, exp = mp.pieces([1], SEED, "identity", "runs")
            _mesh[key] = (V, T, exp)
        elif key[0] == "empty":
            V, T, _, exp = mp.pieces([], SEED, "identity", "runs", unreferenced=300)
            _mesh[key] = (V, T, exp)
        elif len(key) == 4:
            V, T, _ = mesh(key[:3])
            _mesh[key] = (V, mp.spoil(T, V.shape[0], 11, key[3]), None)
        else:
            V, T, _, exp = mp.pieces(seed=SEED, vertex_order=key[1], triangle_order=key[2], **mp.SETS[key[0]])
            _mesh[key] = (V, T, exp)
        for a in _mesh[key][:2]:
            a.setflags(write=False)
    return _mesh[key]


class Want:
    """the oracles' results for a mesh: labels, counts, measures, both tables and the surface's topology; `invalid` triangles
    are left out of all of them"""

    def __init__(self, V, T):
        data, r0, d = field()
        nV = V.shape[0]
        self.invalid = int(np.count_nonzero(~(T.astype(np.int64) < nV).all(axis=1)))
        self.lab, self.ncomp, self.unref, _ = mo.label_components(T, nV)
        self.meas = mo.measure(V, T, r0, d, data.shape)
        self.mtab, self.ab, self.wb = mo.component_table(V, T, self.lab, self.meas.origin)
        self.surf, self.ttab = to.surface(T, nV, self.lab)


def want(key):
    if key not in _want:
        V, T, _ = mesh(key)
        _want[key] = Want(V, T)
    return _want[key]


def device_mesh(g, V, T):
    import torch
    dV = to_device(V.astype(np.float64 if g.dtype == "f64" else np.float32))  # (copies: the shared arrays are read-only)
    dT = to_device(T.copy()) if T.shape[0] else torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    return dV, dT


def host(labels):
    return labels.cpu().numpy().view(np.uint32)


def columns(table, names=None):
    """the named columns' bytes (a row's padding bytes say nothing)"""
    return b"".join(np.ascontiguousarray(table[n]).tobytes() for n in names or table.dtype.names)


def refused(call, n):
    """ERUNTIME with the number of triangles in the message"""
    from mc33_c_library_amd.api import ERUNTIME, MC33Error
    with pytest.raises(MC33Error) as e:
        call()
    assert e.value.code == ERUNTIME and re.search(r"\b%d triangles? " % n, str(e.value)), str(e.value)


def full_check(g, label, key):
    """Every stage on the mesh of `key`, on the context g: labels bit-equal, the measures within their bounds with bounding box
    and origin exact, both component tables with the labels given and made inside, the surface's topology - against the oracle,
    and against the closed forms where the mesh is unspoiled - and a second call with the same integer results.  Where triangles
    name a vertex outside V every call is refused with their number, and what it wrote is the oracle's without them.  Returns
    the integer results, name -> bytes or tuple."""
    V, T, exp = mesh(key)
    w = want(key)
    nV, nT = V.shape[0], T.shape[0]
    dV, dT = device_mesh(g, V, T)
    if w.invalid:
        return check_refused(g, label, dV, dT, nV, nT, w)
    labels, nc, nu = g.label_components(dT, nV)
    assert np.array_equal(host(labels), w.lab), "%s: %d of %d labels differ" % (label, np.count_nonzero(host(labels) != w.lab), nV)
    assert (nc, nu) == (w.ncomp, w.unref), (label, nc, nu, w.ncomp, w.unref)
    got = g.measure(dV, dT)
    tm.check_measures(label, got, w.meas)
    mtab = g.measure_components(dV, dT, labels)
    tm.check_table(label, mtab, w.mtab, w.ab, w.wb, w.meas)
    inside = g.measure_components(dV, dT)
    tm.check_table(label + " (labels made inside)", inside, w.mtab, w.ab, w.wb, w.meas)
    surf = g.topology(dT, nV)
    tt.check_surface(label, surf, w.surf)
    ttab = g.component_topology(dT, nV, labels)
    tt.check_table(label + " (labels given)", ttab, w.ttab)
    tt.check_table(label + " (labels made inside)", g.component_topology(dT, nV), w.ttab)
    if exp is not None:  # the closed forms
        assert np.array_equal(host(labels), exp["labels"]) and (nc, nu) == (exp["components"], exp["unreferenced"])
        tt.check_surface(label + " (closed form)", surf, exp["surface"])
        tt.check_table(label + " (closed form)", ttab, exp["table"])
        for col in ("root", "nV", "nT"):
            assert np.array_equal(mtab[col], exp["table"][col]), (label, col)
    ints = {"labels": host(labels).tobytes(), "counts": (nc, nu), "surface": surf.as_tuple(), "topology rows": columns(ttab),
            "measured rows": columns(mtab, ("root", "nV", "nT"))}
    # a second call
    labels2, nc2, nu2 = g.label_components(dT, nV)
    mtab2 = g.measure_components(dV, dT, labels2)
    again = {"labels": host(labels2).tobytes(), "counts": (nc2, nu2), "surface": g.topology(dT, nV).as_tuple(),
             "topology rows": columns(g.component_topology(dT, nV, labels2)), "measured rows": columns(mtab2, ("root", "nV", "nT"))}
    for k in ints:
        assert again[k] == ints[k], "%s: two calls differ in %s" % (label, k)
    assert tm.all_bits(g.measure(dV, dT)) == tm.all_bits(got), "%s: two calls of measure differ" % label
    return ints


def check_refused(g, label, dV, dT, nV, nT, w):
    """Every call is refused with the number of invalid triangles.  What a refused call wrote is compared where it writes:
    mc33hip_measure_surface, mc33hip_label_components and mc33hip_surface_topology fill their outputs without those triangles.
    mc33hip_measure_components and mc33hip_component_topology return when the flag pass has counted them, before any row is
    made: of them only the code and the count are checked."""
    import torch
    from mc33_c_library_amd.api import ERUNTIME, Measures, SurfaceMeasures, SurfaceTopology, Topology
    given = to_device(w.lab)
    refused(lambda: g.measure(dV, dT), w.invalid)
    refused(lambda: g.label_components(dT, nV), w.invalid)
    refused(lambda: g.measure_components(dV, dT, given), w.invalid)
    refused(lambda: g.measure_components(dV, dT), w.invalid)
    refused(lambda: g.topology(dT, nV), w.invalid)
    refused(lambda: g.component_topology(dT, nV, given), w.invalid)
    refused(lambda: g.component_topology(dT, nV), w.invalid)
    # what the refused calls wrote leaves those triangles out
    L, ctx, pV, pT = g.lib, g.ctx, C.c_void_p(dV.data_ptr()), C.c_void_p(dT.data_ptr())
    m = Measures()
    assert L.mc33hip_measure_surface(ctx, pV, nV, pT, nT, None, C.byref(m)) == ERUNTIME
    tm.check_measures(label + " (refused)", SurfaceMeasures(m), w.meas)
    labels = torch.full((nV,), -1, dtype=torch.int32, device="cuda")
    nc, nu = C.c_ulonglong(), C.c_ulonglong()
    assert L.mc33hip_label_components(ctx, pT, nT, nV, C.c_void_p(labels.data_ptr()), C.byref(nc), C.byref(nu)) == ERUNTIME
    assert np.array_equal(host(labels), w.lab) and (nc.value, nu.value) == (w.ncomp, w.unref)
    t = Topology()
    assert L.mc33hip_surface_topology(ctx, pT, nT, nV, C.byref(t)) == ERUNTIME
    surf = SurfaceTopology(t)
    tt.check_surface(label + " (refused)", surf, w.surf)
    return {"labels": host(labels).tobytes(), "counts": (nc.value, nu.value), "surface": surf.as_tuple()}


def run(key, dtype="f32", then=None):
    """the full check on a context of its own; then: a second mesh on the same context"""
    g = new_grid(dtype)
    try:
        full_check(g, "-".join(str(k) for k in key), key)
        if then is not None:
            full_check(g, "-".join(str(k) for k in then) + " (next call)", then)
    finally:
        g.close()


# ---- a: runs of equal keys of every length around a wave, a block and a tile ---------------------------------------------------------

@pytest.mark.parametrize("triangle_order", mp.TRIANGLE_ORDERS)
@pytest.mark.parametrize("vertex_order", mp.VERTEX_ORDERS)
def test_run_ladder_f32(vertex_order, triangle_order):
    key = ("ladder", vertex_order, triangle_order)
    V, T, exp = mesh(key)
    assert (V.shape[0], T.shape[0], exp["components"]) == (35623, 35376, 120)
    run(key)


@pytest.mark.parametrize("vertex_order,triangle_order", [("permuted", "robin"), ("identity", "runs")])
def test_run_ladder_f64(vertex_order, triangle_order):
    run(("ladder", vertex_order, triangle_order), "f64")


# ---- b: many small components; pieces of more than one step --------------------------------------------------------------------------

@pytest.mark.parametrize("triangle_order", mp.TRIANGLE_ORDERS)
def test_many_small_components(triangle_order):
    key = ("small", "permuted", triangle_order)
    V, T, exp = mesh(key)
    assert V.shape[0] == 346673 and (exp["components"], exp["surface"]["closed_components"]) == (65000, 21667)
    run(key)


def test_single_triangles_in_no_order():
    run(("single", "permuted", "shuffle"))


def test_more_triangles_than_one_step_of_every_wave():
    """Up to 8 blocks per CU x 256 lanes - 524 288 triangles, vertices or slots on 256 CUs - a block's piece of the table kernels
    is one step of its four waves, and nothing is held from a step into the next.  563 200 triangles on 580 800 vertices, in an
    order in which no key follows itself: every lane that begins a run holds a row of another component when its second step
    comes."""
    key = ("long", "permuted", "robin")
    V, T, exp = mesh(key)
    assert min(V.shape[0], T.shape[0]) > 2 * 8 * 256 * 128  # (two steps where the device has 256 CUs; fewer CUs: more steps)
    run(key)


# ---- c: vertex counts at the edges of a tile and of the top-level scan -----------------------------------------------------------------

@pytest.mark.parametrize("unreferenced", [0, 1])
@pytest.mark.parametrize("nV", mp.TILE_EDGE_SIZES + mp.TILE_EDGE_MORE)
def test_tile_and_scan_edges(nV, unreferenced):
    """identity x runs, the last component a single triangle: its root is the last flagged vertex, nV - 3 - unreferenced.  It lies
    in the last tile wherever that tile has room for the triangle's three vertices (a root that owns a triangle has two larger
    vertices behind it) - at nV = 1024 k + 1 and + 2 it lies in the tile before, and the last tile holds the triangle's other
    vertices or the unreferenced one; 1027 and 262147 put the root first in a last tile of three.  From 262147 referenced
    vertices on the root's tile is one of k_cc_scan_top's second round: at 262147 the round's only tile, at 263169 = 257 tiles
    + 1 the first of two - tile 256 holds the root, tile 257 one vertex that is no root."""
    key = ("edge-%d-%d" % (nV, unreferenced), "identity", "runs")
    V, T, exp = mesh(key)
    assert V.shape[0] == nV
    root = int(exp["table"]["root"][-1])
    assert root == nV - 3 - unreferenced and T[-1].tolist() == [root, root + 1, root + 2] and int(exp["table"]["nT"][-1]) == 1
    last = (nV - 1) // MESH_TILE
    assert root // MESH_TILE == (last if (nV - 1) % MESH_TILE >= 2 + unreferenced else last - 1)
    if nV in (1027, 262147) and not unreferenced:
        assert root == last * MESH_TILE
    if nV - unreferenced >= 262147:
        assert root // MESH_TILE >= 256
    run(key)


# ---- d: meshes that are not manifold ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", mp.DEFECTS + (mp.DEFECTS,), ids=mp.DEFECTS + ("all",))
@pytest.mark.parametrize("vertex_order,triangle_order", [("permuted", "shuffle"), ("identity", "runs")])
def test_spoiled_meshes(vertex_order, triangle_order, what):
    clean = ("ladder", vertex_order, triangle_order)
    key = clean + (what,)
    w = want(key)
    named = (what,) if isinstance(what, str) else what
    assert w.invalid == (mp.SPOILED_EACH if "invalid" in named else 0)
    assert "duplicate" not in named or w.surf["nonmanifold_edges"] > 0
    assert "flip" not in named or w.surf["misoriented_edges"] > 0
    assert "degenerate" not in named or w.surf["degenerate_triangles"] == mp.SPOILED_EACH
    run(key, then=clean if w.invalid else None)  # (after a refused call the next one on the context succeeds)


@pytest.mark.parametrize("nV", [4097, 262145])
def test_random_triangle_soup(nV):
    key = ("random", nV)
    w = want(key)
    assert min(w.surf["nonmanifold_edges"], w.surf["misoriented_edges"], w.surf["degenerate_triangles"], w.surf["boundary_loops"]) > 0
    if nV == 262145:
        assert (w.surf["edges"], w.surf["nonmanifold_edges"], w.surf["misoriented_edges"], w.surf["boundary_loops"]) == (832037, 127332, 74996, 315)
    run(key)


# ---- e: one context, any order ---------------------------------------------------------------------------------------------------------

def fresh(key):
    """the integer results of the full check on a context that has seen nothing else"""
    if key not in _fresh:
        g = new_grid()
        try:
            _fresh[key] = full_check(g, "-".join(str(k) for k in key) + " (fresh context)", key)
        finally:
            g.close()
    return _fresh[key]


def compact_every_third(g):
    V, T, exp = mesh(("ladder", "permuted", "shuffle"))
    w = want(("ladder", "permuted", "shuffle"))
    N = np.random.default_rng(3).standard_normal(V.shape).astype(np.float32)
    roots = w.mtab["root"][::3]
    expected = fo.compact(V, N, T, w.lab, roots)
    assert expected.components_kept == 40 and expected.left_out == 0
    dV, dT = device_mesh(g, V, T)
    labels = g.label_components(dT, V.shape[0])[0]
    check_python(g.compact_components(dV, to_device(N), dT, labels, roots), expected)


def smooth_soup(g):
    V, T, _ = mesh(("random", 4097))
    if "smooth" not in _want:
        P, A = so.smooth(V, T, 2, 0.5, -0.53, True)
        _want["smooth"] = (P, so.vertex_normals(P, T), A)
    P, N, A = _want["smooth"]
    dV, dT = device_mesh(g, V, T)
    V2, N2, info = g.smooth(dV, dT, iterations=2, pin_boundary=True)
    assert np.array_equal(bits(V2.cpu().numpy()), bits(P)) and np.array_equal(bits(N2.cpu().numpy()), bits(N))
    assert tuple(info[k] for k in ("max_degree", "isolated_vertices", "boundary_vertices", "invalid_triangles")) == info_of(A)


def extract_own_grid(g):
    def surface(grid):
        V, N, T, cnt = grid.extract(0.5)
        return (cnt.nV, cnt.nT, cnt.active_cells), [x.cpu().numpy().tobytes() for x in (V, N, T)]
    if "extract" not in _fresh:
        g0 = new_grid()
        try:
            _fresh["extract"] = surface(g0)
        finally:
            g0.close()
    got = surface(g)
    assert got[0] == _fresh["extract"][0] and got[0][1] > 0, (got[0], _fresh["extract"][0])
    assert got[1] == _fresh["extract"][1]


def test_one_context_any_order():
    """Scratch that outlives a call - flags, tile sums, ranks, the boundary flags, the loop forest, the rows and the slot table grow
    on demand and are cleared for the current mesh only.  One context takes a large mesh, smaller ones, none at all, the large one
    again, a refused call, with a compaction, a smoothing and an extraction of its own grid in between; every result is the
    oracle's and, integer for integer, that of a context that has seen nothing else."""
    small, ladder = ("small", "permuted", "robin"), ("ladder", "permuted", "shuffle")
    sequence = [small, ladder, ("one",), ("empty",), small, ("edge-262145-0", "identity", "runs"), ladder + (mp.DEFECTS,), ladder]
    between = [compact_every_third, smooth_soup, extract_own_grid]
    assert mesh(("one",))[0].shape[0] == 3 and mesh(("empty",))[1].shape[0] == 0 and want(ladder + (mp.DEFECTS,)).invalid == mp.SPOILED_EACH
    g = new_grid()
    try:
        for step, key in enumerate(sequence):
            label = "step %d: %s" % (step + 1, "-".join(str(k) for k in key))
            got = full_check(g, label, key)
            alone = fresh(key)
            for k in alone:
                assert got[k] == alone[k], "%s: %s differs from a fresh context's" % (label, k)
            between[step % 3](g)
    finally:
        g.close()
