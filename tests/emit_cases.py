"""The grids of tests/test_gpu_emit_shapes.py: every sample type, every vertex store, staged and unstaged rows, tested and slow
records, iso = -0.0, z-slabs with a ghost slice - all small (a few hundred thousand samples at most), because the launch shapes
of that test are what makes the loops of the emit passes long, not the grids.  Pure numpy; the test module turns a case into
device tensors, contexts and references.

A case extracts at `iso` (twice), then at `iso2` - which moves the record count by more than a factor of two, so the hints the
next call sizes its grids by are stale - and at `iso` again (stale the other way)."""
import collections
import functools

import numpy as np

import fixtures as fx

NP = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32}
ROUGH = (9, 66, 258)  # two row segments (256 cells), two y tiles (63 rows), nx & 3 == 1

# name, sample type, () -> dense array, isovalue, second isovalue, origin, spacing, inclined (None, "general", "cell": the
# triangular form), normal_neg, environment beyond the launch shape, layout of tests/layouts.py (None: a dense tensor),
# cut into z-slabs, own_reference (below: rough-quant-negzero)
Case = collections.namedtuple("Case", "name dtype make iso iso2 r0 d inclined normal_neg env layout slabs own_reference")


@functools.lru_cache(maxsize=None)
def _cos():
    return fx.cos_field(48)[0]


# the integer scalings of test_gpu_layouts._grids: (offset, amplitude)
SCALE = {"u8": (128.0, 40.0), "u16": (32768.0, 10000.0), "u32": (2147483648.0, 5e8)}


@functools.lru_cache(maxsize=None)
def smooth(dtype):
    c = _cos()
    if dtype == "f32":
        return c
    if dtype == "f64":
        return c.astype(np.float64)
    off, amp = SCALE[dtype]
    return np.rint(off + amp * c.astype(np.float64)).astype(NP[dtype])


def mapped(dtype, v):
    """the isovalue of the integer grid that v of the float field maps to"""
    off, amp = SCALE[dtype]
    return off + amp * v


@functools.lru_cache(maxsize=None)
def rough(kind):
    if kind == "noise":
        return fx.noise_f32(0, 11, shape=ROUGH)
    if kind == "quant32":
        return fx.noise_quant(32, 2)
    if kind == "quant":
        return fx.noise_quant(0, 5, shape=ROUGH)
    return fx.noise_u8(0, 2, 7, shape=ROUGH)


def matrices(kind):
    return fx.general_matrices() if kind == "general" else fx.cell_matrices(80.0, 95.0, 70.0)


def _case(name, dtype, make, iso, iso2, r0=(0.0, 0.0, 0.0), d=(1.0, 1.0, 1.0), inclined=None, normal_neg=False, env=(), layout=None, slabs=False, own_reference=False):
    return Case(name, dtype, make, float(iso), float(iso2), tuple(r0), tuple(d), inclined, normal_neg, tuple(env), layout, slabs, own_reference)


def _cases():
    out = []
    sm = lambda t: functools.partial(smooth, t)
    # smooth: cos_field(48) at 0.1 in every type; 2.5 leaves a small blob around the maximum (a tenth of the records)
    out.append(_case("smooth-f32", "f32", sm("f32"), 0.1, 2.5))
    out.append(_case("smooth-f64", "f64", sm("f64"), 0.1, 2.5))
    for t in ("u8", "u16", "u32"):
        at = mapped(t, 0.1)  # (an integer: 132, 33768, 2197483648)
        assert at == np.floor(at)
        out.append(_case("smooth-%s-half" % t, t, sm(t), at + 0.5, mapped(t, 2.5) + 0.5))  # no sample can equal x.5
        out.append(_case("smooth-%s-int" % t, t, sm(t), at, mapped(t, 2.5)))              # many slow records
    # the four vertex stores, float (r0 = 0, d = 1 is smooth-f32), and the inclined store in double
    out.append(_case("store1-isotropic", "f32", sm("f32"), 0.1, 2.5, (1.0, 2.0, 3.0), (0.5, 0.5, 0.5)))
    out.append(_case("store2-anisotropic", "f32", sm("f32"), 0.1, 2.5, (1.0, 2.0, 3.0), (0.5, 0.25, 1.0)))
    out.append(_case("store3-general", "f32", sm("f32"), 0.1, 2.5, (-4.0, -4.0, -4.0), (0.2, 0.3, 0.45), "general"))
    out.append(_case("store3-triangular", "f32", sm("f32"), 0.1, 2.5, (-4.0, -4.0, -4.0), (0.25, 0.25, 0.25), "cell"))
    out.append(_case("store3-general-f64", "f64", sm("f64"), 0.1, 2.5, (-4.0, -4.0, -4.0), (0.2, 0.3, 0.45), "general"))
    out.append(_case("nneg-anisotropic", "f32", sm("f32"), 0.1, 2.5, (1.0, 2.0, 3.0), (0.5, 0.25, 1.0), normal_neg=True))
    out.append(_case("nneg-general", "f32", sm("f32"), 0.1, 2.5, (-4.0, -4.0, -4.0), (0.2, 0.3, 0.45), "general", normal_neg=True))
    # rough: tested records, rows that are not staged; slow records inside the batches; iso = -0.0.  The second isovalue of the
    # quantised grids lies above every sample: no record at all
    out.append(_case("rough-noise", "f32", functools.partial(rough, "noise"), 0.05, 0.95))
    out.append(_case("rough-quant32", "f32", functools.partial(rough, "quant32"), 1.0, 2.5))
    out.append(_case("rough-quant", "f32", functools.partial(rough, "quant"), 0.0, 2.5))
    out.append(_case("rough-u8", "u8", functools.partial(rough, "u8"), 3.0, 6.5))
    # iso = -0.0: iso - F is "zero and negative" where F is 0 (Params::negzero_iso).  No sample of an unsigned grid lies above it:
    # the u8 grid has no cut cell and no record there, and the surface is empty - which the passes must get right from the hints of
    # a full one (the second isovalue).  The records that take the -0.0 branch of the slow kernels are the float grid's - where the
    # reference is not a function of its input (its triangle count depends on what earlier calls left in its id caches: DESIGN.md 8,
    # test_gpu_parity.test_negative_zero_isovalue_is_deterministic), so that one case, at that one isovalue, is held to what is: the
    # reference's number of vertices, and the arrays the library gives under its default launch shape (own_reference)
    out.append(_case("rough-u8-negzero", "u8", functools.partial(rough, "u8"), -0.0, 3.0))
    out.append(_case("rough-quant-negzero", "f32", functools.partial(rough, "quant"), -0.0, 2.5, own_reference=True))
    # unstaged: by the switch, and by a pitch that no staged row can have, poison in the padding
    for t in ("f32", "u16"):
        iso, iso2 = (0.1, 2.5) if t == "f32" else (mapped(t, 0.1) + 0.5, mapped(t, 2.5) + 0.5)
        out.append(_case("nostage-%s" % t, t, sm(t), iso, iso2, env=(("MC33_HIP_NO_STAGE", "1"),)))
        out.append(_case("padx_odd-%s" % t, t, sm(t), iso, iso2, layout="padx_odd"))
    # z-slabs, a ghost slice below each but the first
    out.append(_case("slabs-smooth", "f32", sm("f32"), 0.1, 2.5, slabs=True))
    out.append(_case("slabs-quant", "f32", functools.partial(rough, "quant"), 0.0, 2.5, slabs=True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def slab_bounds(nz_total):
    """[0, 7, 8, nz]: a slab of one slice in the middle; on a grid of 8 slices the last bound repeats and goes"""
    return sorted(set([0, 7, 8, nz_total]))


def tags(case):
    """under which headings the walk lengths of a case are booked: its sample type; the inclined store"""
    return (case.dtype,) + (("inclined",) if case.inclined else ())


# The launch shapes: name -> switches.  "slow2" gets MC33_HIP_SLOW_BLOCKS from the slow records the default shape reported.
SHAPES = collections.OrderedDict([
    ("default", {}),
    ("v8", {"MC33_HIP_EMIT_V_BLOCKS": "8"}), ("v16", {"MC33_HIP_EMIT_V_BLOCKS": "16"}),
    ("v32", {"MC33_HIP_EMIT_V_BLOCKS": "32"}), ("v64", {"MC33_HIP_EMIT_V_BLOCKS": "64"}),
    ("t8", {"MC33_HIP_EMIT_BLOCKS": "8"}), ("t16", {"MC33_HIP_EMIT_BLOCKS": "16"}), ("t12", {"MC33_HIP_EMIT_BLOCKS": "12"}),
    ("slow1-thread", {"MC33_HIP_SLOW_BLOCKS": "1", "MC33_HIP_SLOW_SLOTS": "0"}),
    ("slow1-slots", {"MC33_HIP_SLOW_BLOCKS": "1", "MC33_HIP_SLOW_SLOTS": "1"}),
    ("slow2", {"MC33_HIP_SLOW_SLOTS": "1"}),
    ("narrow-vfirst", {"MC33_HIP_CELLS_BLOCKS": "1", "MC33_HIP_EMIT_V_BLOCKS": "8", "MC33_HIP_EMIT_BLOCKS": "8", "MC33_HIP_SLOW_BLOCKS": "1", "MC33_HIP_TRI_FIRST": "0"}),
    ("narrow-tfirst", {"MC33_HIP_CELLS_BLOCKS": "1", "MC33_HIP_EMIT_V_BLOCKS": "8", "MC33_HIP_EMIT_BLOCKS": "8", "MC33_HIP_SLOW_BLOCKS": "1", "MC33_HIP_TRI_FIRST": "1"}),
])
# every switch a shape may set: cleared before a shape is put in force, whatever the environment of the run holds
SWITCHES = sorted(set(k for s in SHAPES.values() for k in s) | {"MC33_HIP_SLOW_BLOCKS", "MC33_HIP_NO_STAGE", "MC33_HIP_EMIT_V_BLOCKS_PER_CU"})
