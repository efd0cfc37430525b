"""What the tests of the mesh passes that need no GPU share (tests/test_*_cpu.py of measure, topology, filter, smooth, simplify,
clip, property, resample, spectrum): the reference's surface of a fixture row, made once; the exported names of every library;
the kernels in the code object; the layout of the headers' structs; the host-logic build of mc33_capi.c with an object on it.
The device-side helpers of the same parts are in tests/mesh_harness.py."""
import contextlib
import os
import subprocess
import tempfile
import types

import fixtures as fx
import measure_oracle as mo
from mc33_capi import MC33Lib, product_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_reference = {}


def reference_mesh(reflibs, name):
    """(data, r0, d, iso, the reference's surface) of a row of measure_oracle.FIXTURES: extracted once, held to the row's sizes,
    and left unchanged - V, N and T are read-only.  Every part's mesh() adds its own derived data to this, under its own cache."""
    if name not in _reference:
        field, iso, (nV, nT, _, _, _) = mo.FIXTURES[name]
        data, r0, d = field()
        s = reflibs["f32"].isosurface(data, iso, r0, d)
        assert (s.nV, s.nT) == (nV, nT), "fixture %s drifted: %d vertices, %d triangles" % (name, s.nV, s.nT)
        for a in (s.V, s.N, s.T):
            a.setflags(write=False)
        _reference[name] = (data, r0, d, iso, s)
    return _reference[name]


def assert_exported(names, dtype):
    """all four flavours of a sample type's library define the names"""
    for ortho, nneg in ((False, False), (True, False), (False, True), (True, True)):
        path = product_path(dtype, ortho=ortho, nneg=nneg)
        assert os.path.exists(path), "build the HIP libraries first (python -m mc33_c_library_amd.build)"
        syms = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        defined = set(line.split()[-1] for line in syms.splitlines() if line.split())
        for n in names:
            assert n in defined, "%s not exported by %s" % (n, os.path.basename(path))


def kernels_of(dtype):
    """{demangled name: metadata} of the gfx950 code object in a sample type's library"""
    from test_code_objects import kernel_metadata
    return {k["pretty"]: k for k in kernel_metadata(product_path(dtype))}


def assert_kernels(dtype, names, max_vgprs=64):
    """the kernels are in the code object, with no private segment, no spilled register and at most max_vgprs registers per lane
    (64: eight waves per SIMD; 128: two blocks of 256 per SIMD at least); returns kernels_of(dtype)"""
    ks = kernels_of(dtype)
    for name in names:
        assert name in ks, (name, sorted(ks))
        assert ks[name]["private_segment_fixed_size"] == 0 and ks[name]["vgpr_spill_count"] == 0, (name, ks[name])
        assert ks[name]["vgpr_count"] <= max_vgprs, (name, ks[name])
    return ks


def c_layout(expressions):
    """the values of C expressions - sizeof(...), offsetof(...) - over both public headers, as the C compiler has them"""
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"marching_cubes_33.h\"\n#include \"mc33_hip.h\"\nint main(void) {\n"
    for e in expressions:
        src += "\tprintf(\"%%zu\\n\", (size_t)(%s));\n" % e
    src += "\treturn 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "sizes.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "sizes.c"), "-o", os.path.join(tmp, "sizes")])
        return [int(x) for x in subprocess.check_output([os.path.join(tmp, "sizes")], text=True).split()]


def offsets(struct, members):
    """the same expressions for c_layout: offsetof(struct, m) of every member"""
    return ["offsetof(%s, %s)" % (struct, m) for m in members]


@contextlib.contextmanager
def host_logic(dtype, n=20, prop=None):
    """mc33_capi.c linked with the emulated device layer, which has none of the mesh passes' entry points (they are weak
    references, so the library still loads), and an MC33 object on a cosine field of n^3 samples.  Yields lib (the MC33Lib), L
    (its CDLL), M (the object), iso (an isovalue that cuts the field) and, with prop(shape, np_dtype) given, Pg: a second grid
    of those samples.  Calls nothing of the product beyond make_grid and create_MC33; frees M, the grid, then Pg on exit."""
    from mc33_emu import build_hostlogic
    lib = MC33Lib(build_hostlogic(dtype), dtype)
    L = lib.lib
    data = fx.cos_field(n)[0] if dtype == "f32" else fx.cos_field_u16(n, n, n)
    iso = 0.0 if dtype == "f32" else 30000.0
    G, keep = lib.make_grid(data)
    Pg, keep2 = lib.make_grid(prop(data.shape, lib.np_dtype)) if prop is not None else (None, None)
    M = L.create_MC33(G)
    assert M
    try:
        yield types.SimpleNamespace(lib=lib, L=L, M=M, iso=iso, Pg=Pg)
    finally:
        L.free_MC33(M)
        L.free_memory_grd(G)
        if Pg is not None:
            L.free_memory_grd(Pg)
        del keep, keep2
