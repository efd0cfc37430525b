"""What the tests of the mesh passes that need no GPU share (tests/test_*_cpu.py of measure, topology, filter, smooth, simplify,
clip, section, cap, render, distance, curvature, property, resample, spectrum):
  reference_mesh      the reference's surface of a fixture row, made once and held to the row's figures
  assert_exported     the exported names of every library
  kernel_metadata, kernels_of, assert_kernels   the kernels in a library's gfx950 code object, their registers and scratch
  MESH_KERNELS, launched   the kernels of the shared mesh layer, and the ones a part names among them
  c_layout            size of C structs and offset and size of their members, as the C compiler has them for a flavour
  c_signatures, ctypes_signature   class and size of a function's return type and parameters, as the C++ compiler deduces
                      them from the headers, and the same string from a row of a ctypes signature table
  host_logic          the host-logic build of mc33_capi.c with an object on it
tests/test_bindings_cpu.py runs c_layout and c_signatures over the whole binding.  The device-side helpers of the same parts
are in tests/mesh_harness.py, what a part's two test files share in tests/<part>_cases.py."""
import contextlib
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
import types

import pytest

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
        assert mo.open_edges(s.T) == mo.FIXTURES[name][2][4], "fixture %s drifted: %d open edges" % (name, mo.open_edges(s.T))
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


LLVM = "/opt/rocm/lib/llvm/bin"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def kernel_metadata(lib):
    """[{name, scratch, vgprs, vgpr_spills, sgpr_spills, lds}] of the gfx950 code object inside a product library."""
    objcopy, bundler, readelf, filt = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf"), shutil.which("c++filt")
    if not (objcopy and bundler and readelf):
        pytest.skip("LLVM binutils of ROCm not found")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(d, "copy.so")])
        subprocess.check_call([bundler, "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
        notes = subprocess.check_output([readelf, "--notes", co], text=True)
    kernels, cur = [], {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\S.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'")
        if k == "agpr_count" or (k == "args" and cur.get("name")):
            pass
        if k == "name" and v.startswith("_Z"):
            cur["name"] = v
        elif k in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size"):
            cur[k] = int(v)
        if k == "wavefront_size":  # last key of a kernel's record (keys are sorted)
            if "name" in cur:
                kernels.append(cur)
            cur = {}
    for kd in kernels:
        if filt:
            kd["pretty"] = subprocess.check_output([filt, kd["name"]], text=True).strip().split("(")[0].replace("void ", "")
        else:
            kd["pretty"] = kd["name"]
    return kernels


# the kernels of the layer the mesh passes share (csrc/mc33_mesh.hip.h; tests/test_mesh_common_cpu.py holds them to the code object)
# (the second argument of k_mesh_place: 0 a rank, 1 the new index or none, 2 row starts with the total behind them)
MESH_KERNELS = ["k_mesh_tile_sum<MeshFlag>", "k_mesh_tile_sum<MeshCount>", "k_mesh_tile_sum<ClipOwned>", "k_mesh_tile_sum<ClipOutputs>", "k_mesh_scan_top",
                "k_mesh_place<MeshFlag, 0>", "k_mesh_place<MeshFlag, 1>", "k_mesh_place<MeshCount, 2>", "k_mesh_clear", "k_mesh_ref"]


def launched(*names):
    """the shared kernels a part launches, by their names in MESH_KERNELS"""
    for n in names:
        assert n in MESH_KERNELS, n
    return list(names)


def kernels_of(dtype):
    """{demangled name: metadata} of the gfx950 code object in a sample type's library"""
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


def _compiled_output(compiler, suffix, head, lines, flags):
    """what a program prints whose main() holds `lines`, one statement per line, each with the label it is about: [(label,
    statement)].  It is compiled over both public headers with the flavour's flags; when the compiler refuses a line, the
    AssertionError names that line's label and quotes the compiler."""
    src = head.splitlines() + ["#include \"marching_cubes_33.h\"", "#include \"mc33_hip.h\"", "int main(void) {"]
    first = len(src) + 1
    src += [statement for _, statement in lines] + ["\treturn 0;", "}", ""]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "probe" + suffix)
        with open(path, "w") as f:
            f.write("\n".join(src))
        r = subprocess.run(compiler + list(flags) + ["-I", os.path.join(ROOT, "include"), path, "-o", os.path.join(tmp, "probe")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            hit = sorted(set(int(n) for n in re.findall(r"probe%s:(\d+):\d+: error" % re.escape(suffix), r.stderr)))
            about = sorted(set(lines[n - first][0] for n in hit if 0 <= n - first < len(lines)))
            errors = [line for line in r.stderr.splitlines() if "error" in line]
            raise AssertionError("the headers do not have what the binding names (%s): %s\n%s" % (" ".join(flags) or "default flavour", ", ".join(about), "\n".join(errors[:8])))
        return subprocess.check_output([os.path.join(tmp, "probe")], text=True)


def c_layout(structs, flags=()):
    """The layout of C structs over both public headers, as the C compiler has it for a flavour's flags.  structs: [(C type, the
    member names)]; returns {C type: (sizeof, {member: (offsetof, sizeof)})}.  A name that is no member of its struct does not
    compile: an AssertionError that names the struct."""
    lines = []
    for ctype, members in structs:
        lines.append((ctype, "\tprintf(\"%%zu\\n\", sizeof(%s));" % ctype))
        for m in members:
            lines.append((ctype, "\tprintf(\"%%zu %%zu\\n\", offsetof(%s, %s), sizeof(((%s *)0)->%s));" % (ctype, m, ctype, m)))
    out = iter(_compiled_output(["gcc"], ".c", "#include <stdio.h>\n#include <stddef.h>", lines, flags).splitlines())
    return {ctype: (int(next(out)), {m: tuple(int(x) for x in next(out).split()) for m in members}) for ctype, members in structs}


_SIGNATURE_PROBE = """#include <cstdio>
#include <type_traits>
template<class T> struct One { static void print() { std::printf(" %c%zu", std::is_pointer<T>::value ? 'p' : std::is_floating_point<T>::value ? 'f' : std::is_signed<T>::value ? 'i' : 'u', sizeof(T)); } };
template<> struct One<void> { static void print() { std::printf(" v0"); } };
template<class F> struct Sig;
template<class R, class... A> struct Sig<R (*)(A...)> { static void print(const char *name) { std::printf("%s", name); One<R>::print(); (One<A>::print(), ...); std::printf("\\n"); } };"""


def c_signatures(names, flags=()):
    """{name: "r a a ..."} of functions the public headers declare, for a flavour's flags: the class (p pointer, f float, i signed,
    u unsigned integer, v void) and size of the return type and of every parameter, deduced by the C++ compiler from
    decltype(&name).  Nothing is called or linked.  A name the headers do not declare does not compile: an AssertionError that
    names it."""
    lines = [(n, "\tSig<decltype(&%s)>::print(\"%s\");" % (n, n)) for n in names]
    out = _compiled_output(["g++", "-std=c++17"], ".cpp", _SIGNATURE_PROBE, lines, flags)
    return {line.split()[0]: " ".join(line.split()[1:]) for line in out.splitlines()}


def ctypes_signature(restype, argtypes):
    """the same string from a row of a signature table"""
    sized = {C.c_double: "f8", C.c_float: "f4", C.c_int: "i4", C.c_uint: "u4", C.c_ulonglong: "u8", C.c_size_t: "u8"}

    def code(t):
        if t is None:
            return "v0"
        if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C._CFuncPtr)):
            return "p8"
        return sized[t]  # (KeyError: a class the tables are not meant to hold)
    return " ".join(code(t) for t in [restype] + list(argtypes))


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
