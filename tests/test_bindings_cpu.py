"""The whole ctypes binding against the two public headers, without a GPU and without a library: every struct mirror
(mc33_c_library_amd/api.py: STRUCTS; tests/mc33_capi.py: MIRRORS) - size, and offset and size of EVERY field, as the C compiler
has them - and every declared signature (api.py: SIGNATURES; mc33_capi.signatures) - class and size of the return type and of
every parameter, as the C++ compiler deduces them from decltype(&function).  One C and one C++ program per flavour of
marching_cubes_33.h.  And: no module under tests/ imports a test module."""
import ast
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import mc33_capi
import measure_oracle as mo
import topology_oracle as to
from mc33_c_library_amd import api
from mesh_checks import c_layout, c_signatures, ctypes_signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# flavour -> (flags, MC33_real is double, GRD_ORTHOGONAL)
FLAVOURS = {}
for _name, _flags, _double in (("f32", [], False), ("f64", ["-DGRD_TYPE_SIZE=8"], True), ("u16", ["-DINTEGER_GRD", "-DGRD_TYPE_SIZE=2"], False)):
    FLAVOURS[_name] = (_flags, _double, False)
    FLAVOURS[_name + "_ortho"] = (_flags + ["-DGRD_ORTHOGONAL"], _double, True)

# functions of mc33_hip.h that the package does not call: none today
NOT_CALLED = set()


def mirror(ctype, flavour):
    """the test-side class for a C type in a flavour (None: no mirror of that layout)"""
    _, double, ortho = FLAVOURS[flavour]
    row = mc33_capi.MIRRORS[ctype]
    return row.get((double, ortho)) if isinstance(row, dict) else row


def mirrors(flavour):
    """[(C type, class)]: every row of STRUCTS and every test-side mirror that has this flavour's layout"""
    rows = list(api.STRUCTS.items()) + [(ctype, mirror(ctype, flavour)) for ctype in mc33_capi.MIRRORS]
    return [(ctype, cls) for ctype, cls in rows if cls is not None]


def members(cls):
    return [api.FIELD_ALIASES.get((cls, f[0]), f[0]) for f in cls._fields_]


_layouts, _signatures = {}, {}


def layouts(flavour):
    if flavour not in _layouts:
        _layouts[flavour] = c_layout([(ctype, members(cls)) for ctype, cls in mirrors(flavour)], FLAVOURS[flavour][0])
    return _layouts[flavour]


def tables(flavour):
    """{name: (restype, argtypes)} of both signature tables in a flavour; a name in both must have the same C signature"""
    _, double, ortho = FLAVOURS[flavour]
    rows = {name: (r, a) for name, (r, a, _) in api.SIGNATURES.items()}
    test_side = mc33_capi.signatures(C.c_double if double else C.c_float, mirror("_GRD", flavour), mirror("surface", flavour),
                                     mirror("MC33", flavour) or mirror("MC33", flavour[:3]))  # (only pointers to MC33 occur)
    for name, row in test_side.items():
        assert name not in rows or ctypes_signature(*rows[name]) == ctypes_signature(*row), name
        rows[name] = row
    return rows


def declared_in_mc33_hip_h():
    return set(re.findall(r"\b(mc33hip_\w+)\(", open(os.path.join(ROOT, "include", "mc33_hip.h")).read()))


def signatures(flavour):
    if flavour not in _signatures:
        _signatures[flavour] = c_signatures(sorted(set(tables(flavour)) | declared_in_mc33_hip_h()), FLAVOURS[flavour][0])
    return _signatures[flavour]


def test_every_struct_mirror_has_the_compilers_layout():
    """one test over all flavours (the message names the flavour and the struct): it stands for the thirteen per-part tests
    of sampled members that it replaced"""
    for flavour in FLAVOURS:
        want = layouts(flavour)
        for ctype, cls in mirrors(flavour):
            size, fields = want[ctype]
            assert C.sizeof(cls) == size, "%s: sizeof(%s) is %d, the header's %s has %d" % (flavour, cls.__name__, C.sizeof(cls), ctype, size)
            for (name, _), member in zip(cls._fields_, members(cls)):
                got = (getattr(cls, name).offset, getattr(cls, name).size)
                assert got == fields[member], "%s: %s.%s at offset %d, %d bytes; the header's %s.%s at %d, %d bytes" % (
                    (flavour, cls.__name__, name) + got + (ctype, member) + fields[member])


def test_every_structure_of_api_py_is_in_the_table():
    classes = set(v for v in vars(api).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure)
    assert classes == set(api.STRUCTS.values()), sorted(c.__name__ for c in classes ^ set(api.STRUCTS.values()))


def test_the_oracles_records_are_the_component_rows():
    """the numpy records of the measure and topology oracles are read from and written to arrays of the two row structs"""
    for record, cls in ((mo.COMPONENT, api.Component), (to.COMPONENT, api.ComponentTopology)):
        assert np.dtype(cls).itemsize == record.itemsize == C.sizeof(cls)
        assert [record.fields[n][1] for n in record.names] == [np.dtype(cls).fields[n][1] for n in record.names]


@pytest.mark.parametrize("name", sorted(tables("f32")))
def test_declared_signature_is_the_headers(name):
    for flavour in FLAVOURS:
        restype, argtypes = tables(flavour)[name]
        got, want = ctypes_signature(restype, argtypes), signatures(flavour)[name]
        assert got == want, "%s (%s): declared %s, the header has %s" % (name, flavour, got, want)


def test_every_function_of_mc33_hip_h_is_declared_or_listed():
    declared, rows = declared_in_mc33_hip_h(), set(api.HIP_API)
    assert set(signatures("f32")) >= declared  # (the probe compiled over every one of them: the expression invented no name)
    assert rows <= declared, sorted(rows - declared)
    assert declared - rows == NOT_CALLED, sorted((declared - rows) ^ NOT_CALLED)


def test_no_module_under_tests_imports_a_test_module():
    found = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            found += ["%s:%d imports %s" % (os.path.basename(path), node.lineno, n) for n in names if n.split(".")[0].startswith("test_")]
    assert not found, "\n".join(found)
