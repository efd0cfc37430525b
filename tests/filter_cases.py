"""What the CPU and the GPU tests of the component filter share (tests/test_filter_cpu.py, tests/test_gpu_filter.py): the
reference's surface of a fixture row with its labels and component tables, made once, and the rows of the issue's table."""
import filter_oracle as fo
import measure_oracle as mo
import topology_oracle as to
from mesh_checks import reference_mesh

_meshes = {}


def mesh(reflibs, name):
    """the reference's surface of a fixture row with its labels and both component tables, computed once and left unchanged"""
    if name not in _meshes:
        data, r0, d, iso, s = reference_mesh(reflibs, name)
        ncomp, unref = mo.FIXTURES[name][2][2:4]
        lab, gc, gu, _ = mo.label_components(s.T, s.nV)
        assert (gc, gu) == (ncomp, unref)
        c = mo.reference_point(r0, d, data.shape)
        tab = mo.component_table(s.V, s.T, lab, c)[0]
        topo = to.component_table(s.T, s.nV, lab)
        for a in (lab, tab, topo):
            a.setflags(write=False)
        _meshes[name] = (data, r0, d, iso, s, lab, tab, topo, c)
    return _meshes[name]


# id -> (fixture, how the roots are chosen from (tab, topo), invert, components kept, nV_out, nT_out; None: the issue gives none)
ROWS = {
    "blobs-every-second": ("blobs", lambda tab, topo: tab["root"][1::2], False, 13, 12600, 25148),
    "blobs-the-1868-row": ("blobs", lambda tab, topo: tab["root"][tab["nT"] == 1868], False, 1, 936, 1868),
    "noise-min16": ("noise", lambda tab, topo: fo.select(tab, min_triangles=16), False, 8, 47990, 101970),
    "noise-not-the-big-one": ("noise", lambda tab, topo: tab["root"][tab["nT"] >= 100], True, 151, 901, 1042),
    "noise-closed": ("noise", lambda tab, topo: fo.select(tab, topo, closed_only=True), False, 86, 548, 752),
    "noise-min-area": ("noise", lambda tab, topo: fo.select(tab, min_area=0.06), False, 2, None, None),
    "quant-min8": ("quant", lambda tab, topo: fo.select(tab, min_triangles=8), False, 9, 15750, 33928),
    "quant-all": ("quant", lambda tab, topo: tab["root"], False, 14, 15775, 33948),
    "quant-closed": ("quant", lambda tab, topo: fo.select(tab, topo, closed_only=True), False, 7, 46, 64),
    "quant-min-volume": ("quant", lambda tab, topo: fo.select(tab, min_abs_volume=5.0), False, 2, None, None),
    "blobs-largest3": ("blobs", lambda tab, topo: fo.select(tab, largest=3), False, 3, None, 5820),
}
SIZED = [k for k, r in ROWS.items() if r[4] is not None and r[5] is not None]  # the eight rows that give both sizes
