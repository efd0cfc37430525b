"""The case atlas: committed witness inputs that reach every reachable unit of the per-cell logic by construction, and the
grids that put them at every grid-face position.  Plain data and helpers (no test module imports another test module).

ROW ATLAS (tests/golden/case_atlas.npz, made by tests/golden/make_case_atlas.py): one witness cell - 8 float32 samples, no
sample equal to the isovalue 0 - per (sign index, pattern offset) pair that mc33o_classify reaches.  A cell's face flags are
bit 0: x = 0, bit 1: y = 0, bit 2: z = 0 (face_flags of mc33_cell.h).  Cells on the 0-faces get FACE records whose ranks are
(table row x face flags), so every witness is placed once at every flag value: row_layout(flags) puts the witnesses at every
other cell position (each keeps its own 8 samples) of a grid whose other samples are FILL, on one side of the isovalue.

RULE ATLAS (tests/golden/rule_atlas.json, made by tests/golden/make_rule_atlas.py): tiny grids of small integers, many of them
equal to the isovalue 0, that between them fire every reachable (face flags, id-source rule word) and (face flags, edge, end)
fall-through of plan_visit, as counted by the MC33_RULE_HOOK of tests/host_emu."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW_ATLAS = os.path.join(GOLDEN, "case_atlas.npz")
RULE_ATLAS = os.path.join(GOLDEN, "rule_atlas.json")

FILL = np.float32(1.0)  # the filler sample of the row layouts (float form; isovalue 0)
ROW_DTYPES = ("f32", "u16", "f64")
NP = {"f32": np.float32, "u16": np.uint16, "f64": np.float64}
U16_ISO, U16_MID, U16_AMP = 32768.0, 32768.0, 30000.0


def load_row_atlas():
    """(index [n] uint8, pattern [n] uint16, cells [n, 2, 2, 2] float32 as [z][y][x], hits [n]: how often the generator's random
    search met the pair), sorted by (index, pattern)"""
    with np.load(ROW_ATLAS) as f:
        return f["index"], f["pattern"], f["cells"], f["hits"]


def pair_keys(index, pattern):
    """one integer per (sign index, pattern offset) pair (pattern offsets are below 4096)"""
    return index.astype(np.int64) * 4096 + pattern.astype(np.int64)


def as_dtype(grid, dtype):
    """A float32 grid around the isovalue 0 (samples in [-1, 1]) as `dtype`: (data, isovalue).  uint16: rint(32768 + 30000 v) at
    isovalue 32768.0."""
    grid = np.asarray(grid, np.float32)
    if dtype == "u16":
        return np.rint(U16_MID + U16_AMP * grid.astype(np.float64)).astype(np.uint16), U16_ISO
    return grid.astype(NP[dtype]), 0.0


def cells_as_line(cells):
    """n independent cells [n, 2, 2, 2] as one 2 x 2 x 2n grid: cell k is the grid's cell x = 2k (the odd cells are junk)"""
    cells = np.asarray(cells)
    return np.ascontiguousarray(cells.transpose(1, 2, 0, 3).reshape(2, 2, 2 * len(cells)))


def classify_cells(oracle, cells, iso):
    """(sign index, pattern offset) of n independent cells through the oracle's mc33o_classify: position does not enter"""
    idx, pat = oracle.classify(cells_as_line(cells), iso)
    return idx[0, 0, ::2], pat[0, 0, ::2]


def random_cells(seed, n):
    """n cells of uniform random float32 samples in [-1, 1) (the universe of the row atlas is what these reach)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.random((n, 2, 2, 2), dtype=np.float32) * np.float32(2.0) - np.float32(1.0))


def _odd_slots(npoints):
    return list(range(1, npoints - 1, 2))  # cell positions 1, 3, ..: samples p, p + 1 are the witness's own


def row_layout_shape(flags, n):
    """(nz, ny, nx) points of the grid that holds n witnesses at face flags `flags` (1..6: sized to n; 0: 10 x 10 x 8 slots)"""
    side = 2 * int(np.ceil(np.sqrt(n))) + 1   # 766 witnesses: 57
    line = 2 * n + 1                          # 766 witnesses: 1533
    return {0: (21, 21, 2 * -(-n // 100) + 1), 1: (side, side, 2), 2: (side, 2, side), 4: (2, side, side),
            3: (line, 2, 2), 5: (2, line, 2), 6: (2, 2, line)}[flags]


def row_layout(flags, cells):
    """(grid [nz, ny, nx] float32, positions [n, 3] = cell (z, y, x) of witness k): the witnesses `cells` each at a cell with face
    flags `flags` (0..6), at every other cell position; everything else FILL"""
    n = len(cells)
    shape = row_layout_shape(flags, n)
    axes = []
    for ax, bit in ((0, 4), (1, 2), (2, 1)):  # z, y, x
        axes.append([0] if flags & bit else _odd_slots(shape[ax]))
    pos = np.array([(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]][:n], np.int64)
    assert len(pos) == n, "layout %d holds %d witnesses, %d wanted" % (flags, len(pos), n)
    grid = np.full(shape, FILL, np.float32)
    for k, (z, y, x) in enumerate(pos):
        grid[z:z + 2, y:y + 2, x:x + 2] = cells[k]
    return grid, pos


def flags_of(shape):
    """face flags of every cell of a grid with `shape` points: [nz - 1, ny - 1, nx - 1]"""
    z, y, x = np.meshgrid(*(np.arange(n - 1) for n in shape), indexing="ij")
    return (x == 0) * 1 + (y == 0) * 2 + (z == 0) * 4


def pairs_at_flags(oracle, data, iso, flags):
    """the set of pair keys the oracle's classification of `data` reaches in cells whose face flags are `flags`"""
    idx, pat = oracle.classify(data, iso)
    m = (flags_of(data.shape) == flags) & (idx != 0) & (idx != 255)
    return set(pair_keys(idx[m], pat[m]).tolist())


# ---- rule atlas ---------------------------------------------------------------------------------------------------------------

def load_rule_atlas():
    """{"grids": [{"shape": [nz, ny, nx], "values": [...]}], "rules": [[flags, rule word], ..], "falls": [[flags, edge, end], ..],
    "unreached": {...}}; values are small integers, isovalue 0"""
    with open(RULE_ATLAS) as f:
        return json.load(f)


def rule_grid(g, dtype="f32"):
    """(data, isovalue) of one witness grid of the rule atlas; uint16: the same integers plus 1000 at isovalue 1000.0"""
    a = np.array(g["values"], np.int64).reshape(g["shape"])
    if dtype == "u16":
        return (a + 1000).astype(np.uint16), 1000.0
    return a.astype(NP[dtype]), 0.0


class OneContext:
    """create_MC33 once, then any sequence of calculate_isosurface on it (the reference's C API); set_data + MC33_grid_changed
    re-upload new samples of the same shape."""

    def __init__(self, lib, data, r0=None, d=None):
        self.lib = lib
        self.G, self.keep = lib.make_grid(data, r0, d)
        self.M = lib.lib.create_MC33(self.G)
        assert self.M

    def surface(self, iso):
        S = self.lib.lib.calculate_isosurface(self.M, self.lib.real(iso))
        assert S
        try:
            return self.lib.copy_surface(S)
        finally:
            self.lib.lib.free_surface_memory(S)

    def set_data(self, data):
        self.keep[...] = data  # (G->F points into this array)
        if hasattr(self.lib.lib, "MC33_grid_changed"):  # (the reference reads G->F on every call)
            self.lib.lib.MC33_grid_changed(self.M)

    def close(self):
        self.lib.lib.free_MC33(self.M)
        self.lib.lib.free_memory_grd(self.G)
