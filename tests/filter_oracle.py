"""The component compaction of include/mc33_hip.h (mc33hip_compact_components) restated in numpy - keep flags, a
cumulative sum, fancy indexing - and the selection rule of include/marching_cubes_33.h (MC33_select_components) restated beside
it.  Integers and rows moved as they are: nothing here has a tolerance.  numpy only."""
import numpy as np

NONE = 0xFFFFFFFF


class Compacted:
    """V, N, T (uint32), attrs (list), vmap (uint32 [nV]: new[v], NONE where dropped), nV_out, nT_out, components_kept, and
    left_out = the triangles counted and left out (invalid ones, and kept ones that name a vertex that is not kept)"""


def compact(V, N, T, labels, roots, invert=False, attrs=()):
    V, N = np.asarray(V), np.asarray(N)
    nV = V.shape[0]
    T = np.asarray(T).reshape(-1, 3).astype(np.int64)
    labels = np.asarray(labels).astype(np.int64) & 0xFFFFFFFF
    valid = (T < nV).all(axis=1) if T.shape[0] else np.zeros(0, bool)
    referenced = np.zeros(nV, bool)
    referenced[T[valid].reshape(-1)] = True
    is_root = np.zeros(nV, bool)
    is_root[np.asarray(roots, np.int64)] = True
    selected = np.zeros(nV, bool)
    inside = labels < nV  # (a label outside the array is nobody's root)
    selected[inside] = is_root[labels[inside]]
    selected ^= bool(invert)
    keep = referenced & selected
    new = np.cumsum(keep) - keep  # the number of kept u < v
    first = np.zeros(T.shape[0], bool)
    first[valid] = keep[T[valid][:, 0]]
    whole = np.zeros(T.shape[0], bool)
    whole[valid] = keep[T[valid]].all(axis=1)
    out = Compacted()
    out.V, out.N = V[keep], N[keep]
    out.attrs = [np.asarray(a)[keep] for a in attrs]
    out.T = new[T[whole]].astype(np.uint32).reshape(-1, 3)
    out.vmap = np.where(keep, new, NONE).astype(np.uint32)
    out.nV_out, out.nT_out = int(np.count_nonzero(keep)), int(np.count_nonzero(whole))
    out.components_kept = int(np.count_nonzero(keep & (labels == np.arange(nV))))
    out.left_out = int(T.shape[0] - np.count_nonzero(valid)) + int(np.count_nonzero(first & ~whole))
    out.keep = keep
    return out


def select(table, topo=None, min_triangles=0, min_area=0.0, min_abs_volume=0.0, largest=0, closed_only=False):
    """the roots MC33_select_components keeps, ascending (uint32); None where it returns -1"""
    if closed_only and topo is None:
        return None
    ok = (table["nT"] >= min_triangles) & (table["area"] >= min_area) & (np.abs(table["volume"]) >= min_abs_volume)
    if closed_only:
        ok &= topo["boundary_edges"] == 0
    rows = np.nonzero(ok)[0]
    if largest and rows.size > largest:
        # the most triangles first, ties to the smaller root
        rows = sorted(rows.tolist(), key=lambda k: (-int(table["nT"][k]), int(table["root"][k])))[:largest]
    return np.sort(table["root"][np.asarray(rows, np.int64)].astype(np.uint32))
