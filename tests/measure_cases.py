"""The checks the GPU tests share that compare measures taken on the device with tests/measure_oracle.py (tests/test_gpu_measure.py,
tests/test_gpu_mesh_pieces.py, tests/test_gpu_layouts.py): every double sum within the oracle's bound, everything else exactly."""
import struct

import numpy as np

import measure_oracle as mo


def check_sum(what, got, want, bound):
    err = abs(got - want)
    print("%-22s got %.17g  oracle %.17g  |diff| %.3g  bound %.3g" % (what, got, want, err, bound))
    assert err <= bound, "%s: |%.17g - %.17g| = %.3g exceeds the bound %.3g" % (what, got, want, err, bound)


def check_measures(label, got, want):
    assert (got.nV, got.nT) == (want.nV, want.nT)
    check_sum(label + " area", got.area, want.area, want.area_bound)
    check_sum(label + " volume", got.volume, want.volume, want.volume_bound)
    for a in range(3):
        check_sum(label + " moment[%d]" % a, got.moment[a], want.moment[a], want.moment_bound[a])
    assert tuple(got.origin) == tuple(want.origin.tolist())
    assert tuple(got.bbox_min) == tuple(want.bbox_min.tolist()) and tuple(got.bbox_max) == tuple(want.bbox_max.tolist()), (got.bbox_min, got.bbox_max, want.bbox_min, want.bbox_max)
    assert got.has_property == want.has_property
    if want.has_property:
        check_sum(label + " property", got.property_integral, want.property_integral, want.property_bound)
    else:
        assert got.property_integral == 0.0


def all_bits(m):
    return struct.pack("<15d", m.area, m.volume, *m.moment, *m.origin, *m.bbox_min, *m.bbox_max, m.property_integral)


def check_table(label, got, want, ab, wb, totals=None):
    assert got.shape[0] == want.shape[0], "%s: %d components, oracle %d" % (label, got.shape[0], want.shape[0])
    for col in ("root", "nV", "nT"):
        assert np.array_equal(got[col], want[col]), "%s: column %s differs in %d rows" % (label, col, np.count_nonzero(got[col] != want[col]))
    assert np.all(np.diff(got["root"].astype(np.int64)) > 0)
    ea, ew = np.abs(got["area"] - want["area"]), np.abs(got["volume"] - want["volume"])
    def worst(e, b):  # (for the printout only; a row whose terms are all 0 has the bound 0)
        return float(np.max(np.divide(e, b, out=np.where(e > 0, np.inf, 0.0), where=b > 0), initial=0.0))
    print("%s: %d components; worst area diff / bound %.3g, volume %.3g" % (label, got.shape[0], worst(ea, ab), worst(ew, wb)))
    assert np.all(ea <= ab) and np.all(ew <= wb)
    if totals is not None:  # the columns add up to the surface's totals
        check_sum(label + " sum of areas", mo.fsum(got["area"]), totals.area, totals.area_bound)
        check_sum(label + " sum of volumes", mo.fsum(got["volume"]), totals.volume, totals.volume_bound)
        assert int(got["nT"].sum()) == totals.nT
