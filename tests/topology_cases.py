"""The checks the GPU tests share that compare the topology taken on the device with tests/topology_oracle.py
(tests/test_gpu_topology.py, tests/test_gpu_mesh_pieces.py): integers, field for field and row for row."""
import numpy as np

import topology_oracle as to


def check_surface(label, got, want):
    print("%s: %r" % (label, got))
    for n in to.SURFACE_FIELDS:
        assert getattr(got, n) == want[n], "%s: %s is %d, oracle %d" % (label, n, getattr(got, n), want[n])


def check_table(label, got, want):
    assert got.shape[0] == want.shape[0], "%s: %d components, oracle %d" % (label, got.shape[0], want.shape[0])
    for col in to.COMPONENT.names:
        assert np.array_equal(got[col], want[col]), "%s: column %s differs in %d rows" % (label, col, np.count_nonzero(got[col] != want[col]))
