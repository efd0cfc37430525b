"""Output arrays inside larger, canaried device tensors, for the GPU tests that hand the emit passes caller-owned memory
(test_gpu_layouts.py, test_gpu_emit_shapes.py): every word of V, N and T holds a canary before the call, the call gets a row
window that is 60 bytes off alignment and 16 rows larger than needed, and afterwards the rows of the surface equal the
reference while every other word still holds the canary.  A vertex or triangle a pass left out shows as a canary row, not as
whatever the allocator held; a row written outside the surface shows too."""
import numpy as np

FRONT, SPARE, EXTRA = 5, 16, 37  # rows in front of the window, spare rows inside its capacity, rows more than needed in all
CANARY32, CANARY64 = 0x7FC0BEEF, 0x7FF8BEEF7FC0BEEF  # NaN bit patterns


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def canaried(nV, nT, v64):
    """V, N [nV + 37, 3] and T [nT + 37, 3] holding the canary in every word"""
    import torch
    V = torch.full((nV + EXTRA, 3), CANARY64, dtype=torch.int64, device="cuda").view(torch.float64) if v64 else \
        torch.full((nV + EXTRA, 3), CANARY32, dtype=torch.int32, device="cuda").view(torch.float32)
    N = torch.full((nV + EXTRA, 3), CANARY32, dtype=torch.int32, device="cuda").view(torch.float32)
    T = torch.full((nT + EXTRA, 3), -1, dtype=torch.int32, device="cuda")
    return V, N, T


def windows(V, N, T, nV, nT):
    """the row windows [5 : 5 + n + 16]: the base 60 bytes off alignment, 16 rows more capacity than needed"""
    w = V[FRONT:FRONT + nV + SPARE], N[FRONT:FRONT + nV + SPARE], T[FRONT:FRONT + nT + SPARE]
    assert all(x.is_contiguous() for x in w) and w[1].data_ptr() % 64 == 60 and w[2].data_ptr() % 64 == 60
    return w


def only_the_rows_were_written(V, N, T, ref, what):
    """rows [5 : 5 + n] equal the reference, every other word of the big tensors still holds the canary"""
    for name, big, want, canary in (("V", V, ref.V, CANARY64 if ref.V.dtype == np.float64 else CANARY32), ("N", N, ref.N, CANARY32),
                                    ("T", T, ref.T, 0xFFFFFFFF)):
        got = words(big.cpu().numpy())
        exp = np.full(got.shape, canary, got.dtype)
        exp[FRONT:FRONT + want.shape[0]] = words(want)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, "%s %s: %d rows differ, the first rows %s (rows %d .. %d are the surface)" % (
            what, name, bad.size, bad[:8].tolist(), FRONT, FRONT + want.shape[0] - 1)
