"""Strided layouts of a grid inside a poisoned flat buffer, for the tests of adopted device buffers (test_gpu_layouts.py)
and of the host emulator (mc33_emu.py, test_host_emu.py).

mc33hip_adopt_device takes any pitch >= npx, any slice >= pitch * npy and any base pointer (include/mc33_hip.h); what the
kernels do with a buffer depends on whether base, pitch and slice are multiples of 4 and of 16 bytes.  A layout here is
(pitch, slice, off) in samples: sample (x, y, z) of the grid sits at flat[off + z * slice + y * pitch + x].  Every sample of
the flat array that is not a grid point holds poison - values that change a sign bit, an "equals the isovalue" flag or an
interpolation when they are read as a sample - so a wrong read shows in the result instead of faulting."""
import math

import numpy as np

# (pitch_only is padx_odd with the slice rounded up to 16 bytes: with slice = pitch * npy an odd pitch makes the slice
# term fail together with the pitch term for most types and row counts, so padx_odd alone does not isolate the pitch term)
LAYOUTS = ("dense", "padx16", "padx4", "padx_odd", "pitch_only", "pady", "slice_odd", "offs", "all")
TAIL = 64  # samples the flat array owns behind the full pitch of the last row


def a16(n, itemsize):
    """the smallest m >= n with m * itemsize a multiple of 16"""
    q = 16 // math.gcd(16, int(itemsize))
    return (int(n) + q - 1) // q * q


def layout(name, shape, itemsize):
    """(pitch, slice, off) in samples of the named layout for a grid of `shape` = (npz, npy, npx)"""
    npz, npy, npx = (int(n) for n in shape)
    odd = lambda n: n | 1
    if name == "dense":
        return npx, npx * npy, 0
    if name == "padx16":
        p = a16(npx + 1, itemsize)
        return p, p * npy, 0
    if name == "padx4":  # rows start on 4-byte (double: 8-byte) but not on 16-byte boundaries
        want = 8 if itemsize == 8 else 4
        p = npx + 1
        while p * itemsize % 16 != want:
            p += 1
        return p, p * npy, 0
    if name == "padx_odd":
        p = odd(npx + 1)
        return p, p * npy, 0
    if name == "pitch_only":
        p = odd(npx + 1)
        return p, a16(p * npy, itemsize), 0
    if name == "pady":
        p = a16(npx + 1, itemsize)
        return p, p * (npy + 3), 0
    if name == "slice_odd":
        p = a16(npx + 1, itemsize)
        return p, p * npy + 1, 0
    if name == "offs":
        p = a16(npx + 1, itemsize)
        return p, p * npy, TAIL + 1
    if name == "all":
        p = odd(npx + 3)
        return p, p * (npy + 2) + 1, TAIL + 3
    raise KeyError(name)


def poison_cycle(dtype, isos):
    """The repeating poison pattern for samples of `dtype`: float types NaN, +3e38, -3e38 and, for every isovalue, the
    isovalue itself and its successor; integer types 0, the largest value and, for every isovalue, floor(iso) and floor(iso) + 1
    (kept inside the type's range)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        vals = [np.nan, 3e38, -3e38]
        for v in isos:
            v = dtype.type(v)
            vals += [v, np.nextafter(v, dtype.type(np.inf))]
        return np.array(vals, dtype)
    top = int(np.iinfo(dtype).max)
    vals = [0, top]
    for v in isos:
        f = int(np.floor(v))
        vals += [min(max(f, 0), top), min(max(f + 1, 0), top)]
    return np.array(vals, dtype)


def flat_size(shape, lay):
    pitch, slc, off = lay
    return off + slc * (shape[0] - 1) + pitch * shape[1] + TAIL


def place(data, lay, isos):
    """A flat 1-D array filled completely with poison, with the dense grid data[z, y, x] written into it in layout
    lay = (pitch, slice, off).  The flat array owns the full pitch of the last row plus TAIL samples."""
    data = np.ascontiguousarray(data)
    pitch, slc, off = lay
    npz, npy, npx = data.shape
    assert pitch >= npx and slc >= pitch * npy and off >= 0
    n = flat_size(data.shape, lay)
    cyc = poison_cycle(data.dtype, isos)
    flat = np.resize(cyc, n)
    it = data.dtype.itemsize
    np.lib.stride_tricks.as_strided(flat[off:], data.shape, (slc * it, pitch * it, it))[...] = data
    return flat


def host_view(flat, shape, lay):
    pitch, slc, off = lay
    it = flat.dtype.itemsize
    return np.lib.stride_tricks.as_strided(flat[off:], shape, (slc * it, pitch * it, it), writeable=False)


def to_device(flat):
    """The flat array uploaded once (uint16 / uint32 carried as int16 / int32 bit patterns, as DeviceGrid takes them)"""
    import torch
    if flat.dtype == np.uint16:
        flat = flat.view(np.int16)
    elif flat.dtype == np.uint32:
        flat = flat.view(np.int32)
    return torch.from_numpy(flat).cuda()


def device_view(flat_dev, shape, lay, full_width=False):
    """The grid as a strided window of the flat device tensor; full_width: rows as wide as the pitch (DeviceGrid's npx=)."""
    import torch
    pitch, slc, off = lay
    shape = (shape[0], shape[1], pitch) if full_width else tuple(shape)
    return torch.as_strided(flat_dev, shape, (slc, pitch, 1), off)


def predicates(ptr, pitch, slc, itemsize):
    """What the two host predicates of the library look at, recomputed from a base address and the strides: for 4 and for 16
    bytes the terms (base, pitch, slice) that are multiples of it."""
    return {b: (ptr % b == 0, pitch * itemsize % b == 0, slc * itemsize % b == 0) for b in (4, 16)}
