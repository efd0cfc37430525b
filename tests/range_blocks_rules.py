"""numpy restatement of the block table and of the block verdicts (include/mc33_hip.h: mc33hip_range_blocks,
mc33hip_block_words), for tests/test_gpu_range_blocks.py.  No GPU is touched here.

A strip is one plane of one tile's footprint: y tile yt starts at sample row 63 yt and has min(64, rows left) sample rows, row
segment seg starts at sample 256 seg.  Its 20 blocks: entry 4 g + k is the sample rows 16 g .. 16 g + 15 of the strip and the
samples 64 k .. 64 k + 63 of the segment, entry 16 + g the halo column (sample 256 seg + 256) over the rows of group g.  Rows past
the strip's last row are that row, samples past the grid's last column are that column: what the sweep's loads would return."""
import warnings

import numpy as np

BLOCKS = 20
UNWRITTEN = np.uint64(0xFFFFFFFFFFFFFFFF)


def dims(shape):
    return (shape[1] - 1 + 62) // 63, (shape[2] - 1 + 255) // 256


def block_index(shape, yt, seg, j):
    """(rows, columns) of entry j of the strip (yt, seg): index arrays into a plane, clamped as the sweep clamps its addresses"""
    ny, nx = shape[1] - 1, shape[2] - 1
    y0 = 63 * yt
    nrows = min(64, ny + 1 - y0)
    g = j // 4 if j < 16 else j - 16
    rows = y0 + np.minimum(16 * g + np.arange(16), nrows - 1)
    if j < 16:
        cols = np.minimum(256 * seg + 64 * (j % 4) + np.arange(64), nx)
    else:
        cols = np.array([min(256 * seg + 256, nx)])
    return rows, cols


def numpy_blocks(a, real):
    """[plane][yt][seg][entry]{min, max} of the samples converted to `real`; {-inf, +inf} where a block holds a NaN"""
    r = a.astype(real)
    nyt, nseg = dims(a.shape)
    t = np.empty((a.shape[0], nyt, nseg, BLOCKS, 2), real)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for yt in range(nyt):
            for seg in range(nseg):
                for j in range(BLOCKS):
                    rows, cols = block_index(a.shape, yt, seg, j)
                    blk = r[:, rows][:, :, cols].reshape(a.shape[0], -1)
                    bad = np.isnan(blk).any(axis=1)
                    t[:, yt, seg, j, 0] = np.where(bad, -np.inf, np.nanmin(blk, axis=1))
                    t[:, yt, seg, j, 1] = np.where(bad, np.inf, np.nanmax(blk, axis=1))
    return t


def codes(blocks, iso):
    """[plane][yt][seg][entry]: 0 live, 1 all samples strictly below the isovalue, 2 all strictly above - compared in the table's type"""
    v = blocks.dtype.type(iso)
    return np.where(blocks[..., 1] < v, 1, np.where(blocks[..., 0] > v, 2, 0)).astype(np.uint64)


def numpy_words(blocks, iso):
    """[plane][yt][seg]: two bits per entry"""
    c = codes(blocks, iso)
    w = np.zeros(c.shape[:-1], np.uint64)
    for j in range(BLOCKS):
        w |= c[..., j] << np.uint64(2 * j)
    return w


def live_strips(tiles, dead, shape_planes, nyt, nseg, zs=0, plane0=0):
    """[plane][yt][seg]: the strips the live tiles of a plan read (a tile reads z_lo + 1 .. z_hi, and z_lo in the lowest of a column)"""
    m = np.zeros((shape_planes, nyt, nseg), bool)
    for (seg, yt, z_lo, z_hi), d in zip(tiles.tolist(), dead.tolist()):
        if not d:
            p0 = z_lo if z_lo == zs else z_lo + 1
            m[p0 - plane0:z_hi + 1 - plane0, yt, seg] = True
    return m


def expected_words(blocks, iso, live):
    """the words as the library shows them from a context whose first sweep with blocks this is: all ones where no live tile reads"""
    return np.where(live, numpy_words(blocks, iso), UNWRITTEN)


def left_out(blocks, iso, live):
    """(blocks of the live tiles, those left out below, above)"""
    c = codes(blocks, iso)[live]
    return int(c.size), int((c == 1).sum()), int((c == 2).sum())


def checkerboard(shape):
    """+1 / -1, constant on every block of every strip: quarters of 64 samples in x; in y the row groups of a y tile, numbered on
    through the tiles by 3 per tile so that the row a tile shares with the next one (its group 3, the next one's group 0) has one
    value; alternating from plane to plane.  Cells are cut along every block border and between every pair of planes."""
    z, y, x = np.ogrid[:shape[0], :shape[1], :shape[2]]
    s = x // 64 + (y % 63) // 16 + 3 * (y // 63) + z
    return np.where(s % 2 == 0, 1.0, -1.0).astype(np.float32)
