"""The work split of the emit passes restated in plain Python, from a launch shape (mc33hip_emit_shape) to who takes what:
which batches every wave of k_emit_vertices walks (XcdBatchWalk, mc33_emit.hip.h), which 256-record chunks every block of
k_emit_fast_triangles takes (XcdWalk), and how many rounds the grid-stride loops of the two slow kernels make.  The tests use it
two ways: test_emit_shapes_cpu.py checks the walks themselves (a partition of the work for every grid the host launches, a
hole for a grid it must not launch), test_gpu_emit_shapes.py feeds it the shapes the device reports and keeps book of the
walk lengths and rounds its cases reached.  Nothing here looks at the library."""

VERTEX_SHAPES = (8, 16, 32, 64)  # MC33_HIP_EMIT_V_BLOCKS of the GPU test
WAVES = 4                        # waves of a block


def round8(n):
    """a grid as the host launches it: whole rounds of the 8 XCDs (read_switches, enqueue_emit)"""
    return (int(n) + 7) & ~7


def batch_walk(nbatch, blocks):
    """XcdBatchWalk: the batches of every wave of a k_emit_vertices grid of `blocks` blocks, [block * 4 + wave] -> [batch, ...]"""
    per_xcd = (nbatch + 7) // 8
    blocks_per_xcd = (blocks + 7) >> 3
    walks = []
    for block in range(blocks):
        xcd, slot = block & 7, block >> 3
        end = min((xcd + 1) * per_xcd, nbatch)
        for wave in range(WAVES):
            first = xcd * per_xcd + slot * 4 + wave
            stride = blocks_per_xcd * 4
            walk, t = [], 0
            while first + t * stride < end:  # at(t) = first + t * stride
                walk.append(first + t * stride)
                t += 1
            walks.append(walk)
    return walks


def record_walk(n, blocks):
    """XcdWalk: the 256-record chunks of every block of a k_emit_fast_triangles grid of `blocks` blocks, [block] -> [chunk, ...]
    (a chunk is taken when its first record lies below the walk's end: thread 0 of the block has work)"""
    chunks = (n + 255) // 256
    per_xcd = (chunks + 7) // 8
    blocks_per_xcd = (blocks + 7) >> 3
    walks = []
    for block in range(blocks):
        xcd, slot = block & 7, block >> 3
        c0 = xcd * per_xcd
        end = min((c0 + per_xcd) * 256, n)
        first, stride = (c0 + slot) * 256, blocks_per_xcd * 256
        walk, e = [], first
        while e < end:
            walk.append(e // 256)
            e += stride
        walks.append(walk)
    return walks


def slow_rounds(n, blocks, slots):
    """(rounds of block 0's loop over n slow records, fell back): k_emit_slow (slots false) takes 256 records per block and
    round; k_emit_slow_slots 16 per block and round, and goes through the list with a thread per record - the fallback - when
    n > 32 * blocks"""
    ceil = lambda a, b: (a + b - 1) // b
    if not slots:
        return ceil(n, blocks * 256), False
    if n > 32 * blocks:
        return ceil(n, blocks * 256), True
    return ceil(n, blocks * 16), False


def walk_lengths(nbatch, blocks):
    """the set of walk lengths over the waves that have work, 4 standing for 'at least 4'"""
    return {min(len(w), 4) for w in batch_walk(nbatch, blocks) if w}


def triangle_rounds(n, blocks):
    return max([len(w) for w in record_walk(n, blocks)] or [0])
