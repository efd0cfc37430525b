"""mc33hip_extract on a stream the caller named returns when its counts are known, with the emit passes still queued
(include/mc33_hip.h: "Completion").  The outputs are complete in stream order, the counts on return; whatever is not ordered by
the stream - another entry point of the context, the copy stream, close() - waits for the emit first.  Every array is compared
bit for bit with the reference built into oracle/_ref."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY, NZ = 300, 70, 40
SENTINEL = -12345.0


def cos_grid(periods=1.0):
    """cos x + cos y + cos z, [NZ, NY, NX] float32; periods: how many times faster than one period per 8 units the field turns"""
    x = np.cos(np.linspace(-9.0, 9.0, NX) * periods)
    y = np.cos(np.linspace(-4.0, 4.0, NY) * periods)
    z = np.cos(np.linspace(-3.0, 3.0, NZ) * periods)
    return ((x[None, None, :] + y[None, :, None]) + z[:, None, None]).astype(np.float32)


@pytest.fixture(scope="module")
def smooth():
    return cos_grid()


@pytest.fixture(scope="module")
def refs(reflibs, smooth):
    """reference surfaces of the smooth field, made once: isovalue -> Surface"""
    made = {}

    def get(iso):
        if iso not in made:
            made[iso] = reflibs["f32"].isosurface(smooth, iso)
        return made[iso]
    return get


def device_grid(data):
    import torch
    from mc33_c_library_amd import DeviceGrid
    return DeviceGrid(torch.from_numpy(data).cuda())


def outputs(capV, capT, fill=None):
    """V, N [capV, 3] float32 and T [capT, 3] int32 on the device; fill: V and N hold it everywhere, T holds -1"""
    import torch
    V = torch.empty((capV, 3), dtype=torch.float32, device="cuda")
    N = torch.empty_like(V)
    T = torch.empty((capT, 3), dtype=torch.int32, device="cuda")
    if fill is not None:
        V.fill_(fill); N.fill_(fill); T.fill_(-1)
    return V, N, T


def same(V, N, T, cnt, ref):
    assert (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
    v, n, t = V[:cnt.nV].cpu().numpy(), N[:cnt.nV].cpu().numpy(), T[:cnt.nT].cpu().numpy().view(np.uint32)
    assert np.array_equal(t, ref.T)
    assert np.array_equal(v.view(np.uint32), ref.V.view(np.uint32))
    nan = np.isnan(ref.N)
    assert np.array_equal(np.isnan(n), nan) and np.array_equal(n[~nan].view(np.uint32), ref.N[~nan].view(np.uint32))


def test_back_to_back_extractions_into_two_sets(smooth, refs):
    """six calls, alternating isovalues and output sets, nothing waited for in between: each set is copied on the same stream
    right behind its call (a clone: enqueued, not waited for) and looked at only at the end"""
    isos = [0.0, 0.4]
    cap = max(refs(i).nV for i in isos) + 8, max(refs(i).nT for i in isos) + 8
    g = device_grid(smooth)
    sets = [outputs(*cap, fill=SENTINEL) for _ in range(2)]
    kept = []
    for k in range(6):
        V, N, T = sets[k % 2]
        cnt, ok = g.extract_into(isos[k % 2], V, N, T)
        assert ok
        kept.append((V.clone(), N.clone(), T.clone(), cnt, isos[k % 2]))
    for V, N, T, cnt, iso in kept:
        same(V, N, T, cnt, refs(iso))
    g.close()


def test_first_call_grows_the_record_arrays(reflibs):
    """a fresh context whose surface needs more work records than the first guess (a cell in 32, and 65 536): the round that does
    not fit emits nothing and is repeated with room"""
    data = cos_grid(periods=5.0)
    ref = reflibs["f32"].isosurface(data, 0.0)
    g = device_grid(data)
    V, N, T = outputs(ref.nV + 8, ref.nT + 8)
    cnt, ok = g.extract_into(0.0, V, N, T)
    assert ok and cnt.active_cells > (NX - 1) * (NY - 1) * (NZ - 1) // 32 + 65536, "the case must exceed the first capacity"
    same(V, N, T, cnt, ref)
    cnt, ok = g.extract_into(0.0, V, N, T)  # (and once more, the emit of the call before still queued)
    assert ok
    same(V, N, T, cnt, ref)
    g.close()


def test_alias_miss_behind_a_gated_tail(smooth, refs, reflibs):
    """a smooth isovalue - no cell with a corner equal to it: the next tail leaves the slow kernels out - and then one equal to a
    sample: the gated tail misses, nothing is emitted, the tail is made again"""
    g = device_grid(smooth)
    hit = float(smooth[NZ // 2, NY // 2, NX // 3])
    ref_hit = reflibs["f32"].isosurface(smooth, hit)
    V, N, T = outputs(max(refs(0.0).nV, ref_hit.nV) + 8, max(refs(0.0).nT, ref_hit.nT) + 8)
    for iso, ref in ((0.0, refs(0.0)), (0.0, refs(0.0)), (hit, ref_hit), (0.0, refs(0.0))):
        cnt, ok = g.extract_into(iso, V, N, T)
        assert ok
        same(V, N, T, cnt, ref)
    g.close()


def test_capacity_too_small_leaves_the_outputs_alone(smooth, refs):
    import torch
    ref = refs(0.0)
    g = device_grid(smooth)
    V, N, T = outputs(ref.nV - 1, ref.nT + 8, fill=SENTINEL)
    for _ in range(2):  # (the second call: the counters of the first were known and said the same)
        cnt, ok = g.extract_into(0.0, V, N, T)
        assert not ok and (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
    torch.cuda.synchronize()
    assert bool((V == SENTINEL).all()) and bool((N == SENTINEL).all()) and bool((T == -1).all())
    g.close()


def test_close_right_after_a_return(smooth, refs):
    ref = refs(0.0)
    g = device_grid(smooth)
    V, N, T = outputs(ref.nV + 8, ref.nT + 8)
    cnt, ok = g.extract_into(0.0, V, N, T)
    g.close()
    assert ok
    same(V, N, T, cnt, ref)


def test_other_entry_points_right_after_a_return(smooth, refs):
    """count, emit_into, set_timing(2) + timing(): each behind an extraction that has just returned"""
    g = device_grid(smooth)
    r0, r4 = refs(0.0), refs(0.4)
    cap = max(r0.nV, r4.nV) + 8, max(r0.nT, r4.nT) + 8
    V, N, T = outputs(*cap)
    V2, N2, T2 = outputs(*cap)
    cnt, ok = g.extract_into(0.0, V, N, T)
    assert ok
    c4 = g.count(0.4)                       # count behind a return ...
    assert (c4.nV, c4.nT) == (r4.nV, r4.nT)
    same(V, N, T, cnt, r0)                  # (what the extraction wrote stands)
    g.emit_into(V2, N2, T2)                 # ... and the emit of that count
    same(V2, N2, T2, c4, r4)
    cnt, ok = g.extract_into(0.0, V, N, T)
    assert ok
    g.emit_into(V2, N2, T2)                 # emit_into behind a return: the range last counted is the extraction's
    same(V2, N2, T2, cnt, r0)
    cnt, ok = g.extract_into(0.4, V, N, T)
    assert ok
    g.set_timing(2)                         # the timing level behind a return; a timed call then waits for its passes
    g.timing()                              # (no events were recorded for the call before: nothing to report, nothing to wait for)
    same(V, N, T, cnt, r4)
    cnt, ok = g.extract_into(0.0, V, N, T)
    assert ok
    t = g.timing()
    assert t.total_ms > 0.0 and t.sweep_ms > 0.0 and t.emit_ms > 0.0
    same(V, N, T, cnt, r0)
    g.close()


def test_library_stream_is_complete_on_return(smooth, refs):
    """a context on a stream of the library's own: nothing the caller can order its reads by, so the call returns with the
    outputs complete; the test makes no stream call and reads through torch's stream, which that stream is not ordered with"""
    from mc33_c_library_amd.api import OK
    ref = refs(0.0)
    g = device_grid(smooth)
    assert g.lib.mc33hip_own_stream(g.ctx) == OK
    V, N, T = outputs(ref.nV + 8, ref.nT + 8)  # (not filled: a fill on torch's stream would not be ordered before the passes either)
    cnt, ok = g.extract_into(0.0, V, N, T)
    assert ok
    same(V, N, T, cnt, ref)
    g.close()


@pytest.mark.parametrize("many", [False, True], ids=["download_concurrent", "download_many"])
def test_copy_stream_right_after_a_return(smooth, refs, many):
    """the one road to the arrays that the caller's stream does NOT order: the context's copy stream (mc33hip_download_concurrent,
    mc33hip_download_many with concurrent = 1).  Right behind an extraction that returned at its counts the copy must still find
    the arrays complete - the entry point waits for the queued passes first (finish_pending_emit) - and so must a second one"""
    import ctypes as C
    from mc33_c_library_amd.api import OK
    ref = refs(0.0)
    g = device_grid(smooth)
    V, N, T = outputs(ref.nV + 8, ref.nT + 8, fill=SENTINEL)
    import torch
    torch.cuda.synchronize()  # (the fills are done: what the copies find was written by the passes)
    for _ in range(2):
        cnt, ok = g.extract_into(0.0, V, N, T)
        assert ok and (cnt.nV, cnt.nT) == (ref.nV, ref.nT)
        hv, hn, ht = np.empty((cnt.nV, 3), np.float32), np.empty((cnt.nV, 3), np.float32), np.empty((cnt.nT, 3), np.uint32)
        pairs = [(hv, V), (hn, N), (ht, T)]
        if many:
            dst = (C.c_void_p * 3)(*[h.ctypes.data for h, _ in pairs])
            src = (C.c_void_p * 3)(*[d.data_ptr() for _, d in pairs])
            nb = (C.c_size_t * 3)(*[h.nbytes for h, _ in pairs])
            assert g.lib.mc33hip_download_many(g.ctx, C.c_int(3), dst, src, nb, C.c_int(1)) == OK
        else:
            for h, d in pairs:
                assert g.lib.mc33hip_download_concurrent(g.ctx, C.c_void_p(h.ctypes.data), C.c_void_p(d.data_ptr()), C.c_size_t(h.nbytes)) == OK
        assert np.array_equal(ht, ref.T) and np.array_equal(hv.view(np.uint32), ref.V.view(np.uint32))
        nan = np.isnan(ref.N)
        assert np.array_equal(np.isnan(hn), nan) and np.array_equal(hn[~nan].view(np.uint32), ref.N[~nan].view(np.uint32))
        V.fill_(SENTINEL); N.fill_(SENTINEL); T.fill_(-1)  # (on the stream the next extraction is enqueued on: ordered before it)
    g.close()
