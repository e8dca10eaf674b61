"""The handle's growable device buffers (csrc/cpx_internal.h: DeviceBuffer): a buffer that grows between two calls, one
that cpx_release_memory gave back, and one a refused call must leave alone, never change a result.  Everything here is
integer or deterministic work compared bit for bit with an engine whose buffers were allocated once, at the final
size: no tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (6, 12, 9)  # frames per clip; clip 0 alone is the B = 1 call that sizes the buffers first


def make_clip(seed, n):
    """Background noise and, from the second frame on, one warm blob that walks: components and a track for certain."""
    from cpx import synth

    clip = synth.make_clip(np.random.default_rng(seed), n, max_blobs=0).astype(np.float32)
    yy, xx = np.mgrid[0:120, 0:160].astype(np.float32)
    for t in range(1, n):
        cy, cx = 30.0 + 6.0 * t + seed, 40.0 + 8.0 * t
        clip[t] += 300.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 5.0 * 5.0))
    return np.rint(clip).astype(np.uint16)


@pytest.fixture(scope="module")
def clips():
    return [make_clip(s, n) for s, n in enumerate(LENGTHS)]


def new_engine():
    from cpx.engine import TrackEngine

    return TrackEngine(model="lepton3")  # 160 x 120


def batch(eng, some):
    frames = np.concatenate(some)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in some])]).astype(np.int32)
    return eng.upload_frames(frames), offs, eng.make_meta(len(frames))


def run_track(eng, some):
    """-> (result, what the call left: records, components per frame, every clip's background state)"""
    dev, offs, meta = batch(eng, some)
    r = eng.track_batch(dev, offs, meta)
    r.check()
    out = {"info": r.info.tobytes(), "comps": [r.components(f).tobytes() for f in range(r.total)]}
    for b in range(len(some)):
        bg, w, avg = eng.get_background(b)
        out["bg%d" % b] = (bg.tobytes(), w.tobytes(), avg)
    assert sum(len(c) for c in out["comps"]) > 0
    return r, out


def run_assoc_final(eng, r, some):
    """cpx_associate_batch, then cpx_finalize_tracks.  The engine's max_frames is 4,096: the end-of-clip scalars take
    B x 4,096 x 20 bytes (80 KB per clip), the association's arrays well under 40 KB per clip (64 components x 16 active
    tracks x 24-byte scores is the largest), so the second call finds the shared buffer too small and grows it."""
    import torch

    from cpx.tracking import make_filter_params

    _, offs, meta = batch(eng, some)
    B = len(some)
    a = eng.associate_batch(r, offs, meta)
    a.check()
    pool, tracks, ntr, status, regions, rcounts = a._fetch()
    assert int(ntr.sum()) > 0
    mt = a.params.max_tracks
    fp = make_filter_params(max_active_tracks=a.params.max_active_tracks, max_tracks_per_clip=mt)
    with eng._own_stream():
        summ = torch.zeros(B * mt * 30, dtype=torch.int32, device=eng.device)
        counts = torch.zeros((B, 4), dtype=torch.int32, device=eng.device)
    rc = eng.lib.cpx_finalize_tracks(eng.h, C.byref(fp), offs.ctypes.data_as(C.POINTER(C.c_int32)),
                                     C.c_void_p(meta.ctypes.data), B, C.c_void_p(a.pool_dev.data_ptr()),
                                     C.c_void_p(a.tracks_dev.data_ptr()), C.c_void_p(a.ntracks_dev.data_ptr()),
                                     C.c_void_p(summ.data_ptr()), C.c_void_p(counts.data_ptr()))
    assert rc == 0, eng._err()
    eng.synchronize()
    return {"pool": pool.tobytes(), "tracks": tracks.tobytes(), "ntr": ntr.tobytes(), "status": status.tobytes(),
            "regions": [regions[f, :rcounts[f]].tobytes() for f in range(len(rcounts))],
            "summaries": summ.cpu().numpy().tobytes(), "counts": counts.cpu().numpy().tobytes()}


@pytest.fixture(scope="module")
def fresh(clips):
    """The B = 3 batch on an engine that never held smaller buffers: what every test below compares with."""
    eng = new_engine()
    r, track = run_track(eng, clips)
    assoc = run_assoc_final(eng, r, clips)
    del r
    eng.close()
    return track, assoc


def test_growth_keeps_results(clips, fresh):
    eng = new_engine()
    r, _ = run_track(eng, clips[:1])       # B = 1 sizes the workspace, the schedule ...
    run_assoc_final(eng, r, clips[:1])     # ... and the association / end-of-clip buffer
    r, track = run_track(eng, clips)       # B = 3: all three grow
    assert track == fresh[0]
    assert run_assoc_final(eng, r, clips) == fresh[1]
    del r
    eng.close()


def ir_frames():
    H, W = 33, 64  # the smallest shape of tests/test_ir_gpu.py, its six densities
    rng = np.random.default_rng(H * 1000 + W)
    return np.stack([(rng.random((H, W)) < d).astype(np.uint8) * 255 for d in (0.0, 0.01, 0.3, 0.6, 0.9, 1.0)])


def test_release_and_reuse(clips, fresh):
    import torch

    from cpx._lib import CpxError

    eng = new_engine()
    ir_dev = torch.from_numpy(ir_frames()).to(eng.device)

    def three_calls():
        r, track = run_track(eng, clips)
        assoc = run_assoc_final(eng, r, clips)
        counts, comps, _ = eng.ir_detect(ir_dev, 0, 17 * 32)
        return track, assoc, counts.tobytes(), [comps[i, :counts[i]].tobytes() for i in range(len(counts))]

    before = three_calls()
    assert before[:2] == fresh
    assert eng.lib.cpx_release_memory(eng.h) == 0
    with pytest.raises(CpxError) as ei:
        eng.get_background(0)
    assert ei.value.code == -1
    arena = C.c_size_t(1)
    assert eng.lib.cpx_graph_arena_allocated(eng.h, C.byref(arena)) == 0 and arena.value == 0
    assert three_calls() == before
    eng.close()


def test_refused_resume_leaves_the_workspace_alone(clips, fresh):
    import torch

    eng = new_engine()
    clip = clips[0]
    n = len(clip)
    dev = eng.upload_frames(clip)
    meta = eng.make_meta(n)
    with eng._own_stream():
        comps = torch.zeros(n * eng.cap * 8, dtype=torch.int32, device=eng.device)
        info = torch.zeros(n * 20, dtype=torch.int32, device=eng.device)
        filt = torch.zeros((n, eng.height, eng.width), dtype=torch.float32, device=eng.device)

    def track_frame(n_prev, n_frames, filtered):
        return eng.lib.cpx_track_frame(eng.h, C.c_void_p(dev.data_ptr()), C.c_void_p(meta.ctypes.data), n_prev, n_frames,
                                       C.c_void_p(comps.data_ptr()), C.c_void_p(info.data_ptr()), None,
                                       C.c_void_p(filtered.data_ptr()) if filtered is not None else None, None)

    assert track_frame(0, 4, filt) == 0
    assert track_frame(4, 6, None) == -1  # without filtered_dev the state needs a larger workspace than the stream's
    assert "the stream's workspace is gone" in eng._err()
    eng.synchronize()
    r, track = run_track(eng, clips)
    assert track == fresh[0]
    del r
    eng.close()
