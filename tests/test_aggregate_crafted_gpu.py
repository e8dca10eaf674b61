"""cpx_aggregate_predictions on crafted cases (tests/aggregate_crafted.py) against the float32 statement of the
reference's aggregation, which tests/test_aggregate_crafted_cpu.py pins to the reference's own TrackPrediction: label
counts around the 8-lane blocks of np.sum up to 128, tracks with 0 / 1 / 2 / 5 segments (a first and a last track with
none), a second workgroup, the low-evidence cap with 1 / 6 / 7 distinct frames of 25 and at square_width 1, winners on
and off the false-positive label, no such label, and a total that is not above 0.5.  Bit for bit."""
import ctypes as C

import numpy as np
import pytest

import aggregate_crafted as ac

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in ac.cases()}


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3")
    yield eng
    eng.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_aggregate_kernel_equals_float32_statement(engine, name):
    import torch

    from cpx._lib import CROP_REQ_DTYPE

    case = CASES[name]
    want, want_best = ac.expected(case)
    probs, sample_track, frames = ac.flatten(case)
    n_tracks, L, sq = len(case["probs"]), case["L"], case["square_width"]
    assert n_tracks > 64 and frames.shape[1] == sq * sq
    reqs = np.zeros(frames.size, CROP_REQ_DTYPE)
    reqs["frame"] = frames.reshape(-1)
    reqs["width"] = reqs["height"] = 1
    reqs["track"] = np.repeat(sample_track, sq * sq)
    reqs["sample"] = np.repeat(np.arange(len(probs), dtype=np.int32), sq * sq)
    reqs["tile"] = np.tile(np.arange(sq * sq, dtype=np.int32), len(probs))
    dev = engine.device
    probs_d = torch.from_numpy(probs).to(dev)
    st_d = torch.from_numpy(sample_track).to(dev)
    reqs_d = engine._to_dev(reqs)
    scores = torch.full((n_tracks, L), -7.0, dtype=torch.float32, device=dev)
    best = torch.full((n_tracks,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = engine.lib.cpx_aggregate_predictions(
        engine.h, C.c_void_p(probs_d.data_ptr()), C.c_void_p(st_d.data_ptr()), len(probs), C.c_void_p(reqs_d.data_ptr()),
        n_tracks, L, case["fp_index"], sq, C.c_void_p(scores.data_ptr()), C.c_void_p(best.data_ptr()))
    assert rc == 0, engine._err()
    engine.synchronize()
    got, got_best = scores.cpu().numpy(), best.cpu().numpy()
    diff = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    print("%s: %d of %d tracks differ, max |difference| %.3g" % (name, len(diff), n_tracks,
                                                                float(np.abs(got - want).max())))
    assert len(diff) == 0, (name, diff[:10], [len(case["probs"][t]) for t in diff[:10]])
    assert np.array_equal(got_best, want_best)
