"""bench.py --dump-outputs: dump_outputs writes what one step handed its caller as float32 / float64 .npy files, at
samples drawn from a fixed seed (the same files for the same inputs), within 64 MB.  Checked on stand-ins of the step's
TrackBatchResult / BatchResult built from CPU tensors."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Track:
    def __init__(self, rng, total, cap, H, W, labels):
        from cpx._lib import COMPONENT_DTYPE, FRAME_INFO_DTYPE

        info = np.zeros(total, FRAME_INFO_DTYPE)
        info["frame_number"] = np.arange(total)
        info["n_components"] = rng.integers(0, cap + 3, total)   # (> cap: an overflowed frame reports the count found)
        info["threshold"] = rng.random(total)
        info["reserved"] = rng.integers(-9, 9, total)            # never written by the kernel: not dumped
        comps = np.zeros((total, cap), COMPONENT_DTYPE)
        for n in COMPONENT_DTYPE.names:
            comps[n] = rng.integers(0, 100, (total, cap))
        self.info = info
        self.info_dev = torch.from_numpy(info.view(np.int32).copy())
        self.comps_dev = torch.from_numpy(comps.view(np.int32).reshape(-1).copy())
        self.cap, self.total = cap, total
        self.filtered_dev = torch.from_numpy(rng.random((total, H, W), dtype=np.float32))
        self.labels_dev = torch.from_numpy(rng.integers(0, 50, (total, H, W), dtype=np.int32)) if labels else None


class _Batch:
    def __init__(self, rng, B, n_tracks, n_samples):
        from cpx.tracking import TRACK_SUMMARY_DTYPE

        mt = 8
        s = np.zeros(B * mt, TRACK_SUMMARY_DTYPE)
        s["id"] = np.arange(B * mt)
        s["score"] = rng.random(B * mt)
        self.summaries_dev = torch.from_numpy(s.view(np.int32).copy())
        self.counts = rng.integers(0, 9, (B, 4)).astype(np.int32)
        self.n_tracks, self.n_samples = n_tracks, n_samples
        self.track_clip = torch.from_numpy(rng.integers(0, B, (n_tracks, 2), dtype=np.int32))
        self.scores = torch.from_numpy(rng.random((n_tracks, 17), dtype=np.float32))
        self.best = torch.from_numpy(rng.integers(0, 17, n_tracks, dtype=np.int32))
        self.logits = torch.from_numpy(rng.standard_normal((n_samples, 17), dtype=np.float32))
        self.probs = torch.from_numpy(rng.random((n_samples, 17), dtype=np.float32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_e2e(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    from cpx._lib import COMPONENT_DTYPE

    B, T, cap = 40, 30, 6
    rng = np.random.default_rng(3)
    track, batch = _Track(rng, B * T, cap, 12, 16, labels=False), _Batch(rng, B, 25, 31)
    n1 = bench.dump_outputs(str(tmp_path / "a"), torch, np, track, batch, B, T)
    n2 = bench.dump_outputs(str(tmp_path / "b"), torch, np, track, batch, B, T)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert n1 == n2 <= 64 << 20 and sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert {"frames_sampled", "frame_info", "components", "filtered", "counts", "track_summaries", "track_clip", "scores",
            "best", "logits", "probs"} <= set(a) and "labels" not in a
    fr = a["frames_sampled"].astype(np.int64)
    assert fr.size == min(bench.DUMP_INFO_FRAMES, B * T) and np.all(np.diff(fr) > 0)
    assert np.array_equal(a["frame_info"][:, 0], fr)                       # frame_number, the first field
    assert a["frame_info"].shape[1] == len(track.info.dtype.names) - 1      # without `reserved`
    want = np.minimum(track.info["n_components"][fr], cap)
    assert a["components"].shape == (want.sum(), 1 + len(COMPONENT_DTYPE.names))
    f0 = fr[np.nonzero(want)[0][0]]
    rows = a["components"][a["components"][:, 0] == f0]
    comps = track.comps_dev.numpy().view(COMPONENT_DTYPE).reshape(B * T, cap)[f0, : len(rows)]
    assert np.array_equal(rows[:, 1], comps["x"])
    img = a["frames_imaged"].astype(np.int64)
    assert np.isin(img, fr).all() and np.array_equal(a["filtered"], track.filtered_dev.numpy()[img])
    assert np.array_equal(a["scores"], batch.scores.numpy()) and np.array_equal(a["best"], batch.best.numpy())
    assert np.array_equal(a["track_clip"], batch.track_clip.numpy()) and np.array_equal(a["probs"], batch.probs.numpy())


def test_dump_outputs_track_stage_and_row_cap(tmp_path, monkeypatch):
    sys.path.insert(0, REPO)
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 10)
    B, T = 8, 20
    rng = np.random.default_rng(4)
    track = _Track(rng, B * T, 4, 12, 16, labels=True)
    bench.dump_outputs(str(tmp_path / "t"), torch, np, track, None, B, T)
    t = _load(str(tmp_path / "t"))
    img = t["frames_imaged"].astype(np.int64)
    assert t["labels"].dtype == np.float32 and np.array_equal(t["labels"], track.labels_dev.numpy()[img])
    assert "scores" not in t and "counts" not in t
    batch = _Batch(rng, B, 25, 31)
    bench.dump_outputs(str(tmp_path / "e"), torch, np, track, batch, B, T)
    e = _load(str(tmp_path / "e"))
    rows = e["track_rows"].astype(np.int64)
    assert rows.size == 10 and np.array_equal(e["scores"], batch.scores.numpy()[rows])
    assert e["probs"].shape == (10, 17) and e["sample_rows"].size == 10
