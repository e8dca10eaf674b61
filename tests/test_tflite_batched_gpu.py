"""TFLite graph models in the batched many-file classify path: the pipeline's chunked forwards give the bits of one
forward, and a directory the metadata files of the per-file path.  Synthetic graphs (tests/tflite_build.py)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

from test_tflite_graph_gpu import LABELS17, _inc3_config, inception_model  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def test_pipeline_chunks_equal_one_forward(engine, inception_model):
    """_front over the possum and hedgehog fixtures, then classify_front with the graph network in chunks of three
    samples: the probabilities are those of one forward over all samples, bit for bit, the track
    scores their aggregation, and a graph network has no logits."""
    import torch

    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter
    from cpx.pipeline import BatchPipeline
    from helpers import load_clip

    d, _, _ = inception_model
    interp = get_interpreter(_inc3_config(d).classify.models[0])
    assert isinstance(interp, LiteInterpreter)
    clips, metas = [], []
    for name in ("possum", "hedgehog"):
        frames, t_on, ffc, bgf, _ = load_clip(name)
        clips.append(frames)
        metas.append(engine.make_meta(frames.shape[0], t_on, ffc, bgf))
    offs = np.concatenate([[0], np.cumsum([c.shape[0] for c in clips])]).astype(np.int32)
    meta = np.concatenate(metas)
    frames_dev = engine.upload_frames(np.concatenate(clips))
    net = interp._network(engine)
    assert net is interp._network(engine) and net.eng is engine and not net.has_logits   # one device graph per engine
    fpi = LABELS17.index("false-positive")
    pipe = BatchPipeline(engine, net, n_labels=len(LABELS17), fp_index=fpi, cnn_chunk=3, limits_flags=interp.limits_flags())
    torch.cuda.current_stream(engine.device).synchronize()
    with torch.cuda.stream(engine.torch_stream()):
        front = pipe._front(frames_dev, offs, meta, None)
        # classify_front's equal chunks: the fixtures plan six samples (possum 1 + 1, hedgehog 4), which cnn_chunk = 3 cuts
        # into 3 + 3 -- equal chunking has no uneven cut of six for any chunk size, so "several chunks" is what is pinned
        chunk = -(-front.n_samples // -(-front.n_samples // pipe.sample_chunk()))
        assert front.n_tracks >= 2 and chunk == 3 and front.n_samples > chunk
        front = pipe.classify_front(front, frames_dev, keep_samples=True)
    assert front.logits is None
    want = net.dev.forward(front.samples_dev)
    assert tuple(front.probs.shape) == (front.n_samples, len(LABELS17)) and torch.equal(front.probs, want)
    assert float(want.min()) >= 0.0 and float(want.max() - want.min()) > 0.1
    scores = torch.empty((front.n_tracks, len(LABELS17)), dtype=torch.float32, device=engine.device)
    best = torch.empty(front.n_tracks, dtype=torch.int32, device=engine.device)
    rc = engine.lib.cpx_aggregate_predictions(
        engine.h, C.c_void_p(want.data_ptr()), C.c_void_p(front.sample_track_dev.data_ptr()), front.n_samples,
        C.c_void_p(front.reqs_dev.data_ptr()), front.n_tracks, len(LABELS17), fpi, 5,
        C.c_void_p(scores.data_ptr()), C.c_void_p(best.data_ptr()))
    assert rc == 0
    engine.synchronize()
    assert torch.equal(front.scores, scores) and torch.equal(front.best, best)
    # the arena budget cuts the chunk, in equal chunks, without changing a bit
    per = net.arena_bytes_per_sample
    tight = BatchPipeline(engine, net, n_labels=len(LABELS17), fp_index=fpi, cnn_chunk=2048, network_bytes=2 * per + per // 2,
                          limits_flags=interp.limits_flags())
    assert tight.sample_chunk() == 2
    with torch.cuda.stream(engine.torch_stream()):
        again = tight.classify_front(front, frames_dev)
    assert torch.equal(again.probs, want)


def _load(p):
    with open(p) as fh:
        m = json.load(fh)
    for k in ("tracking_time", "source", "id"):
        m.pop(k, None)
    for model in m["models"]:
        model.pop("classify_time", None)
    for t in m["tracks"]:
        for pm in t["predictions"]:
            pm.pop("classify_time", None)
            for seg in pm.get("predictions", []):
                seg.pop("predicted_time", None)  # wall clock
    return m


def test_directory_with_a_graph_model_takes_the_batched_path(tmp_path, inception_model):
    """ClipClassifier.process(directory, track=True) with a LiteInterpreter model: the batched path runs (last_run is
    set) and writes, per recording, the file process_files writes under the same (identity) segment draws; a truncated
    recording fails alone."""
    from cpx.classify.clipclassifier import ClipClassifier
    from helpers import GOLDEN, IdentityDraws

    d, _, _ = inception_model
    cfg = _inc3_config(d)
    a, b = tmp_path / "a", tmp_path / "b"
    for dd in (a, b):
        dd.mkdir()
        for name in ("possum", "hedgehog"):
            shutil.copy(os.path.join(GOLDEN, name + ".cptv"), dd / (name + ".cptv"))
    raw = (b / "possum.cptv").read_bytes()
    (b / "truncated.cptv").write_bytes(raw[: len(raw) // 3])
    with IdentityDraws():
        ClipClassifier(cfg).process_files(sorted(str(p) for p in a.glob("*.cptv")))
    cc = ClipClassifier(cfg)
    cc.process(str(b), track=True)
    assert cc.last_run is not None and cc.last_run["files"] == 2
    assert not (b / "truncated.txt").exists()
    for name in ("possum", "hedgehog"):
        ma, mb = _load(a / (name + ".txt")), _load(b / (name + ".txt"))
        assert len(ma["tracks"]) > 0 and ma["tracks"][0]["predictions"][0]["model_id"] == 9
        assert ma == mb, name
