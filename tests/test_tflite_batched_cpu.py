"""Where ClipClassifier.process(directory, track=True) sends a run: to the batched path (cpx.track.bulk.run_files_bulk)
for models that build a device network -- the WR-ResNet and, now, a TFLite graph (LiteInterpreter) -- and per file for a
served model or models with different normalisation variants.  No GPU: both routes are replaced by recorders."""
import json
import os
import shutil

import pytest

import tflite_build as tb
from helpers import GOLDEN

LABELS = ["bird", "false-positive", "possum"]


@pytest.fixture()
def models(tmp_path):
    from cpx.config.config import ModelConfig
    from cpx.ml_tools import wrresnet as wr

    d = tmp_path / "models"
    d.mkdir()
    (d / "inc3.tflite").write_bytes(tb.inception_v3(len(LABELS), (), seed=13, width=0.25))
    hp = {"frame_size": 32, "model_name": "inceptionv3", "channels": ["thermal", "thermal", "filtered"]}
    with open(d / "inc3.json", "w") as fh:
        json.dump({"labels": LABELS, "hyperparams": hp, "type": "thermal", "version": "test"}, fh)
    wr.save_model(str(d / "wr"), wr.random_weights(len(LABELS), seed=3), LABELS, hyperparams={"frame_size": 32})
    return {
        "graph": ModelConfig.load({"id": 9, "name": "inc3", "model_file": str(d / "inc3.tflite")}),
        "wr": ModelConfig.load({"id": 1, "name": "wr", "model_file": str(d / "wr.npz")}),
        "served": ModelConfig.load({"id": 2, "name": "wr-served", "model_file": str(d / "wr.npz"), "run_over_network": True}),
    }


class _Tracker:
    timings = {"files": 2}


def route(tmp_path, monkeypatch, model_list):
    """-> ("bulk" | "per_file", the ClipClassifier) for a directory of two recordings."""
    from cpx.classify import clipclassifier as cc
    from cpx.config import Config
    from cpx.track import bulk

    clips = tmp_path / "clips"
    clips.mkdir()
    for name in ("possum", "hedgehog"):
        shutil.copy(os.path.join(GOLDEN, name + ".cptv"), clips / (name + ".cptv"))
    taken = []

    def fake_bulk(filenames, config, **kw):
        taken.append(("bulk", sorted(os.path.basename(f) for f in filenames)))
        assert kw["clip_classifier"] is classifier
        return {}, _Tracker()

    def fake_files(self, filenames, **kw):
        taken.append(("per_file", sorted(os.path.basename(f) for f in filenames)))
        return []

    monkeypatch.setattr(bulk, "run_files_bulk", fake_bulk)
    monkeypatch.setattr(cc.ClipClassifier, "process_files", fake_files)
    cfg = Config.get_defaults()
    cfg.classify.models = list(model_list)
    classifier = cc.ClipClassifier(cfg)
    classifier.process(str(clips), track=True)
    assert taken == [(taken[0][0], ["hedgehog.cptv", "possum.cptv"])]
    return taken[0][0], classifier


@pytest.mark.parametrize("name", ["graph", "wr"])
def test_directory_with_a_device_network_takes_the_batched_path(tmp_path, monkeypatch, models, name):
    from cpx.ml_tools.interpreter import LiteInterpreter, WRResNetInterpreter

    way, classifier = route(tmp_path, monkeypatch, [models[name]])
    assert isinstance(classifier.models[models[name].id], LiteInterpreter if name == "graph" else WRResNetInterpreter)
    assert way == "bulk" and classifier.last_run == _Tracker.timings


def test_served_model_goes_per_file(tmp_path, monkeypatch, models):
    way, classifier = route(tmp_path, monkeypatch, [models["served"]])
    assert way == "per_file" and classifier.last_run is None


def test_mixed_normalisation_variants_go_per_file(tmp_path, monkeypatch, models):
    """A WR-ResNet and an Inception-v3 graph in one run: the graph's input scaling (x / 127.5 - 1, applied by the crop
    kernel) makes their limits_flags differ."""
    way, classifier = route(tmp_path, monkeypatch, [models["wr"], models["graph"]])
    flags = [c.limits_flags() for c in classifier.models.values()]
    assert len(flags) == 2 and flags[0] != flags[1]
    assert way == "per_file"


def test_bulk_refuses_a_served_model_with_the_same_words(models):
    from cpx.ml_tools.interpreter import get_interpreter
    from cpx.track import bulk

    for name in ("graph", "wr"):
        bulk.require_device_network(get_interpreter(models[name]))
    served = get_interpreter(models["served"], run_over_network=True)
    with pytest.raises(NotImplementedError) as e:
        bulk.require_device_network(served)
    assert str(e.value) == ("only the WR-ResNet network runs in the batched forward: a TFLite graph model (LiteInterpreter) "
                            "or a model served over the network is classified by the one-file path "
                            "(ClipClassifier.process_file / process_files)")


def test_graph_network_chunk_is_clamped_by_its_arena():
    """BatchPipeline.sample_chunk(): cnn_chunk for a network without a per-sample arena, and as many samples as
    network_bytes holds for one that states arena_bytes_per_sample -- at least one."""
    from cpx.pipeline import BatchPipeline

    class Net:
        eng = None
        arena_bytes_per_sample = 1000

    def pipe(net, **kw):
        p = BatchPipeline.__new__(BatchPipeline)
        p.net, p.cnn_chunk, p.network_bytes = net, kw.get("cnn_chunk", 2048), kw.get("network_bytes")
        return p

    assert pipe(Net()).sample_chunk() == 2048
    assert pipe(Net(), network_bytes=10 ** 9).sample_chunk() == 2048
    assert pipe(Net(), network_bytes=513999).sample_chunk() == 513
    assert pipe(Net(), network_bytes=10).sample_chunk() == 1
    assert pipe(object(), network_bytes=10).sample_chunk() == 2048
    assert pipe(None, network_bytes=10, cnn_chunk=7).sample_chunk() == 7
