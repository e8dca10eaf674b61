"""The float32 TFLite graph executor (cpx_graph_*, cpx/ml_tools/tflite_graph.py) on the GPU against the float64
evaluation of the same flatbuffer (tests/tflite_eval.py, which reads the Graph only).  The flatbuffers are synthetic
(tests/tflite_build.py): the reference's TFLite runtime and the released weights are not available here, so parity with the
released file itself is pinned only by test_released_model_parity below, which runs where CPX_TFLITE_PARITY_NPZ names a dump."""
import json
import os

import numpy as np
import pytest

import tflite_build as tb
import tflite_eval as te

pytestmark = pytest.mark.gpu

# float32 accumulation against the accumulated magnitude sum |x| |w|: the bound tests/test_cnn_gpu.py holds the
# float32-accurate convolutions to
CONV_REL = 4e-6


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3", device=0)
    yield eng
    eng.close()


def run(engine, blob, x, output=None, channel_map=None):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    plan = build_plan(g, input_shape=x.shape[1:] if channel_map is None else (x.shape[1], x.shape[2], len(channel_map)),
                      output=output, channel_map=channel_map)
    dev = GraphDevice(engine, plan)
    out = dev.forward(torch.from_numpy(np.ascontiguousarray(x)).to(engine.device)).cpu().numpy()
    dev.close()
    return g, plan, out


def one_conv(rng, kh, kw, stride, padding, cin, cout, size, act=tb.RELU):
    m = tb.Model()
    x = m.tensor([1, size, size, cin], name="input")
    m.inputs = [x]
    w = rng.normal(0, np.sqrt(2.0 / (kh * kw * cin)), size=(cout, kh, kw, cin)).astype(np.float32)
    m.outputs = [m.conv(x, w, rng.normal(0, 0.05, size=cout).astype(np.float32), stride, padding, act)]
    return m.finish()


CONV_CASES = [
    # kh, kw, stride, padding, cin, cout, size
    (1, 1, 1, tb.SAME, 192, 2048, 8),
    (1, 1, 2, tb.VALID, 48, 80, 17),
    (3, 3, 2, tb.VALID, 3, 32, 79),
    (3, 3, 1, tb.SAME, 32, 48, 38),
    (3, 3, 2, tb.SAME, 80, 192, 38),
    (3, 3, 1, tb.VALID, 288, 32, 17),
    (5, 5, 1, tb.SAME, 48, 80, 38),
    (5, 5, 2, tb.SAME, 3, 48, 17),
    (1, 7, 1, tb.SAME, 192, 288, 17),
    (7, 1, 1, tb.SAME, 80, 192, 17),
    (7, 1, 2, tb.SAME, 32, 3, 8),
    (1, 3, 1, tb.SAME, 2048, 48, 8),
    (3, 1, 1, tb.SAME, 288, 2048, 3),
    (1, 3, 1, tb.VALID, 32, 32, 3),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "%dx%d_s%d_%s_%dto%d_at%d" % (c[0], c[1], c[2], "SV"[c[3]], c[4], c[5], c[6]))
def test_convolution_against_float64(engine, case):
    kh, kw, stride, padding, cin, cout, size = case
    rng = np.random.default_rng(kh * 100 + kw * 10 + stride + cin + cout + size)
    blob = one_conv(rng, kh, kw, stride, padding, cin, cout, size, act=tb.NONE)
    x = rng.uniform(-1, 1, size=(2, size, size, cin)).astype(np.float32)
    g, plan, got = run(engine, blob, x)
    vals, mag = te.evaluate(g, x, magnitudes=True)
    want = vals[g.outputs[0]]
    assert got.shape == want.shape
    rel = float((np.abs(got - want) / mag[g.outputs[0]]).max())
    print("%s: max |error| / sum |x||w| = %.3g" % (case, rel))
    assert rel < CONV_REL, rel


@pytest.mark.parametrize("act", [tb.RELU, tb.RELU6])
def test_convolution_activation_and_folded_affine(engine, act):
    """CONV_2D -> MUL const -> ADD const (activation): folded into the convolution's scale and shift."""
    rng = np.random.default_rng(5 + act)
    m = tb.Model()
    x = m.tensor([1, 17, 17, 32], name="input")
    m.inputs = [x]
    w = rng.normal(0, 0.1, size=(48, 3, 3, 32)).astype(np.float32)
    y = m.conv(x, w, rng.normal(0, 0.05, size=48).astype(np.float32), 1, tb.SAME, tb.NONE)
    y = m.binary("MUL", y, rng.uniform(0.5, 2.0, size=48).astype(np.float32))
    y = m.binary("SUB", y, rng.normal(0, 1.0, size=48).astype(np.float32), act)
    m.outputs = [y]
    xs = rng.uniform(-3, 3, size=(2, 17, 17, 32)).astype(np.float32)
    g, plan, got = run(engine, m.finish(), xs)
    assert [o.name for o in plan.ops] == ["CONV_2D+MUL+SUB"]
    want = te.evaluate(g, xs)[g.outputs[0]]
    assert float(np.abs(got - want).max()) < 2e-5


@pytest.mark.parametrize("conv_first", [True, False])
def test_channel_sliced_stores_leave_the_neighbours_alone(engine, conv_first):
    """Convolution, average pool (SAME: the border divisor) and max pool write their slices of one concatenated tensor;
    whichever runs last would destroy the others' channels if it stored outside its slice."""
    rng = np.random.default_rng(9)
    m = tb.Model()
    x = m.tensor([1, 17, 17, 20], name="input")
    m.inputs = [x]
    w = rng.normal(0, 0.1, size=(12, 3, 3, 20)).astype(np.float32)

    def conv():
        return m.conv(x, w, rng.normal(0, 0.05, size=12).astype(np.float32), 1, tb.SAME, tb.RELU)

    c = conv() if conv_first else None
    a = m.pool("AVERAGE_POOL_2D", x, 3, 1, tb.SAME)
    p = m.pool("MAX_POOL_2D", x, 3, 1, tb.SAME)
    if c is None:
        c = conv()
    m.outputs = [m.unary("RELU6", m.concat([a, c, p]))]
    xs = rng.uniform(-2, 8, size=(3, 17, 17, 20)).astype(np.float32)
    g, plan, got = run(engine, m.finish(), xs)
    assert not plan.copies()
    want = te.evaluate(g, xs)[g.outputs[0]]
    assert got.shape == want.shape == (3, 17, 17, 52)
    assert float(np.abs(got - want).max()) < 2e-5


@pytest.mark.parametrize("kind,k,stride,padding,size", [("AVERAGE_POOL_2D", 3, 1, tb.SAME, 17), ("AVERAGE_POOL_2D", 3, 1, tb.SAME, 3),
                                                       ("AVERAGE_POOL_2D", 3, 2, tb.SAME, 8), ("MAX_POOL_2D", 3, 2, tb.VALID, 79),
                                                       ("MAX_POOL_2D", 3, 2, tb.SAME, 38), ("AVERAGE_POOL_2D", (2, 5), (2, 1), tb.VALID, 17)])
def test_pools(engine, kind, k, stride, padding, size):
    rng = np.random.default_rng(size)
    m = tb.Model()
    x = m.tensor([1, size, size, 20], name="input")
    m.inputs = [x]
    m.outputs = [m.pool(kind, x, k, stride, padding)]
    xs = rng.uniform(-5, -1, size=(2, size, size, 20)).astype(np.float32)   # negative: a padded zero must never win a maximum
    g, plan, got = run(engine, m.finish(), xs)
    want = te.evaluate(g, xs)[g.outputs[0]]
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) < (0 if kind[0] == "M" else 2e-6) + 1e-30


def test_elementwise_head_and_pad(engine):
    rng = np.random.default_rng(21)
    m = tb.Model()
    x = m.tensor([1, 8, 8, 24], name="input")
    m.inputs = [x]
    a = m.unary("RELU", m.binary("MUL", x, rng.uniform(0.5, 2, size=24).astype(np.float32)))
    b = m.pool("AVERAGE_POOL_2D", m.pad(x, [[0, 0], [1, 1], [1, 1], [0, 0]]), 3, 1, tb.VALID)
    y = m.binary("ADD", a, b, tb.RELU6)
    y = m.binary("SUB", y, a)
    y = m.mean(y, keep_dims=True)
    y = m.reshape(y, [1, 24])
    y = m.dense(y, rng.normal(0, 0.3, size=(40, 24)).astype(np.float32), rng.normal(0, 0.1, size=40).astype(np.float32), tb.RELU)
    y = m.dense(y, rng.normal(0, 0.3, size=(7, 40)).astype(np.float32), rng.normal(0, 0.1, size=7).astype(np.float32))
    m.outputs = [m.softmax(y, 1.5)]
    xs = rng.uniform(-2, 2, size=(4, 8, 8, 24)).astype(np.float32)
    g, plan, got = run(engine, m.finish(), xs)
    want = te.evaluate(g, xs)[g.outputs[0]]
    assert float(np.abs(got - want).max()) < 1e-5 and abs(float(got.sum()) - 4.0) < 1e-4


def samples(n, size, seed):
    """Seeded 0..255 samples that differ in structure, scaled x / 127.5 - 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    out = []
    for s in range(n):
        planes = [127.5 + 110 * np.sin(2 * np.pi * ((s + 1) * xx * (c + 1) + (2 * s + 1) * yy + 0.3 * c)) for c in range(3)]
        img = np.stack(planes, axis=-1) + rng.normal(0, 10, size=(size, size, 3))
        out.append(np.clip(img, 0, 255))
    return (np.stack(out) / 127.5 - 1.0).astype(np.float32)


# Measured on an MI355X (width 1.0, 160 x 160 x 3, N = 3): float32 on the CPU deviates from float64 by 3.49e-6 on the
# logits, the device by 3.45e-6 -- ratio 0.99.
# the device may deviate from float64 by this multiple of what a float32 evaluation of the same graph on the CPU does:
# both are float32 arithmetic on the same values; only the summation order and fused multiply-add differ, and a maximum
# over 3 x 17 logits of one run against another's scatters by a small factor
LOGIT_MULTIPLE = 4.0


def test_inception_v3_whole_network(engine):
    """Measured on an MI355X: see the figures printed below and DESIGN.md section 2."""
    import torch

    blob = tb.inception_v3(17, (), seed=7, width=1.0, head_gain=4.0)
    x = samples(3, 160, seed=11)
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(blob)
    logits_t = g.ops[-1]["inputs"][0]
    v64 = te.evaluate(g, x)
    v32 = te.evaluate(g, x, dtype=torch.float32)
    yard = float(np.abs(v32[logits_t] - v64[logits_t]).max())
    tol = LOGIT_MULTIPLE * yard
    _, _, logits = run(engine, blob, x, output=logits_t)
    _, _, probs = run(engine, blob, x)
    err = float(np.abs(logits - v64[logits_t]).max())
    spread = min(float(np.ptp(v64[logits_t], axis=1).min()), float(np.ptp(v64[logits_t], axis=0).max()))
    print("float32-CPU vs float64: %.3g; device vs float64: %.3g (ratio %.2f); spread of the logits %.3g"
          % (yard, err, err / yard, spread))
    assert spread >= 100 * tol, (spread, tol)   # the logits tell samples and labels apart by far more than the tolerance
    assert err <= tol, (err, yard)
    assert float(np.abs(probs - v64[g.outputs[0]]).max()) <= 1e-3


def test_batch_does_not_matter_and_arena_is_reused(engine):
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    g = Graph(tb.inception_v3(9, (32,), seed=3, width=0.25))
    dev = GraphDevice(engine, build_plan(g))
    assert engine.lib.cpx_release_memory(engine.h) == 0   # the handle's arena is shared: start from none
    x = samples(1, 160, seed=5)
    one = dev.forward(torch.from_numpy(x).to(engine.device)).cpu().numpy()
    five = dev.forward(torch.from_numpy(np.repeat(x, 5, axis=0)).to(engine.device)).cpu().numpy()
    again = dev.forward(torch.from_numpy(np.repeat(x, 5, axis=0)).to(engine.device)).cpu().numpy()
    assert all(np.array_equal(five[k], one[0]) for k in range(5))
    assert np.array_equal(five, again)
    # the arena: what the plan says, what the handle grew to, released and regrown
    assert dev.arena_bytes(5) == 5 * dev.plan.arena_bytes_per_sample == dev.arena_allocated()
    assert engine.lib.cpx_release_memory(engine.h) == 0 and dev.arena_allocated() == 0
    assert np.array_equal(dev.forward(torch.from_numpy(x).to(engine.device)).cpu().numpy(), one)
    assert dev.arena_allocated() == dev.arena_bytes(1)
    dev.close()


def test_wrresnet_and_graph_share_a_handle():
    """A WR-ResNet network and a graph on one handle, forwards alternating: one stream, two arenas; cpx_destroy frees both."""
    import torch

    import cnn_oracle as co
    from cpx.engine import TrackEngine
    from cpx.ml_tools import wrresnet as wr
    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    eng = TrackEngine(model="lepton3", device=0)
    rng = np.random.default_rng(2)
    xw = rng.uniform(0, 255, size=(2, 160, 160, 2)).astype(np.float32)
    w = co.calibrate_bn(wr.random_weights(17, seed=3), xw)
    want_w, _ = co.forward(w, xw)
    net = wr.WRResNetDevice(eng, w, 17)
    g = Graph(tb.inception_v3(9, (), seed=4, width=0.25))
    dev = GraphDevice(eng, build_plan(g))
    xg = samples(2, 160, seed=6)
    want_g = te.evaluate(g, xg)[g.outputs[0]]
    for _ in range(2):
        logits, _ = net.forward(torch.from_numpy(xw).to(eng.device))
        assert float(np.abs(logits.cpu().numpy() - want_w).max()) <= 2e-4
        got = dev.forward(torch.from_numpy(xg).to(eng.device)).cpu().numpy()
        assert float(np.abs(got - want_g).max()) <= 1e-3
    eng.close()   # the network and the graph are still alive: the handle frees them
    net.close()
    dev.close()


def test_channel_map_feeds_three_channels_from_two(engine):
    rng = np.random.default_rng(8)
    blob = one_conv(rng, 3, 3, 1, tb.SAME, 3, 32, 17)
    x2 = rng.uniform(-1, 1, size=(2, 17, 17, 2)).astype(np.float32)
    g, plan, got = run(engine, blob, x2, channel_map=[0, 0, 1])
    want = te.evaluate(g, x2[..., [0, 0, 1]])[g.outputs[0]]
    assert plan.ops[0].name == "CHANNEL_MAP" and float(np.abs(got - want).max()) < 2e-5


def test_released_model_parity(engine):
    """Parity with the reference's runtime on the released file: CPX_TFLITE_PARITY_NPZ names an archive with `model` (the
    path of the .tflite), `inputs` [N, H, W, C] and `outputs` [N, n_labels] dumped where ai_edge_litert runs."""
    path = os.environ.get("CPX_TFLITE_PARITY_NPZ")
    if not path:
        pytest.skip("CPX_TFLITE_PARITY_NPZ is not set: no dump of the released model on this machine")
    z = np.load(path, allow_pickle=False)
    with open(str(z["model"]), "rb") as fh:
        blob = fh.read()
    _, _, got = run(engine, blob, z["inputs"].astype(np.float32))
    assert float(np.abs(got - z["outputs"]).max()) <= 1e-3


@pytest.mark.parametrize("kind", ["conv", "conv_thin", "MAX_POOL_2D", "AVERAGE_POOL_2D"])
def test_sliced_store_leaves_a_sentinel_buffer_untouched(engine, kind):
    """A one-operator graph whose output is a channel slice of a buffer filled with a sentinel: the slice holds the
    result, every other channel still holds the sentinel, bit for bit."""
    import torch

    from cpx.ml_tools.tflite_graph import GraphDevice, build_plan
    from cpx.ml_tools.tflite_reader import Graph

    rng = np.random.default_rng(31)
    cin, cout, size = (20, 48, 17) if kind != "conv_thin" else (3, 5, 19)
    if kind.startswith("conv"):
        blob = one_conv(rng, 3, 3, 1, tb.SAME, cin, cout, size)
    else:
        m = tb.Model()
        x = m.tensor([1, size, size, cin], name="input")
        m.inputs = [x]
        m.outputs = [m.pool(kind, x, 3, 2, tb.SAME)]
        blob, cout = m.finish(), cin
    g = Graph(blob)
    xs = rng.uniform(-2, 2, size=(3, size, size, cin)).astype(np.float32)
    want = te.evaluate(g, xs)[g.outputs[0]]
    off, stride = 7, cout + 7 + 38   # the slice neither starts nor ends on a 32-channel tile
    plan = build_plan(g)
    dev = GraphDevice(engine, plan, out_slice=(off, stride))
    sentinel = np.float32(-12345.678)
    out = torch.full((3, want.shape[1], want.shape[2], stride), float(sentinel), dtype=torch.float32, device=engine.device)
    dev.forward(torch.from_numpy(xs).to(engine.device), out=out)
    got = out.cpu().numpy()
    dev.close()
    assert float(np.abs(got[..., off:off + cout] - want).max()) < 2e-5
    assert np.all(got[..., :off] == sentinel) and np.all(got[..., off + cout:] == sentinel)


LABELS17 = ["bird", "cat", "deer", "dog", "false-positive", "hedgehog", "human", "kiwi", "leporidae", "mustelid", "penguin",
            "possum", "rodent", "sheep", "vehicle", "wallaby", "land-bird"]


@pytest.fixture(scope="module")
def inception_model(tmp_path_factory):
    """A width-0.25 Inception-v3 file + sidecar: three input channels fed from the two-channel sample by the channel map."""
    from helpers import GOLDEN

    d = tmp_path_factory.mktemp("inc3")
    with open(os.path.join(GOLDEN, "classify_variants_golden.json")) as fh:
        golden = json.load(fh)
    assert golden["labels"] == LABELS17
    hp = dict(golden["variants"]["inceptionv3_scaling"]["hyperparams"])
    assert hp == {"frame_size": 32, "model_name": "inceptionv3"}
    hp["channels"] = ["thermal", "thermal", "filtered"]
    blob = tb.inception_v3(len(LABELS17), (), seed=13, width=0.25, head_gain=4.0)
    (d / "inc3.tflite").write_bytes(blob)
    with open(d / "inc3.json", "w") as fh:
        json.dump({"labels": LABELS17, "hyperparams": hp, "type": "thermal", "version": "test"}, fh)
    return d, blob, golden["variants"]["inceptionv3_scaling"]


def _inc3_config(d):
    from cpx.config import Config
    from cpx.config.config import ModelConfig

    cfg = Config.get_defaults()
    cfg.tracking["thermal"].denoise = False
    cfg.classify.models = [ModelConfig.load({"id": 9, "name": "inc3", "model_file": str(d / "inc3.tflite")})]
    return cfg


def test_clip_classifier_with_a_lite_interpreter(tmp_path, inception_model):
    """The possum fixture tracked, then classified by ClipClassifier's one-file path with a LiteInterpreter: the network
    inputs are the reference's (tests/golden/classify_variants_golden.json, `inceptionv3_scaling`: the two-channel sample,
    whose thermal channel the channel map repeats), and the predictions are the aggregation of the float64 evaluator's
    probabilities on those inputs, by the oracle chain, at 1e-3."""
    import shutil
    import zlib

    import classify_oracle as co
    from helpers import GOLDEN
    from cpx.classify.clipclassifier import ClipClassifier
    from cpx.ml_tools.interpreter import LiteInterpreter, get_interpreter
    from cpx.ml_tools.tflite_reader import Graph
    from cpx.track.trackextractor import extract_file

    d, blob, gold = inception_model
    g = Graph(blob)
    cfg = _inc3_config(d)
    src = tmp_path / "possum.cptv"
    shutil.copy(os.path.join(GOLDEN, "possum.cptv"), src)
    clip, _, _ = extract_file(src, cfg, False, save_meta=False)

    def evaluator_probs(x2):
        return te.evaluate(g, np.ascontiguousarray(x2[..., [0, 0, 1]]))[g.outputs[0]]

    # ---- the network's inputs and the track scores, on the reference's segments ----
    interp = get_interpreter(cfg.classify.models[0])
    assert isinstance(interp, LiteInterpreter)
    seen = {}
    device_predict = interp.predict

    def predict(x):
        seen["x"] = x.cpu().numpy()
        return device_predict(x)

    interp.predict = predict
    assert len(clip.tracks) == len(gold["possum"]) > 0
    for track, want in zip(clip.tracks, gold["possum"]):
        assert track.get_id() == want["track_id"]
        segs = [np.array(s) for s in want["segments"]]
        pred = interp.classify_track(clip, track, segment_frames=segs)
        x = seen["x"]
        assert list(x.shape) == want["shape"]
        assert [zlib.crc32(np.ascontiguousarray(s).tobytes()) & 0xFFFFFFFF for s in x] == want["crc"]
        probs = evaluator_probs(x)
        got = np.array([p.prediction for p in pred.predictions], dtype=np.float64)
        assert got.shape == probs.shape and float(np.abs(got - probs).max()) <= 1e-3
        assert float(np.ptp(probs, axis=1).min()) > 0.1     # the labels are told apart by far more than the tolerance
        score = co.classified_track(probs, prediction_frames=segs, labels=LABELS17)
        assert float(np.abs(np.array(pred.class_best_score) - score).max()) <= 1e-3
    # ---- the one-file path: metadata JSON through the existing code ----
    meta = ClipClassifier(cfg).process_file(str(src), track=True)
    assert meta and os.path.exists(src.with_suffix(".txt"))
    assert meta["models"][0]["id"] == 9
    H, W = clip.res_y, clip.res_x
    assert len(meta["tracks"]) == len(clip.tracks)
    for tm, track in zip(meta["tracks"], clip.tracks):
        assert tm["id"] == track.get_id()
        (pm,) = tm["predictions"]
        assert pm["model_id"] == 9 and set(pm["all_class_confidences"]) == set(LABELS17)
        segs = [np.array(p["frames"]) for p in pm["predictions"]]
        by_frame = {r.frame_number: r for r in track.bounds_history}
        x, _ = co.preprocess_segments(lambda q: clip.frame_buffer.get_frame(q).thermal,
                                      lambda q: clip.frame_buffer.get_frame(q).filtered.astype(np.float64),
                                      by_frame, track.bounds_history, segs, 32, (1, 1, W - 2, H - 2))
        x = (np.asarray(x, np.float32) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
        score = co.classified_track(evaluator_probs(x), prediction_frames=segs, labels=LABELS17)
        got = np.array([pm["all_class_confidences"][l] for l in LABELS17])
        assert np.abs(got - np.round(score, 3)).max() <= 1e-3 + 1e-9
        assert pm["tag"] == LABELS17[int(np.argmax(score))]
