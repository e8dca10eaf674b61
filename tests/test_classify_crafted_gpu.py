"""cpx_limits_kernel and cpx_crop_kernel on crafted cases (tests/classify_crafted.py), driven through
engine.preprocess_segments as tests/test_classify_gpu.py does:

  * against the CRC32 of the network inputs the REFERENCE built for the same crafted tracks
    (tests/golden/classify_crafted_golden.json, made by tests/golden/make_golden_classify_crafted.py): every model
    variant at frame size 32 and 64, the default also at 48, 96 and 128, single frames also at 96 and 128;
  * against oracle/classify_oracle.py where the reference's tracker cannot produce the input: the filtered frames
    replaced by crafted tensors (all zero, constant, negative and non-integer) and thermal crops that are constant
    above, below and exactly at the frame median, for every flag combination the Python side can produce;
  * the limits record, the order of the requests, and the host-side refusal of out-of-frame requests.

The reference and the oracle both resize with oracle/cv2_shim.py, because cv2 is not installed where the goldens are
made: the bilinear resize is pinned only as far as that shim is, and these tests inherit that.
Every oracle branch used as an expectation here is pinned to a reference-made fixture in tests/test_oracle_golden.py
(the variants and the single-frame path by classify_variants_golden.json and classify_crafted_golden.json, the
post-process path by postprocess_golden.npz); the post-process path combined with another variant is the composition
of branches pinned one by one."""
import json
import os

import numpy as np
import pytest

import classify_crafted as cc
from helpers import GOLDEN, crc

pytestmark = pytest.mark.gpu

POST_PROCESS, THERMAL_DIFF_NORM, NO_DIFF_NORM, ALWAYS_CLIP, SWAP_CHANNELS, TF_SCALING = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def engine():
    from cpx.engine import TrackEngine

    eng = TrackEngine(model="lepton3")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "classify_crafted_golden.json")) as fh:
        return json.load(fh)


def _track(engine, frames):
    dev = engine.upload_frames(frames)
    res = engine.track_batch(dev, np.array([0, len(frames)], np.int32), engine.make_meta(len(frames), cc.TIME_ON, cc.LAST_FFC),
                             want_filtered=True)
    res.check()
    return dev, res


@pytest.fixture(scope="module")
def crafted(engine, gold):
    """The crafted clip tracked on the device: (frames, device frames, track result, filtered on the host)."""
    frames = cc.clip_frames()
    assert crc(frames) == gold["frames_crc"]
    dev, res = _track(engine, frames)
    filtered = res.filtered()
    assert crc(filtered.astype(np.int32)) == gold["filtered_crc"]   # the reference's own filtered frames
    return frames, dev, res, filtered


def variant_flags(tmp_path, variant, single):
    """The limits flags the Python side produces for a variant's hyper-parameters: Interpreter.limits_flags."""
    from cpx import _lib
    from cpx.ml_tools.interpreter import WRResNetInterpreter

    assert (_lib.LIMITS_POST_PROCESS, _lib.LIMITS_THERMAL_DIFF_NORM, _lib.LIMITS_NO_DIFF_NORM, _lib.LIMITS_ALWAYS_CLIP,
            _lib.LIMITS_SWAP_CHANNELS, _lib.LIMITS_TF_SCALING) == (POST_PROCESS, THERMAL_DIFF_NORM, NO_DIFF_NORM,
                                                                   ALWAYS_CLIP, SWAP_CHANNELS, TF_SCALING)
    hp = cc.VARIANTS[variant]
    with open(tmp_path / "m.json", "w") as fh:
        json.dump({"labels": ["a", "false-positive"], "hyperparams": dict(hp, frame_size=32), "type": "thermal"}, fh)
    other = hp.get("model_name", "wr-resnet") != "wr-resnet"
    return WRResNetInterpreter(tmp_path / "m.npz", run_over_network=other, load_model=False).limits_flags(single)


def requests(track_list, single):
    """-> refs, track offsets, reqs, n_samples, [sample range per track]; as Interpreter._device_preprocess builds
    them: one ref per usable region (in_segment where sampled), one request per tile."""
    from cpx._lib import CROP_REQ_DTYPE, REGION_REF_DTYPE

    refs, offs, reqs, spans, sample = [], [0], [], [], 0
    for ti, t in enumerate(track_list):
        segs = [[r.frame_number] for r in cc.usable(t["regions"])] if single else t["segments"]
        used = {f for s in segs for f in s}
        for r in cc.usable(t["regions"]):
            refs.append((r.frame_number, r.x, r.y, r.width, r.height, 1 if r.frame_number in used else 0))
        offs.append(len(refs))
        first = sample
        for seg in segs:
            for tile, fn in enumerate(seg):
                r = t["regions"][fn]
                reqs.append((fn, r.x, r.y, r.width, r.height, ti, sample, tile))
            sample += 1
        spans.append((first, sample))
    return (np.array(refs, dtype=REGION_REF_DTYPE), np.array(offs, np.int32), np.array(reqs, dtype=CROP_REQ_DTYPE),
            sample, spans)


def oracle_kwargs(variant):
    hp = cc.VARIANTS[variant]
    return dict(diff_norm=hp.get("diff_norm", True), thermal_diff_norm=hp.get("thermal_diff_norm", False),
                channels=tuple(hp.get("channels", ["thermal", "filtered"])),
                tf_scaling=hp.get("model_name", "wr-resnet") == "inceptionv3")


def oracle_inputs(frames, filtered, track, variant, fs, single, post):
    import classify_oracle as co

    kw = oracle_kwargs(variant)
    thermal_of, filtered_of = (lambda q: frames[q]), (lambda q: filtered[q])
    if single:
        return co.preprocess_frames(thermal_of, filtered_of, track["regions"], cc.usable(track["regions"]), fs, cc.CROP, **kw)
    by_frame = {r.frame_number: r for r in track["regions"]}
    if post:
        kw["thermal_diff_norm"] = False   # post_process_file never computes thermal limits (clipclassifier.py:465)
    return co.preprocess_segments(thermal_of, filtered_of, by_frame, track["regions"], track["segments"], fs, cc.CROP,
                                  post_process=post, **kw)


def check_limits(limits, frames, filtered, track_list, single, post):
    """The limits record of every track against the oracle's get_limits / get_thermal_limits / post_process_limits and
    the reference's clip test."""
    import classify_oracle as co

    for lim, t in zip(limits, track_list):
        by_frame = {r.frame_number: r for r in t["regions"]}
        if post:
            sampled = {f: by_frame[f] for s in t["segments"] for f in s}
            mn, mx = co.post_process_limits(sampled, lambda q: filtered[q])
        else:
            mn, mx = co.get_limits(t["regions"], lambda q: filtered[q])
            tmn, tmx = co.get_thermal_limits(t["regions"], lambda q: frames[q])
            assert (lim["therm_min"], lim["therm_max"]) == (np.float32(tmn), np.float32(tmx)), t["name"]
        assert (lim["filt_min"], lim["filt_max"]) == (np.float32(mn), np.float32(mx)), (t["name"], lim, mn, mx)
        want_clip = 1 if (single or post) else int(cc.clip_at_zero_expected(frames, t))
        assert lim["clip_at_zero"] == want_clip, t["name"]


# ---------------------------------------------------------------------------------------------------------------------
# against the reference's network inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,fs", cc.RUNS)
def test_crafted_inputs_equal_reference(tmp_path, engine, gold, crafted, variant, fs):
    frames, dev, res, filtered = crafted
    track_list = cc.tracks()
    hit = cc.coverage(fs, track_list)    # a later edit cannot thin the list
    assert {"whole", "left", "right", "top", "bottom", "both_y"} <= hit
    run = gold["runs"][cc.run_key(variant, fs)]
    single = cc.VARIANTS[variant].get("square_width", 5) == 1
    refs, offs, reqs, ns, spans = requests(track_list, single)
    x, limits = engine.preprocess_segments(dev, res, refs, offs, reqs, ns, frame_size=fs, square_width=1 if single else 5,
                                           limits_flags=variant_flags(tmp_path, variant, single))
    x = x.cpu().numpy()
    for t, (s0, s1), want in zip(track_list, spans, run["tracks"]):
        got = [crc(s) for s in x[s0:s1]]
        assert len(got) == len(want["crc"])
        bad = [i for i, (a, b) in enumerate(zip(got, want["crc"])) if a != b]
        if bad:
            i, s = bad[0], x[s0 + bad[0]]
            raise AssertionError("%s fs %d track %s: %d of %d samples differ; sample %d min/max/mean %.6f %.6f %.6f, "
                                 "reference %.6f %.6f %.6f" % (variant, fs, t["name"], len(bad), len(got), i, s.min(), s.max(),
                                                               s.astype(np.float64).mean(), want["min"][i], want["max"][i],
                                                               want["mean"][i]))
    check_limits(limits, frames, filtered, track_list, single, False)
    if not single:
        assert [int(c) for c in limits["clip_at_zero"]] == [int(gold["clip_at_zero"][t["name"]]) for t in track_list]


# ---------------------------------------------------------------------------------------------------------------------
# against the oracle, on inputs the reference's tracker cannot produce
# ---------------------------------------------------------------------------------------------------------------------
BLOCKS = {"above": (30, 60, 40), "below": (70, 60, -40), "at": (110, 60, 0)}   # x, y, offset from the frame median


def constant_block_frames():
    """The crafted clip with three 20 x 20 blocks of one value per frame: 40 above, 40 below and exactly AT the frame
    median (which is made an integer by the block itself: 400 equal pixels in the middle of the order statistics)."""
    frames = cc.clip_frames()
    for f in frames:
        for _ in range(4):
            m = int(np.floor(np.median(f)))
            for x, y, d in BLOCKS.values():
                f[y:y + 20, x:x + 20] = m + d
            if np.median(f) == m:
                break
        assert np.median(f) == m
    return frames


def block_tracks():
    out = []
    for name, (x, y, _) in BLOCKS.items():
        out.append(dict(name="const_" + name, regions=[cc.Region(t, x, y, 20, 20) for t in range(25)],
                        segments=[list(range(25))]))
    base = cc.tracks()
    return out + [base[0], base[7]]   # one geometry track (single pixels, sizes around fs) and limits17


class _Result:
    """What preprocess_segments reads of a track result: crafted filtered frames beside the real frame records."""

    def __init__(self, res, filtered_dev):
        self.filtered_dev, self.info_dev = filtered_dev, res.info_dev


@pytest.fixture(scope="module")
def blocks(engine):
    frames = constant_block_frames()
    dev, res = _track(engine, frames)
    return frames, dev, res, res.filtered()


def crafted_filtered(kind, real):
    rng = np.random.default_rng(77)
    if kind == "zero":
        return np.zeros_like(real)
    if kind == "constant":
        return np.full_like(real, 7.0)
    if kind == "negative_constant":
        return np.full_like(real, -3.5)
    if kind == "negative_fractions":   # all below zero, multiples of 1/8: the default max is floored at 0
        return (-50.0 + np.round(rng.normal(0.0, 5.0, real.shape) * 8) / 8).clip(-90, -0.125).astype(np.float32)
    assert kind == "fractions"         # the tracker's frames shifted by a quarter: both signs, no integers
    return (real + np.float32(0.25)).astype(np.float32)


@pytest.mark.parametrize("kind", ["zero", "constant", "negative_constant", "negative_fractions", "fractions"])
def test_crafted_filtered_and_constant_crops_equal_oracle(tmp_path, engine, blocks, kind):
    import torch

    frames, dev, res, real = blocks
    filtered = crafted_filtered(kind, real)
    assert filtered.dtype == np.float32 and filtered.shape == real.shape
    stand_in = _Result(res, torch.from_numpy(filtered).to(engine.device))
    track_list = block_tracks()
    # the constant crops are what they claim: above, below and at the median (integer arithmetic on the frames)
    for name, (x, y, d) in BLOCKS.items():
        for f in frames[:25]:
            assert np.all(f[y:y + 20, x:x + 20].astype(np.int64) * 2 == int(2 * np.median(f)) + 2 * d)
    fs = 32
    combos = [(v, single, False) for v in cc.VARIANTS for single in [cc.VARIANTS[v].get("square_width", 5) == 1]]
    combos += [(v, False, True) for v in ("default", "thermal_diff_norm", "no_diff_norm", "channels_swapped",
                                          "inceptionv3_scaling")]
    seen_flags = set()
    for variant, single, post in combos:
        flags = variant_flags(tmp_path, variant, single)
        if post:   # ClipClassifier.post_process_file
            flags = POST_PROCESS | (flags & ~THERMAL_DIFF_NORM)
        seen_flags.add(flags)
        refs, offs, reqs, ns, spans = requests(track_list, single)
        x, limits = engine.preprocess_segments(dev, stand_in, refs, offs, reqs, ns, frame_size=fs,
                                               square_width=1 if single else 5, limits_flags=flags)
        x = x.cpu().numpy()
        for t, (s0, s1) in zip(track_list, spans):
            want, _ = oracle_inputs(frames, filtered, t, variant, fs, single, post)
            assert want.shape == x[s0:s1].shape
            assert np.array_equal(x[s0:s1], want), (kind, variant, single, post, t["name"],
                                                    float(np.abs(x[s0:s1] - want).max()))
        check_limits(limits, frames, filtered, track_list, single, post)
    assert len(seen_flags) >= 11


@pytest.mark.parametrize("flags,post", [(0, False), (THERMAL_DIFF_NORM, False), (POST_PROCESS, True)])
def test_limits_record_equals_oracle(engine, crafted, flags, post):
    """filt_min / filt_max / therm_min / therm_max / clip_at_zero of the crafted tracks (1, 16, 17 and 40 usable
    regions, blank and empty ones skipped) on the tracker's filtered frames and on all-negative fractional ones, where
    the default maximum is floored at 0 and the post-process one is not."""
    import torch

    frames, dev, res, real = crafted
    track_list = cc.tracks()
    refs, offs, reqs, ns, _ = requests(track_list, False)
    for filtered in (real, crafted_filtered("negative_fractions", real)):
        stand_in = _Result(res, torch.from_numpy(np.ascontiguousarray(filtered)).to(engine.device))
        _, limits = engine.preprocess_segments(dev, stand_in, refs, offs, reqs[:0], 0, limits_flags=flags)
        assert len(limits) == len(track_list)
        check_limits(limits, frames, filtered, track_list, False, post)
        if filtered is not real:
            assert np.all(limits["filt_max"] == 0) != post and np.all(limits["filt_min"] < 0)


def test_request_order_and_shared_frames(engine, crafted):
    """The requests in shuffled order give the same bytes; two samples over the same frames and rectangles are equal."""
    frames, dev, res, _ = crafted
    base = cc.tracks()
    track_list = [base[0], base[0], base[6]]   # the same track twice, and one whose segment repeats frames
    refs, offs, reqs, ns, spans = requests(track_list, False)
    x, _ = engine.preprocess_segments(dev, res, refs, offs, reqs, ns)
    x = x.cpu().numpy()
    shuffled = reqs[np.random.default_rng(5).permutation(len(reqs))]
    assert not np.array_equal(shuffled, reqs)
    y, _ = engine.preprocess_segments(dev, res, refs, offs, shuffled, ns)
    assert np.array_equal(y.cpu().numpy(), x)
    assert np.array_equal(x[0], x[1]) and not np.array_equal(x[0], x[2])


def test_out_of_frame_requests_are_refused_before_any_launch(engine, crafted):
    import torch

    frames, dev, res, _ = crafted
    track_list = cc.tracks()[:2]
    refs, offs, reqs, ns, _ = requests(track_list, False)
    out = torch.full((ns, 160, 160, 2), 123.0, dtype=torch.float32, device=engine.device)

    def refused(refs_, reqs_, **kw):
        with pytest.raises(ValueError):
            engine.preprocess_segments(dev, res, refs_, offs, reqs_, ns, out=out, **kw)
        engine.synchronize()
        assert bool((out == 123.0).all())

    for field, value in (("x", -1), ("y", -1), ("x", cc.W - 1), ("y", cc.H - 1), ("width", cc.W + 1), ("height", 0),
                         ("frame", cc.T), ("frame", -1), ("track", 2), ("track", -1), ("sample", ns), ("sample", -1),
                         ("tile", 25), ("tile", -1)):
        bad = reqs.copy()
        bad[field][7] = value
        refused(refs, bad)
    bad = reqs.copy()
    bad["tile"][3] = 1                       # in range for 5 x 5 tiles, out of range for a single frame
    refused(refs, bad[:4], square_width=1)
    for field, value in (("x", cc.W - 1), ("y", -2), ("frame", cc.T), ("height", cc.H + 1)):
        bad = refs.copy()
        bad[field][3] = value
        refused(bad, reqs)
    # an empty region stays legal whatever else it says: the limits kernel skips it before reading anything
    ok = refs.copy()
    ok["width"][3], ok["frame"][3], ok["x"][3] = 0, 10 ** 6, -5
    x, _ = engine.preprocess_segments(dev, res, ok, offs, reqs, ns, out=out)
    assert x is out and not bool((out == 123.0).any())
