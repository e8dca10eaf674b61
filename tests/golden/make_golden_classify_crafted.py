#!/usr/bin/env python3
"""Classification pre-processing golden for CRAFTED tracks (tests/classify_crafted.py): one seeded 160 x 120 clip,
tracked by the REFERENCE under oracle/refharness.py so that frames, filtered frames and medians are its own, then given
tracks whose bounds_history holds chosen rectangles -- single pixels, regions of exactly the frame size, sides that
round on an exact half or to zero, every edge placement, crops above and below the frame median, 1 / 16 / 17 / 40
usable regions -- and classified by the reference's own Interpreter (classify_track; preprocess_frames for the
single-frame models, as make_golden_classify_variants.py does) with a stand-in predict that records the network
input.  Stored per sample: CRC32 and min / max / mean; plus the CRC32 of the reference's filtered frames, the
rectangles and the segments.  -> classify_crafted_golden.json

Also the aggregation cases of tests/test_aggregate_crafted_gpu.py through the reference's TrackPrediction.classified_track
+ Interpreter.track_prediction_from_raw, stored as float32 bit patterns.  -> aggregate_crafted_golden.json

    python tests/golden/make_golden_classify_crafted.py      (build container only)
"""
import json
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in ("oracle", "tests", "classifier-pipeline_amd"):
    sys.path.insert(0, os.path.join(REPO, p))
sys.path.insert(0, HERE)
import refharness as rh  # noqa: E402
import aggregate_crafted as ac  # noqa: E402
import classify_crafted as cc  # noqa: E402
from helpers import encode_cptv  # noqa: E402
from make_golden_classify import LABELS, fake_predict  # noqa: E402


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF)


def reference_tracks(clip, config):
    trackmod, regionmod = rh.ref("track.track"), rh.ref("track.region")
    out = []
    for i, t in enumerate(cc.tracks()):
        track = trackmod.Track(clip.get_id(), id=i + 1, fps=clip.frames_per_second, crop_rectangle=clip.crop_rectangle,
                               tracking_config=config.tracking["thermal"])
        track.start_frame = 0
        track.bounds_history = [regionmod.Region(r.x, r.y, r.width, r.height, centroid=None, mass=r.mass,
                                                 frame_number=r.frame_number, blank=r.blank) for r in t["regions"]]
        out.append(track)
    return out


def classify_runs():
    interp_mod = rh.ref("ml_tools.interpreter")
    frames = cc.clip_frames()
    track_list = cc.tracks()
    for fs in cc.FRAME_SIZES:
        print("fs", fs, "classes", sorted(cc.coverage(fs, track_list)))
    want_clip = {t["name"]: cc.clip_at_zero_expected(frames, t) for t in track_list}
    assert want_clip["clip_on"] and not want_clip["clip_off"], want_clip
    out = {"labels": LABELS, "seed": cc.SEED, "frames_crc": crc(frames), "clip_at_zero": want_clip,
           "tracks": [{"name": t["name"], "regions": [list(r.as_tuple()) for r in t["regions"]], "segments": t["segments"]}
                      for t in track_list], "runs": {}}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "crafted.cptv")
        encode_cptv(path, frames, [16] * cc.T, time_on=cc.TIME_ON, last_ffc=cc.LAST_FFC, model=b"lepton3")
        clip, ex = rh.run_tracking(path, denoise=False)
        assert clip.ffc_frames == [] and tuple(int(v) for v in (clip.crop_rectangle.x, clip.crop_rectangle.y,
                                                                 clip.crop_rectangle.width, clip.crop_rectangle.height)) == cc.CROP
        out["filtered_crc"] = crc(np.stack([np.asarray(clip.get_frame(i).filtered) for i in range(cc.T)]).astype(np.int32))
        tracks = reference_tracks(clip, rh.default_config())
        for variant, fs in cc.RUNS:
            params = dict({"frame_size": fs}, **cc.VARIANTS[variant])
            mfile = os.path.join(td, "model.json")
            json.dump({"labels": LABELS, "hyperparams": params, "type": "thermal", "version": "golden"}, open(mfile, "w"))
            captured = {}

            class Capture(interp_mod.Interpreter):
                TYPE = "capture"

                def shape(self):
                    return 1, (None, 5 * fs, 5 * fs, 2)

                def predict(self, x):
                    captured["x"] = np.array(x, dtype=np.float32, copy=True)
                    return fake_predict(x)

            interp = Capture(mfile)
            single = params.get("square_width", 5) == 1
            per_track = []
            for t, track in zip(track_list, tracks):
                if single:
                    samples = interp.frames_for_prediction(clip, track, frames_per_classify=1)
                    assert [r.frame_number for r in samples] == [r.frame_number for r in cc.usable(t["regions"])]
                    _, pre, _ = interp.preprocess_frames(clip, track, samples)
                    x = np.array(pre, dtype=np.float32)
                else:
                    interp.classify_track(clip, track, segment_frames=[np.array(s) for s in t["segments"]])
                    x = captured["x"]
                side = fs * (1 if single else 5)
                assert x.shape[1:] == (side, side, 2), x.shape
                per_track.append({"crc": [crc(s) for s in x], "min": [float(s.min()) for s in x],
                                  "max": [float(s.max()) for s in x],
                                  "mean": [float(s.astype(np.float64).mean()) for s in x]})
            out["runs"][cc.run_key(variant, fs)] = {"hyperparams": params, "tracks": per_track}
            print(variant, fs, [len(p["crc"]) for p in per_track])
    with open(os.path.join(HERE, "classify_crafted_golden.json"), "w") as fh:
        json.dump(out, fh)


def aggregate_runs():
    """Every case of aggregate_crafted.cases() through the reference: TrackPrediction via track_prediction_from_raw
    (classified_track, then the low-evidence cap), per track.  A track without a segment is never aggregated there
    (classify_track returns None): no entry."""
    interp_mod = rh.ref("ml_tools.interpreter")

    class NoNetwork(interp_mod.Interpreter):
        TYPE = "none"

        def shape(self):
            return None

        def predict(self, x):
            raise NotImplementedError

    out = {"cases": {}}
    with tempfile.TemporaryDirectory() as td:
        for case in ac.cases():
            labels = ac.labels(case["L"], case["fp_index"])
            mfile = os.path.join(td, "model.json")
            json.dump({"labels": labels, "hyperparams": {"square_width": case["square_width"]}, "type": "thermal",
                       "version": "golden"}, open(mfile, "w"))
            interp = NoNetwork(mfile)
            rows = []
            for probs, seg_frames in zip(case["probs"], case["frames"]):
                if len(probs) == 0:
                    rows.append(None)
                    continue
                tp = interp.track_prediction_from_raw(1, [list(f) for f in seg_frames], [p for p in probs],
                                                      [1] * len(probs))
                score = np.asarray(tp.class_best_score)
                assert score.dtype == np.float32, score.dtype
                rows.append([int(v) for v in score.view(np.uint32)])
            out["cases"][case["name"]] = rows
            print(case["name"], sum(r is not None for r in rows), "tracks")
    with open(os.path.join(HERE, "aggregate_crafted_golden.json"), "w") as fh:
        json.dump(out, fh)


POST_VARIANTS = ("no_diff_norm", "channels_swapped", "inceptionv3_scaling")


def postprocess_variant_runs():
    """ClipClassifier.post_process_file of the reference, <clip>.txt mode, as make_golden_postprocess.py runs it, but
    for models with diff_norm = False, swapped channels and the inceptionv3 input scaling: CRC32 per network input.
    -> postprocess_variants_golden.json"""
    import shutil

    from helpers import IdentityDraws

    interp_mod = rh.ref("ml_tools.interpreter")
    ccmod = rh.ref("classify.clipclassifier")
    te = rh.ref("track.trackextractor")
    rh.ref("config.config")
    cfgmod = rh.ref("config.classifyconfig")
    tools = rh.ref("ml_tools.tools")
    out = {}
    for name in ("possum", "hedgehog"):
        for variant in POST_VARIANTS:
            config = rh.default_config()
            config.tracking["thermal"].denoise = False
            with tempfile.TemporaryDirectory() as td:
                clip_file = os.path.join(td, name + ".cptv")
                shutil.copy(os.path.join(HERE, name + ".cptv"), clip_file)
                mfile = os.path.join(td, "model.json")
                params = dict({"frame_size": 32}, **cc.VARIANTS[variant])
                json.dump({"labels": LABELS, "hyperparams": params, "type": "thermal", "version": "golden"}, open(mfile, "w"))
                config.classify.models = [cfgmod.ModelConfig.load({"id": 7, "name": "wr-test", "model_file": mfile})]
                te.extract_file(clip_file, config, False)
                chunks, seg_log = [], {}

                class Capture(interp_mod.Interpreter):
                    TYPE = "capture"

                    def shape(self):
                        return 1, (None, 160, 160, 2)

                    def predict(self, x):
                        chunks.append(np.array(x, dtype=np.float32, copy=True))
                        return fake_predict(x)

                interp = Capture(mfile)
                interp.id, interp.port = 7, 8123
                orig = interp.frames_for_prediction

                def logged(clip, track, **args):
                    segs = orig(clip, track, **args)
                    seg_log[track.get_id()] = [[int(f) for f in s.frame_indices] for s in segs]
                    return segs

                interp.frames_for_prediction = logged
                classifier = ccmod.ClipClassifier(config)
                classifier.get_classifier = lambda model, location=None: interp
                with IdentityDraws():
                    classifier.post_process_file(clip_file, None)
                meta = tools.load_clip_metadata(os.path.join(td, name + ".txt"))
            x = np.concatenate(chunks)
            tracks, pos = [], 0
            for t in meta["tracks"]:   # chunks arrive track by track
                segs = seg_log.get(t["id"], [])
                tracks.append({"id": t["id"], "segments": segs, "crc": [crc(s) for s in x[pos:pos + len(segs)]]})
                pos += len(segs)
            assert pos == len(x)
            out["%s_%s" % (name, variant)] = {"hyperparams": params, "tracks": tracks}
            print(name, variant, [(t["id"], len(t["crc"])) for t in tracks])
    with open(os.path.join(HERE, "postprocess_variants_golden.json"), "w") as fh:
        json.dump(out, fh)


if __name__ == "__main__":
    which = sys.argv[1:] or ["classify", "aggregate", "postprocess"]
    if "classify" in which:
        classify_runs()
    if "aggregate" in which:
        aggregate_runs()
    if "postprocess" in which:
        postprocess_variant_runs()
