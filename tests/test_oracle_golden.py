"""The oracle restatement (oracle/track_oracle.py) against the vectors the
reference itself produced (tests/golden/make_golden.py) -- every frame of both
fixture clips, every stage, bit for bit; and against the reference's own golden
tests/clips/possum.txt."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, crc, load_clip, load_golden


def _run(name, dn):
    import track_oracle as to

    frames, t_on, ffc, bgf, hdr = load_clip(name)
    cfg = to.OracleConfig(hdr.model)
    cfg.denoise = bool(dn)
    return to.track_clip(frames, t_on, ffc, bgf, cfg, keep=True), frames


@pytest.mark.parametrize("name,dn", [("possum", 0), ("hedgehog", 0), ("possum", 1), ("synth35", 0)])
def test_oracle_matches_reference_vectors(name, dn):
    out, frames = _run(name, dn)
    z, gt = load_golden(name, dn)
    fr = out["frames"]
    assert len(fr) == int(z["n_frames"])
    assert np.array_equal(out["init_bg"].astype(np.int32), z["init_bg"])
    assert float(out["init_avg"]) == float(z["init_avg"])
    for i, f in enumerate(fr):
        assert f["ffc"] == bool(z["ffc"][i]), i
        assert f["bg_used_avg"] == z["bg_used_avg"][i], i
        assert f["bg_after_avg"] == z["bg_after_avg"][i], i
        assert f["threshold"] == z["threshold"][i], i
        assert crc(f["filtered"]) == z["crc_filtered"][i], i
        if dn == 0:
            assert crc(f["obj_u8"]) == z["crc_obj_u8"][i], i
        assert crc(f["mask"].astype(np.int32)) == z["crc_mask"][i], i
        assert crc(f["bg_after"]) == z["crc_bg_after"][i], i
        assert crc(f["weight_after"].astype(np.float64)) == z["crc_weight_after"][i], i
        a, b = z["comp_offsets"][i], z["comp_offsets"][i + 1]
        assert f["n_components"] == b - a, i
        assert np.array_equal(f["stats"], z["comp_stats"][a:b]), i
        assert np.array_equal(f["centroids"], z["comp_centroids"][a:b]), i
        a, b = z["region_offsets"][i], z["region_offsets"][i + 1]
        got = np.array(
            [
                (r.x, r.y, r.width, r.height, r.mass, r.id, float(r.pixel_variance), r.was_cropped,
                 r.is_along_border, float(r.centroid[0]), float(r.centroid[1]))
                for r in f["regions"]
            ],
            dtype=np.float64,
        ).reshape(-1, 11)
        assert np.array_equal(got, z["regions"][a:b]), i
    # final tracks
    assert len(out["tracks"]) == len(gt["tracks"])
    for t, g in zip(out["tracks"], gt["tracks"]):
        assert (t.id, t.start_frame, t.end_frame) == (g["id"], g["start_frame"], g["end_frame"])
        assert t.stats["score"] == g["score"]
        assert len(t.bounds) == len(g["positions"])
        for r, p in zip(t.bounds, g["positions"]):
            assert (r.x, r.y, r.width, r.height, int(r.mass), r.frame_number, r.blank) == (
                p["x"], p["y"], p["width"], p["height"], p["mass"], p["frame_number"], p["blank"])
            assert float(r.pixel_variance) == p["pixel_variance"]
    assert [(r, t.id) for r, t in out["filtered_tracks"]] == [(f["reason"], f["id"]) for f in gt["filtered"]]


def test_oracle_matches_possum_txt():
    """Default config (denoise on) vs the reference's committed golden metadata."""
    out, _ = _run("possum", 1)
    with open(os.path.join(GOLDEN, "possum.txt")) as fh:
        gold = json.load(fh)
    assert len(out["tracks"]) == len(gold["tracks"]) == 2
    for t, g in zip(out["tracks"], gold["tracks"]):
        assert t.id == g["id"]
        assert t.start_frame == g["frame_start"] and t.end_frame == g["frame_end"]
        assert len(t.bounds) == g["num_frames"]
        assert abs(t.stats["score"] - g["tracking_score"]) <= 1e-6 * g["tracking_score"]
        for r, p in zip(t.bounds, g["positions"]):
            assert (r.x, r.y, r.width, r.height, int(r.mass), r.frame_number, r.blank) == (
                p["x"], p["y"], p["width"], p["height"], p["mass"], p["frame_number"], p["blank"])
            assert abs(round(float(r.pixel_variance), 2) - p["pixel_variance"]) < 1e-3


@pytest.mark.parametrize("name,fs", [("possum", 32), ("hedgehog", 32), ("hedgehog", 64)])
def test_classify_oracle_matches_reference_inputs(name, fs):
    """oracle/classify_oracle.py against the network inputs the reference's own
    Interpreter.classify_track built (tests/golden/make_golden_classify.py)."""
    import classify_oracle as co

    out, frames = _run(name, 0)
    z = np.load(os.path.join(GOLDEN, "%s_classify_fs%d.npz" % (name, fs)))
    with open(os.path.join(GOLDEN, "%s_classify_fs%d.json" % (name, fs))) as fh:
        meta = json.load(fh)
    fr = out["frames"]
    proc_thermal = {f["index"]: None for f in fr}
    _, _, _, bgf, _ = load_clip(name)
    proc = [i for i in range(frames.shape[0]) if not bgf[i]]
    thermal_of = lambda q: frames[proc[q]]
    filtered_of = lambda q: fr[q]["filtered"].astype(np.float64)
    H, W = frames.shape[1:]
    crop = (1, 1, W - 2, H - 2)
    assert len(out["tracks"]) == len(meta["tracks"])
    for ti, (t, m) in enumerate(zip(out["tracks"], meta["tracks"])):
        assert t.id == m["track_id"]
        segs = z["t%d_segments" % ti]
        by_frame = {r.frame_number: r for r in t.bounds}
        x, info = co.preprocess_segments(thermal_of, filtered_of, by_frame, t.bounds, segs, fs, crop)
        want = z["t%d_input" % ti]
        assert x.shape == want.shape
        assert np.array_equal(x, want), (name, ti, np.abs(x - want).max())
        score = co.classified_track(z["t%d_pred" % ti], prediction_frames=segs, labels=meta["labels"])
        assert np.array_equal(score, np.array(m["class_best_score"]))


_CLIP_RUNS = {}


def _classify_clip(name):
    """The oracle's tracks and filtered frames of a fixture clip, once per session, as callables for classify_oracle."""
    if name not in _CLIP_RUNS:
        out, frames = _run(name, 0)
        _, _, _, bgf, _ = load_clip(name)
        proc = [i for i in range(frames.shape[0]) if not bgf[i]]
        fr = out["frames"]
        _CLIP_RUNS[name] = (out, lambda q: frames[proc[q]], lambda q: fr[q]["filtered"].astype(np.float64),
                            (1, 1, frames.shape[2] - 2, frames.shape[1] - 2))
    return _CLIP_RUNS[name]


def oracle_kwargs(hyperparams):
    """Model hyper-parameters (the sidecar's "hyperparams") -> the variant arguments of classify_oracle."""
    return dict(diff_norm=hyperparams.get("diff_norm", True), thermal_diff_norm=hyperparams.get("thermal_diff_norm", False),
                channels=tuple(hyperparams.get("channels", ["thermal", "filtered"])),
                tf_scaling=hyperparams.get("model_name", "wr-resnet") == "inceptionv3")


VARIANTS = ["thermal_diff_norm", "no_diff_norm", "thermal_diff_norm_no_diff_norm", "channels_swapped", "single_frame",
            "single_frame_thermal_diff_norm", "inceptionv3_scaling", "inceptionv3_scaling_single_frame"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["hedgehog", "possum"])
def test_classify_oracle_variants_match_reference_inputs(name, variant):
    """Every model variant of oracle/classify_oracle.py (thermal limits, per-tile normalise, channel order, the
    single-frame path, both input scalings) against the CRC32 of what the reference's own Interpreter built
    (tests/golden/make_golden_classify_variants.py), sample by sample."""
    import classify_oracle as co

    with open(os.path.join(GOLDEN, "classify_variants_golden.json")) as fh:
        g = json.load(fh)["variants"][variant]
    hp = g["hyperparams"]
    out, thermal_of, filtered_of, crop = _classify_clip(name)
    assert len(out["tracks"]) == len(g[name])
    for t, want in zip(out["tracks"], g[name]):
        assert t.id == want["track_id"]
        if hp.get("square_width", 5) == 1:
            samples = [r for r in t.bounds if not r.blank and r.width > 0 and r.height > 0]
            assert [r.frame_number for r in samples] == want["segments"]
            x, _ = co.preprocess_frames(thermal_of, filtered_of, t.bounds, samples, hp["frame_size"], crop,
                                        **oracle_kwargs(hp))
        else:
            by_frame = {r.frame_number: r for r in t.bounds}
            x, _ = co.preprocess_segments(thermal_of, filtered_of, by_frame, t.bounds, want["segments"], hp["frame_size"],
                                          crop, **oracle_kwargs(hp))
        assert list(x.shape) == want["shape"] and x.dtype == np.float32
        assert [crc(s) for s in x] == want["crc"], (name, variant, t.id)


@pytest.mark.parametrize("name", ["possum", "hedgehog"])
def test_classify_oracle_post_process_matches_reference_inputs(name):
    """classify_oracle.preprocess_segments(post_process=True) against the network inputs of the reference's
    ClipClassifier.post_process_file in its <clip>.txt mode (tests/golden/make_golden_postprocess.py), bit for bit.
    That mode re-reads the file with a fresh background model which, unlike the tracking walk, stands still on
    FFC-affected frames; neither fixture clip has one, so the filtered frames of the oracle's tracking walk are the
    second walk's."""
    import classify_oracle as co

    with open(os.path.join(GOLDEN, "postprocess_golden.json")) as fh:
        gold = json.load(fh)["runs"][name + "_meta"]
    z = np.load(os.path.join(GOLDEN, "postprocess_golden.npz"))
    out, thermal_of, filtered_of, crop = _classify_clip(name)
    assert out["ffc_frames"] == []
    n = 0
    for g in gold["tracks"]:
        if not g["segments"]:
            continue
        by_frame = {p[4]: Rect(*p) for p in g["positions"]}
        x, _ = co.preprocess_segments(thermal_of, filtered_of, by_frame, None, g["segments"], 32, crop, post_process=True)
        want = z["%s_meta_t%d_input" % (name, g["id"])]
        assert x.shape == want.shape
        assert np.array_equal(x, want), (name, g["id"], float(np.abs(x - want).max()))
        n += len(x)
    assert n >= 1


@pytest.mark.parametrize("variant", ["no_diff_norm", "channels_swapped", "inceptionv3_scaling"])
@pytest.mark.parametrize("name", ["possum", "hedgehog"])
def test_classify_oracle_post_process_variants_match_reference_inputs(name, variant):
    """The post-process path combined with diff_norm = False (Frame.normalize on a float64 filtered crop), swapped
    channels and the input scaling, against the CRC32 of what the reference's post_process_file fed its model
    (tests/golden/postprocess_variants_golden.json, <clip>.txt mode)."""
    import classify_oracle as co

    with open(os.path.join(GOLDEN, "postprocess_variants_golden.json")) as fh:
        gold = json.load(fh)["%s_%s" % (name, variant)]
    with open(os.path.join(GOLDEN, "postprocess_golden.json")) as fh:
        positions = {t["id"]: t["positions"] for t in json.load(fh)["runs"][name + "_meta"]["tracks"]}
    out, thermal_of, filtered_of, crop = _classify_clip(name)
    assert out["ffc_frames"] == []
    n = 0
    for g in gold["tracks"]:
        if not g["segments"]:
            continue
        by_frame = {p[4]: Rect(*p) for p in positions[g["id"]]}
        x, _ = co.preprocess_segments(thermal_of, filtered_of, by_frame, None, g["segments"], 32, crop, post_process=True,
                                      **dict(oracle_kwargs(gold["hyperparams"]), thermal_diff_norm=False))
        assert [crc(s) for s in x] == g["crc"], (name, variant, g["id"])
        n += len(x)
    assert n >= 1


_CRAFTED = {}


def _crafted():
    """The crafted clip (tests/classify_crafted.py) through the oracle's pixel stage, once per session."""
    import classify_crafted as cc
    import track_oracle as to

    if not _CRAFTED:
        with open(os.path.join(GOLDEN, "classify_crafted_golden.json")) as fh:
            _CRAFTED["gold"] = json.load(fh)
        frames = cc.clip_frames()
        out = to.track_clip(frames, cc.TIME_ON, cc.LAST_FFC, None, to.OracleConfig("lepton3"), keep=True, do_tracking=False)
        _CRAFTED["frames"] = frames
        _CRAFTED["filtered"] = np.stack([f["filtered"] for f in out["frames"]]).astype(np.int32)
    return _CRAFTED["gold"], _CRAFTED["frames"], _CRAFTED["filtered"]


def test_crafted_clip_and_cases_are_the_golden_ones():
    """The seeded clip, the oracle's filtered frames of it and the case list are what the reference was run on; the
    case list still hits every geometry class at every frame size."""
    import classify_crafted as cc

    gold, frames, filtered = _crafted()
    assert crc(frames) == gold["frames_crc"] and crc(filtered) == gold["filtered_crc"]
    tracks = cc.tracks()
    assert [(t["name"], [list(r.as_tuple()) for r in t["regions"]], t["segments"]) for t in tracks] == [
        (t["name"], t["regions"], t["segments"]) for t in gold["tracks"]]
    for fs in cc.FRAME_SIZES:
        cc.coverage(fs, tracks)
    assert {cc.run_key(v, fs) for v, fs in cc.RUNS} == set(gold["runs"])
    for t in tracks:
        assert cc.clip_at_zero_expected(frames, t) == gold["clip_at_zero"][t["name"]]
    assert gold["clip_at_zero"]["clip_on"] and not gold["clip_at_zero"]["clip_off"]


def crafted_oracle_inputs(variant, fs, frames, filtered, track):
    """classify_oracle on one crafted track -> (network inputs float32, info)."""
    import classify_crafted as cc
    import classify_oracle as co

    hp = dict({"frame_size": fs}, **cc.VARIANTS[variant])
    thermal_of, filtered_of = (lambda q: frames[q]), (lambda q: filtered[q].astype(np.float64))
    if hp.get("square_width", 5) == 1:
        return co.preprocess_frames(thermal_of, filtered_of, track["regions"], cc.usable(track["regions"]), fs, cc.CROP,
                                    **oracle_kwargs(hp))
    by_frame = {r.frame_number: r for r in track["regions"]}
    return co.preprocess_segments(thermal_of, filtered_of, by_frame, track["regions"], track["segments"], fs, cc.CROP,
                                  **oracle_kwargs(hp))


def _crafted_runs():
    import classify_crafted as cc

    return cc.RUNS


@pytest.mark.parametrize("variant,fs", _crafted_runs())
def test_classify_oracle_matches_reference_on_crafted_tracks(variant, fs):
    """oracle/classify_oracle.py, every variant and frame size, against the CRC32 of what the reference's Interpreter
    built for the crafted tracks (tests/golden/make_golden_classify_crafted.py)."""
    import classify_crafted as cc

    gold, frames, filtered = _crafted()
    run = gold["runs"][cc.run_key(variant, fs)]
    for t, want in zip(cc.tracks(), run["tracks"]):
        x, info = crafted_oracle_inputs(variant, fs, frames, filtered, t)
        got = [crc(s) for s in x]
        bad = [i for i, (a, b) in enumerate(zip(got, want["crc"])) if a != b]
        assert len(got) == len(want["crc"]) and not bad, (
            t["name"], bad[:5], [(float(x[i].min()), float(x[i].max()), float(x[i].astype(np.float64).mean()),
                                  want["min"][i], want["max"][i], want["mean"][i]) for i in bad[:1]])
        if "square_width" not in cc.VARIANTS[variant]:
            assert info["clip_at_zero"] == gold["clip_at_zero"][t["name"]]


class Rect:
    def __init__(self, x, y, width, height, frame_number, blank=False):
        self.x, self.y, self.width, self.height, self.frame_number, self.blank = x, y, width, height, frame_number, blank


@pytest.mark.parametrize("name,dn", [("possum", 0), ("hedgehog", 0), ("possum", 1)])
def test_thumbnail_oracle_matches_reference(name, dn):
    """oracle/thumbnail_oracle.py (+ the findContours / TC89_L1 restatement in cv2_shim) against the
    per-frame thumbnail statistics the reference produced, and for the default config against the
    thumbnail entries of the reference's own golden possum.txt."""
    import thumbnail_oracle as th

    out, frames = _run(name, dn)
    fr = out["frames"]
    with open(os.path.join(GOLDEN, "%s_dn%d_thumbs.json" % (name, dn))) as fh:
        gold = json.load(fh)
    _, t_on, ffc, bgf, hdr = load_clip(name)
    proc = [i for i in range(frames.shape[0]) if not bgf[i]]
    assert len(out["tracks"]) == len(gold["tracks"])
    for t, g in zip(out["tracks"], gold["tracks"]):
        stats, max_mass, max_md, min_md, max_contour = th.track_thumb_stats(
            t.bounds, lambda q: fr[q]["mask"], lambda q: frames[proc[q]])
        assert [[s.region.frame_number, s.contours, float(s.median_diff)] for s in stats] == g["stats"]
        assert (max_mass, max_md, min_md, max_contour) == (
            g["max_mass"], g["max_median_diff"], g["min_median_diff"], g["max_contour"])
        best, score = th.thumbnail_info(t.bounds, lambda q: fr[q]["mask"], lambda q: frames[proc[q]])
        gb = g["best"]
        assert best.region.frame_number == gb["region"]["frame_number"]
        assert (best.contours, float(best.median_diff), score) == (gb["contours"], gb["median_diff"], gb["score"])
    if (name, dn) == ("possum", 1):
        with open(os.path.join(GOLDEN, "possum.txt")) as fh:
            ref_gold = json.load(fh)
        for t, g in zip(out["tracks"], ref_gold["tracks"]):
            best, score = th.thumbnail_info(t.bounds, lambda q: fr[q]["mask"], lambda q: frames[proc[q]])
            gt = g["thumbnail"]
            r = best.region
            assert (r.x, r.y, r.width, r.height, int(r.mass), r.frame_number) == tuple(
                gt["region"][k] for k in ("x", "y", "width", "height", "mass", "frame_number"))
            assert (best.contours, float(best.median_diff), round(score)) == (
                gt["contours"], gt["median_diff"], gt["score"])


@pytest.mark.parametrize("name,n", [("possum", 30), ("hedgehog", 8)])
def test_trackless_thumbnail_oracle_matches_reference(name, n):
    import thumbnail_oracle as th
    import track_oracle as to

    frames, t_on, ffc, bgf, hdr = load_clip(name)
    with open(os.path.join(GOLDEN, "%s_trackless_thumbs.json" % name)) as fh:
        gold = json.load(fh)
    frames, t_on, ffc, bgf = frames[:n], t_on[:n], ffc[:n], bgf[:n]
    out = to.track_clip(frames, t_on, ffc, bgf, to.OracleConfig(hdr.model), keep=True)
    assert len(out["tracks"]) == 0 and sum(len(r) for r in out["region_history"]) == gold["n_region_history"]
    proc = [i for i in range(n) if not bgf[i]]
    means = [frames[i].mean() for i in proc]
    x, y, w, h, fn, centroid, mass = th.trackless_thumb(out["region_history"], means, lambda q: frames[proc[q]],
                                                        frames[0])
    g = gold["trackless"]
    assert (x, y, w, h, fn, mass) == (g["x"], g["y"], g["width"], g["height"], g["frame_number"], g["mass"])
    assert [float(centroid[0]), float(centroid[1])] == g["centroid"]


def _busy_golden():
    z = np.load(os.path.join(GOLDEN, "busy_tracks.npz"))
    return z["seeds"], z["rows"], z["offsets"], int(z["frames"])


def busy_clip(seed, T):
    from cpx import synth

    return synth.make_clip(np.random.default_rng(1000 + int(seed)), T, max_blobs=8)


def test_oracle_matches_reference_on_busy_scenes():
    """Association / Kalman / blank regions beyond the fixture clips: every track the reference created on 11 seeded
    busy scenes (tests/golden/make_golden_busy.py), bounds and the Python-int typing of widths / heights included."""
    import track_oracle as to

    seeds, rows, offsets, T = _busy_golden()
    t_on, ffc = [100000 + 111 * i for i in range(T)], [40000] * T
    n_py = 0
    for k, seed in enumerate(seeds):
        out = to.track_clip(busy_clip(seed, T), t_on, ffc, None, to.OracleConfig("lepton3"), keep=True)
        mine = sorted(list(out["tracks"]) + [t for _, t in out["filtered_tracks"]], key=lambda t: t.id)
        got = [(t.id, r.x, r.y, r.width, r.height, int(r.mass), r.frame_number, int(bool(r.blank)), int(r.py[2]),
                int(r.py[3])) for t in mine for r in t.bounds]
        want = rows[offsets[k]:offsets[k + 1]]
        assert np.array_equal(np.asarray(got, np.int32), want), seed
        n_py += int((want[:, 8] | want[:, 9]).sum())
    assert n_py > 10


def _busy_classify_cases():
    """(clip frames, oracle output, [(oracle track, golden track entry)]) per clip of busy_classify_fs32.json; tracks
    are paired by birth (start frame + first box): the reference numbers same-frame births in set order (F14)."""
    import track_oracle as to

    with open(os.path.join(GOLDEN, "busy_classify_fs32.json")) as fh:
        gold = json.load(fh)
    T = gold["frames"]
    t_on, ffc = [100000 + 111 * i for i in range(T)], [40000] * T
    cases = []
    for c in gold["clips"]:
        frames = busy_clip(c["seed"], T)
        out = to.track_clip(frames, t_on, ffc, None, to.OracleConfig("lepton3"), keep=True)
        births = {(t.start_frame, t.bounds[0].x, t.bounds[0].y, t.bounds[0].width, t.bounds[0].height): t
                  for t in out["tracks"]}
        pairs = []
        for g in c["tracks"]:
            t = births.get((g["start_frame"],) + tuple(g["first"]))
            assert t is not None, (c["seed"], g["id"])
            pairs.append((t, g))
        assert len(pairs) == len(out["tracks"])
        cases.append((frames, out, pairs))
    return cases


def test_classify_oracle_matches_reference_on_busy_scenes():
    """Network inputs for 19 tracks of two busy synthetic scenes (many regions on the frame border: the edge-anchored
    branches of resize_and_pad) against the CRCs of what the reference's Interpreter.classify_track fed its model."""
    import classify_oracle as co

    n_samples = n_edge = 0
    for frames, out, pairs in _busy_classify_cases():
        fr = out["frames"]
        for t, g in pairs:
            by_frame = {r.frame_number: r for r in t.bounds}
            segs = [np.array(s) for s in g["segments"]]
            x, _ = co.preprocess_segments(lambda q: frames[q], lambda q: fr[q]["filtered"].astype(np.float64),
                                          by_frame, t.bounds, segs, 32, (1, 1, 158, 118))
            assert [crc(x[i]) for i in range(x.shape[0])] == g["crc"], g["id"]
            n_samples += x.shape[0]
            n_edge += g["edge_regions"]
    assert n_samples >= 30 and n_edge > 100


def test_thumbnail_oracle_matches_reference_on_busy_scenes():
    """Per-frame contour counts / median differences and the chosen thumbnail for the ~20 tracks of two busy synthetic
    scenes (tests/golden/busy_thumbs.json: reference run, make_golden_thumbs.py --busy): ~700 more contours for the
    findContours + TC89_L1 restatement than the fixture clips hold."""
    import thumbnail_oracle as th
    import track_oracle as to

    with open(os.path.join(GOLDEN, "busy_thumbs.json")) as fh:
        gold = json.load(fh)
    T = gold["frames"]
    t_on, ffc = [100000 + 111 * i for i in range(T)], [40000] * T
    n = 0
    for c in gold["clips"]:
        frames = busy_clip(c["seed"], T)
        out = to.track_clip(frames, t_on, ffc, None, to.OracleConfig("lepton3"), keep=True)
        fr = out["frames"]
        births = {(t.start_frame, t.bounds[0].x, t.bounds[0].y, t.bounds[0].width, t.bounds[0].height): t
                  for t in out["tracks"]}
        assert len(c["tracks"]) == len(out["tracks"])
        for g in c["tracks"]:
            t = births[(g["start_frame"],) + tuple(g["first"])]
            stats, max_mass, max_md, min_md, max_contour = th.track_thumb_stats(
                t.bounds, lambda q: fr[q]["mask"], lambda q: frames[q])
            assert [[s.region.frame_number, s.contours, float(s.median_diff)] for s in stats] == g["stats"], g["id"]
            best, score = th.thumbnail_info(t.bounds, lambda q: fr[q]["mask"], lambda q: frames[q])
            gb = g["best"]
            assert (best.region.frame_number, best.contours, float(best.median_diff), score) == (
                gb["region"]["frame_number"], gb["contours"], gb["median_diff"], gb["score"])
            n += len(stats)
    assert n > 500


def test_oracle_track_scores_and_rejects_on_busy_scenes():
    """End-of-clip statistics, score order and reject reasons of the busy scenes against the reference
    (tests/golden/busy_tracks_info.json)."""
    import track_oracle as to

    with open(os.path.join(GOLDEN, "busy_tracks_info.json")) as fh:
        info = json.load(fh)
    _, _, _, T = _busy_golden()
    t_on, ffc = [100000 + 111 * i for i in range(T)], [40000] * T
    n_rej = 0
    for c in info:
        out = to.track_clip(busy_clip(c["seed"], T), t_on, ffc, None, to.OracleConfig("lepton3"), keep=True)
        got = [[t.id, t.stats["score"], t.stats["frames_moved"], t.stats["max_offset"], t.stats["average_mass"],
                t.stats["delta_std"]] for t in out["tracks"]]
        assert len(got) == len(c["kept"])
        for g, w in zip(got, c["kept"]):
            assert g[0] == w[0] and g[2] == w[2], c["seed"]
            assert g[1] == pytest.approx(w[1], rel=1e-12) and g[3] == pytest.approx(w[3], rel=1e-12)
            assert g[4] == pytest.approx(w[4], rel=1e-12) and g[5] == pytest.approx(w[5], rel=1e-6)
        assert [[r, t.id] for r, t in out["filtered_tracks"]] == c["filtered"], c["seed"]
        n_rej += len(c["filtered"])
    assert n_rej > 0
