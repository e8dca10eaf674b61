"""TEST INFRASTRUCTURE ONLY -- CPU restatement (NumPy) of the reference's
classification pre-processing and prediction aggregation; the checker for the
HIP crop/tile kernel.  Every branch is pinned, bit for bit, by fixtures the
reference itself produced (tests/test_oracle_golden.py):
  default model                       *_classify_fs*.npz (make_golden_classify.py), busy_classify_fs32.json,
                                      classify_crafted_golden.json (frame sizes 32, 48, 64, 96, 128)
  thermal_diff_norm, diff_norm=False, classify_variants_golden.json (make_golden_classify_variants.py, fs 32) and
  both, channel order, input scaling, classify_crafted_golden.json (make_golden_classify_crafted.py, fs 32 and 64;
  single frames (preprocess_frames)   single frames also 96 and 128)
  post_process=True                   postprocess_golden.npz (make_golden_postprocess.py, <clip>.txt mode)
  post_process with diff_norm=False,  postprocess_variants_golden.json (make_golden_classify_crafted.py)
  swapped channels, input scaling
  constant tiles (max == min)         the 1 x 1 / 1 x 7 / 7 x 1 regions of classify_crafted_golden.json
  classified_track                    the class_best_score of the classify goldens
A branch without such a fixture must not serve as the expectation of a GPU test.

Follows (paths relative to /root/reference/src):
  ml_tools/interpreter.py:255-313   preprocess_frames (single-frame models)
  ml_tools/interpreter.py:315-363   get_limits
  ml_tools/interpreter.py:365-474   preprocess_segments
  ml_tools/preprocess.py:56-113     preprocess_frame
  ml_tools/preprocess.py:119-144    preprocess_single_frame
  ml_tools/imageprocessing.py:11-82 resize_and_pad / resize_cv
  ml_tools/preprocess.py:151-202    preprocess_movement (+ imageprocessing.py:85-104 square_clip)
  ml_tools/frame.py:187-191         Frame.normalize
  classify/clipclassifier.py:465-552 post_process_file's crops, limits and preprocess_frame call
  classify/trackprediction.py:127-171 classified_track
cv2.resize is oracle/cv2_shim.py:resize (not pinned by any reference golden: the goldens above were made
with the reference running on the same shim).
"""

import numpy as np

import cv2_shim as cv


def get_limits(regions, filtered_of):
    """min / max of region.subimage(frame.filtered) over the track's non-blank regions
    (max starts at 0) -- interpreter.py:315-363 with diff_norm=True, thermal_diff_norm=False.
    get_limits first calls Frame.float_arrays() (frame.py:316-324), which turns the stored
    filtered frames into float32 IN PLACE: the limits are float32 scalars and everything
    downstream of it (crop, resize, normalise) is float32 arithmetic."""
    min_diff, max_diff = None, 0
    for r in reversed(regions):
        if r.blank or r.width <= 0 or r.height <= 0:
            continue
        f = filtered_of(r.frame_number)
        if f is None:
            continue
        sub = np.float32(f[r.y : r.y + r.height, r.x : r.x + r.width])
        new_max, new_min = np.amax(sub), np.amin(sub)
        if min_diff is None or new_min < min_diff:
            min_diff = new_min
        if new_max > max_diff:
            max_diff = new_max
    return min_diff, max_diff


def resize_and_pad(frame, fs, region, crop, pad=None, interpolation=cv.INTER_LINEAR):
    """imageprocessing.py:11-70 with keep_edge=True, edge_offset=(0,0,0,0)."""
    scale = (np.array((fs, fs)) / np.array(frame.shape[:2])).min()
    width = min(max(round(frame.shape[1] * scale), 1), fs)
    height = min(max(round(frame.shape[0] * scale), 1), fs)
    if pad is None:
        pad = np.min(frame)
    out = np.full((fs, fs), pad, dtype=frame.dtype)
    small = cv.resize(np.float32(frame), (width, height), interpolation=interpolation)
    fh, fw = small.shape[:2]
    ox = (fs - fw) // 2
    oy = (fs - fh) // 2
    cx, cy, cw, ch = crop
    if region.x <= cx:
        ox = min(0, fs - fw)
    elif region.x + region.width >= cx + cw:
        ox = max((fs - 0) - fw, 0)
    if region.y <= cy:
        oy = min(0, fs - fh)
    elif region.y + region.height >= cy + ch:
        oy = max(fs - fh - 0, 0)
    out[oy : oy + fh, ox : ox + fw] = small
    return out


def normalize(data, mn=None, mx=None, new_max=1):
    """imageprocessing.py:151-169."""
    if data.size == 0:
        return np.zeros(data.shape)
    if mx is None:
        mx = np.amax(data)
    if mn is None:
        mn = np.amin(data)
    if mx == mn:
        if mx == 0:
            return np.zeros(data.shape)
        return data / mx
    return new_max * (np.float32(data) - mn) / (mx - mn)


def get_thermal_limits(regions, thermal_of):
    """thermal_norm_limits of get_limits (interpreter.py:338-345, thermal_diff_norm=True): min / max of
    float32(thermal) - np.median(float32 thermal) over the WHOLE frame of every usable region, both starting at None."""
    lo = hi = None
    for r in reversed(regions):
        if r.blank or r.width <= 0 or r.height <= 0:
            continue
        th = thermal_of(r.frame_number)
        if th is None:
            continue
        th = np.float32(th)
        diff = th - np.median(th)
        new_max, new_min = np.amax(diff), np.amin(diff)
        if lo is None or new_min < lo:
            lo = new_min
        if hi is None or new_max > hi:
            hi = new_max
    return lo, hi


def post_process_limits(regions_by_frame, filtered_of):
    """The limits of ClipClassifier.post_process_file (clipclassifier.py:476-500): over the SAMPLED regions only, in
    frame order, both started by the first crop (the max is not floored at 0); np.min / np.max of the float64 crop
    thermal - background, so the limits are np.float64 scalars."""
    limits = None
    for fn in sorted(regions_by_frame):
        r = regions_by_frame[fn]
        sub = np.asarray(filtered_of(fn)[r.y : r.y + r.height, r.x : r.x + r.width], dtype=np.float64)
        f_min, f_max = np.min(sub), np.max(sub)
        if limits is None:
            limits = [f_min, f_max]
        else:
            if f_min < limits[0]:
                limits[0] = f_min
            if f_max > limits[1]:
                limits[1] = f_max
    return limits


def preprocess_frame(thermal, filtered, region, fs, crop, median, limits, clip_at_zero, thermal_limits=None,
                     sub_median=True):
    """preprocess.py:56-113 for the classify calls (calculate_filtered=False) -> (thermal [fs,fs], filtered [fs,fs]),
    each float32 or -- where NumPy makes it so -- float64: normalize()'s np.zeros for a constant-zero tile, and the
    filtered channel under float64 limits (post_process_file).
      limits          filtered_norm_limits, or None (diff_norm=False and post_process_file without diff_norm):
                      Frame.normalize() then normalises BOTH channels over the tile itself (frame.py:187-191)
      thermal_limits  thermal_norm_limits (thermal_diff_norm=True): no clip at zero (preprocess.py:92); used for the
                      thermal normalise only when `limits` is given too (preprocess.py:95-109)
      sub_median      False for post_process_file, which subtracts the frame median from the crop BEFORE the resize
                      (clipclassifier.py:480-486) and passes cropped=True, sub_median=False."""
    t = np.float32(thermal[region.y : region.y + region.height, region.x : region.x + region.width])
    f = filtered[region.y : region.y + region.height, region.x : region.x + region.width]
    if sub_median:
        f = np.float32(f)
    else:
        t -= median
        f = np.asarray(f, dtype=np.float64)  # (np.float64(a 1 x 1 array) would be a scalar)
    t = resize_and_pad(t, fs, region, crop)
    f = resize_and_pad(f, fs, region, crop, pad=0)
    if sub_median:
        t -= median
    if thermal_limits is None and clip_at_zero:
        np.clip(t, 0, None, out=t)
    if limits is not None:
        f = normalize(f, mn=limits[0], mx=limits[1], new_max=255)
        if thermal_limits is not None:
            t = normalize(t, mn=thermal_limits[0], mx=thermal_limits[1], new_max=255)
        else:
            t = normalize(t, new_max=255)
    else:
        t = normalize(t, new_max=255)
        f = normalize(f, new_max=255)
    return t, f


def inc3_preprocess(x):
    """interpreter.py:563-566, in the dtype of x."""
    x /= 127.5
    x -= 1.0
    return x


def _model_limits(track_regions, filtered_of, thermal_of, diff_norm, thermal_diff_norm):
    """get_limits as preprocess_segments / preprocess_frames call it (interpreter.py:268-269,403-406)."""
    limits = thermal_limits = None
    if diff_norm or thermal_diff_norm:
        if diff_norm:
            limits = get_limits(track_regions, filtered_of)
        if thermal_diff_norm:
            thermal_limits = get_thermal_limits(track_regions, thermal_of)
    return limits, thermal_limits


def preprocess_segments(thermal_of, filtered_of, regions_by_frame, track_regions, segments, fs, crop, square_width=5,
                        diff_norm=True, thermal_diff_norm=False, channels=("thermal", "filtered"), tf_scaling=False,
                        post_process=False):
    """interpreter.py:365-474 + preprocess.py:151-202 (square_clip: imageprocessing.py:85-104).  segments: list of
    square_width**2 frame numbers each.  filtered frames are float32 after Frame.float_arrays().
    post_process=True is ClipClassifier.post_process_file's preparation of the same segments instead
    (clipclassifier.py:465-552): limits over the sampled crops, median first, always clipped at zero, no thermal
    limits ever (:465)."""
    medians, unique = {}, {}
    clip_at_zero = True
    for seg in segments:
        for fn in seg:
            fn = int(fn)
            if fn in unique:
                continue
            r = regions_by_frame[fn]
            unique[fn] = r
            th = thermal_of(fn)
            medians[fn] = np.median(th)
            if clip_at_zero and not post_process:
                sub = np.float32(th[r.y : r.y + r.height, r.x : r.x + r.width]) - medians[fn]
                if np.median(sub) <= 0:
                    clip_at_zero = False
    if post_process:
        limits = post_process_limits(unique, filtered_of) if diff_norm else None
        thermal_limits = None
    else:
        limits, thermal_limits = _model_limits(track_regions, filtered_of, thermal_of, diff_norm, thermal_diff_norm)
    data = {}
    for fn, r in unique.items():
        data[fn] = preprocess_frame(thermal_of(fn), filtered_of(fn), r, fs, crop, medians[fn], limits, clip_at_zero,
                                    thermal_limits=thermal_limits, sub_median=not post_process)
    sq = square_width
    out = np.zeros((len(segments), sq * fs, sq * fs, 2), dtype=np.float64)
    order = [("thermal", "filtered").index(c) for c in channels]
    for s, seg in enumerate(segments):
        assert len(seg) == sq * sq, "parity runs use full segments (short ones are padded at random, F13)"
        for i, fn in enumerate(seg):
            ty, tx = divmod(i, sq)
            tile = data[int(fn)]
            for c, src in enumerate(order):
                out[s, ty * fs : (ty + 1) * fs, tx * fs : (tx + 1) * fs, c] = np.float32(tile[src])
    if tf_scaling:
        out = inc3_preprocess(out)  # on the float64 tiled array, cast after (preprocess.py:200-202)
    info = dict(medians=medians, limits=limits, thermal_limits=thermal_limits, clip_at_zero=clip_at_zero)
    return np.float32(out), info


def preprocess_frames(thermal_of, filtered_of, track_regions, samples, fs, crop, diff_norm=True,
                      thermal_diff_norm=False, channels=("thermal", "filtered"), tf_scaling=False):
    """Single-frame models: interpreter.py:255-313 + preprocess.py:119-144.  samples: the regions to classify
    (frames_for_prediction with frames_per_classify = 1: every usable region of the track).  preprocess_frame runs with
    its defaults median=None, clip_thermals_at_zero=True; the sample is np.stack of its channels -- float32, unless
    normalize() returned np.zeros for a constant-zero tile, which makes the stack float64 -- and the input scaling
    runs in that dtype."""
    limits, thermal_limits = _model_limits(track_regions, filtered_of, thermal_of, diff_norm, thermal_diff_norm)
    order = [("thermal", "filtered").index(c) for c in channels]
    out = []
    for r in samples:
        th = thermal_of(r.frame_number)
        tile = preprocess_frame(th, filtered_of(r.frame_number), r, fs, crop, np.median(th), limits, True,
                                thermal_limits=thermal_limits)
        image = np.stack([tile[src] for src in order], axis=2)
        if tf_scaling:
            image = inc3_preprocess(image)
        out.append(image)
    info = dict(limits=limits, thermal_limits=thermal_limits, clip_at_zero=True)
    return np.float32(np.array(out)), info


def classified_track(predictions, smooth_masses=None, prediction_frames=None, labels=None, square_width=5):
    """class_best_score of a track from its segment predictions: trackprediction.py:127-171 plus the
    low-evidence cap of Interpreter.track_prediction_from_raw (interpreter.py:151-168): a single segment
    with fewer than square_width**2 / 4 distinct frames that is not 'false-positive' is capped at 0.5."""
    predictions = np.asarray(predictions)
    if smooth_masses is not None:
        masses = np.array(smooth_masses)
        smoothed = predictions * masses[:, None]
        score = np.sum(smoothed, axis=0) / np.sum(masses)
    else:
        score = np.sum(predictions, axis=0)
        score = score / np.sum(score)
    if prediction_frames is not None and len(prediction_frames) == 1 and \
            len(set(int(f) for f in prediction_frames[0])) < square_width**2 / 4:
        if labels is None or labels[int(np.argmax(score))] != "false-positive":
            total = np.sum(score)
            if total > 0.5:
                score = score * (0.5 / total)
    return score
