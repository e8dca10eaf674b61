"""Crafted cases for cpx_aggregate_predictions and their expectation, stated as explicit np.float32 operations in the
order the reference evaluates them (classify/trackprediction.py:121-171, ml_tools/interpreter.py:151-168) -- so the
expectation does not depend on the NumPy that happens to be installed.  tests/golden/make_golden_classify_crafted.py
runs the same cases through the reference's TrackPrediction (-> tests/golden/aggregate_crafted_golden.json);
tests/test_aggregate_crafted_cpu.py pins this statement to that, bit for bit; tests/test_aggregate_crafted_gpu.py
holds the kernel to this statement, bit for bit."""
import numpy as np

LABEL_COUNTS = (1, 2, 5, 7, 8, 9, 15, 16, 17, 33, 128)
N_TRACKS = 70                                  # more than the 64 tracks of one workgroup
SEGMENTS = (0, 1, 2, 5, 1, 1, 0, 1, 2, 1)      # per track, cycled; the first and the last track have none
DISTINCT = (1, 6, 7, 25)                       # distinct frames of a single segment: the cap applies below 25 / 4 = 6.25


def labels(L, fp_index):
    out = ["label%d" % i for i in range(L)]
    if fp_index >= 0:
        out[fp_index] = "false-positive"
    return out


def _segment_frames(rng, n_tiles, distinct):
    """n_tiles sorted frame numbers with exactly `distinct` different values."""
    distinct = min(distinct, n_tiles)
    values = np.sort(rng.choice(200, distinct, replace=False))
    idx = np.sort(np.concatenate([np.arange(distinct), rng.integers(0, distinct, n_tiles - distinct)]))
    return [int(v) for v in values[idx]]


def _launch(name, L, fp_index, square_width, seed, extra=()):
    rng = np.random.default_rng(seed)
    per = square_width * square_width
    probs, frames = [], []
    single = 0
    for t in range(N_TRACKS):
        s = 0 if t in (0, N_TRACKS - 1) else SEGMENTS[t % len(SEGMENTS)]
        p = (rng.random((s, L)) ** 3).astype(np.float32)          # skewed, like a network's confidences
        f = []
        for k in range(s):
            f.append(_segment_frames(rng, per, DISTINCT[(single + k) % len(DISTINCT)] if s == 1 else per))
        if s == 1:
            # every other capped-or-not situation with the winner ON the false-positive label (no cap then)
            if fp_index >= 0 and (single // len(DISTINCT)) % 2 == 1:
                p[0, fp_index] = np.float32(1.5)
            single += 1
        probs.append(p)
        frames.append(f)
    for p, f in extra:
        probs.insert(N_TRACKS - 1, np.asarray(p, np.float32).reshape(len(f), L))
        frames.insert(N_TRACKS - 1, f)
    return dict(name=name, L=L, fp_index=fp_index, square_width=square_width, probs=probs, frames=frames)


def cases():
    out = []
    for L in LABEL_COUNTS:
        extra = []
        if L == 8:
            # a label sum that overflows float32: every score is x / inf = 0, the total 0 is not above 0.5 -> no cap
            extra.append(([[3e38, 3e38, 1, 1, 1, 1, 1, 1]], [[5] * 25]))
        out.append(_launch("L%d" % L, L, min(1, L - 1), 5, 1000 + L, extra))
    out.append(_launch("L9_no_false_positive_label", 9, -1, 5, 2001))
    out.append(_launch("L17_fp_last", 17, 16, 5, 2002))
    # single-frame models: one tile per sample, one distinct frame, and 1 < 1 / 4 is false -> never capped
    out.append(_launch("L9_square_width_1", 9, 4, 1, 2003))
    return out


def f32_sum(v):
    """np.sum of a contiguous float32 vector of at most 128 elements, as NumPy's pairwise_sum evaluates it: a plain
    loop below 8 elements; else eight running sums over the blocks of 8, combined as ((0+1)+(2+3))+((4+5)+(6+7)),
    then the tail in order."""
    n = len(v)
    assert n <= 128
    if n < 8:
        total = np.float32(0.0)
        for x in v:
            total = np.float32(total + x)
        return total
    r = [np.float32(x) for x in v[:8]]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = np.float32(r[j] + v[i + j])
        i += 8
    total = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3]))
                       + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
    for x in v[i:]:
        total = np.float32(total + x)
    return total


def expected(case):
    """-> (scores float32 [n_tracks, L], best int32 [n_tracks]); a track without a segment scores 0 and has best -1."""
    L, sq, fp = case["L"], case["square_width"], case["fp_index"]
    n = len(case["probs"])
    scores, best = np.zeros((n, L), np.float32), np.full(n, -1, np.int32)
    with np.errstate(over="ignore"):
        for t, (p, f) in enumerate(zip(case["probs"], case["frames"])):
            if len(p) == 0:
                continue
            s = np.zeros(L, np.float32)
            for seg in p:                                   # np.sum(predictions, axis=0): segment by segment
                s = (s + seg).astype(np.float32)
            s = (s / f32_sum(s)).astype(np.float32)         # class_best_score / np.sum(class_best_score)
            b = int(np.argmax(s))
            if len(p) == 1 and len(set(f[0])) < sq ** 2 / 4 and b != fp:
                total = f32_sum(s)                          # cap_confidences(0.5)
                if total > 0.5:
                    s = (s * np.float32(np.float32(0.5) / total)).astype(np.float32)
            scores[t], best[t] = s, b
    return scores, best


def flatten(case):
    """-> (probs [n_samples, L], sample_track [n_samples], frames per sample [n_samples, square_width**2])."""
    L = case["L"]
    probs = np.concatenate([p.reshape(-1, L) for p in case["probs"]]).astype(np.float32)
    sample_track = np.array([t for t, p in enumerate(case["probs"]) for _ in range(len(p))], np.int32)
    frames = np.array([seg for f in case["frames"] for seg in f], np.int32).reshape(len(probs), -1)
    return probs, sample_track, frames
