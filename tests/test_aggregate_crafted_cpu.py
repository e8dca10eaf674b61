"""The float32 statement of the track aggregation (tests/aggregate_crafted.py: expected) against what the REFERENCE's
TrackPrediction.classified_track + Interpreter.track_prediction_from_raw gave for the same crafted cases
(tests/golden/aggregate_crafted_golden.json, made by tests/golden/make_golden_classify_crafted.py): bit for bit.
The GPU test holds cpx_aggregate_predictions to that statement."""
import json
import os

import numpy as np
import pytest

import aggregate_crafted as ac
from helpers import GOLDEN

CASES = {c["name"]: c for c in ac.cases()}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "aggregate_crafted_golden.json")) as fh:
        return json.load(fh)["cases"]


def test_case_list_covers_what_it_claims():
    assert {c["L"] for c in CASES.values()} == set(ac.LABEL_COUNTS)
    assert {c["square_width"] for c in CASES.values()} == {1, 5} and {c["fp_index"] < 0 for c in CASES.values()} == {True, False}
    for c in CASES.values():
        n_seg = [len(p) for p in c["probs"]]
        assert len(n_seg) > 64 and n_seg[0] == 0 and n_seg[-1] == 0 and {0, 1, 2, 5} <= set(n_seg)
        if c["square_width"] == 5:
            distinct = {len(set(f[0])) for p, f in zip(c["probs"], c["frames"]) if len(p) == 1}
            assert {1, 6, 7} <= distinct
    # on the cap path, winners on and off the false-positive label
    c = CASES["L17"]
    scores, best = ac.expected(c)
    capped = [t for t, (p, f) in enumerate(zip(c["probs"], c["frames"])) if len(p) == 1 and len(set(f[0])) < 6.25]
    assert {bool(best[t] == c["fp_index"]) for t in capped} == {True, False}
    sums = scores[capped].astype(np.float64).sum(axis=1)
    assert np.any(np.abs(sums - 0.5) < 1e-6) and np.any(np.abs(sums - 1.0) < 1e-6)
    # the overflowing track: total 0, not above 0.5
    scores, _ = ac.expected(CASES["L8"])
    assert np.all(scores[-2] == 0) and len(CASES["L8"]["probs"][-2]) == 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_float32_statement_equals_reference_track_prediction(golden, name):
    scores, best = ac.expected(CASES[name])
    rows = golden[name]
    assert len(rows) == len(scores)
    n = 0
    for t, row in enumerate(rows):
        if row is None:   # the reference never aggregates a track without a segment
            assert len(CASES[name]["probs"][t]) == 0 and best[t] == -1 and not scores[t].any()
            continue
        want = np.array(row, np.uint32)
        assert np.array_equal(scores[t].view(np.uint32), want), (name, t, scores[t], want.view(np.float32))
        assert best[t] == int(np.argmax(want.view(np.float32)))
        n += 1
    assert n >= 50
