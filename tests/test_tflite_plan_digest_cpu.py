"""build_plan hands the device the same plans as the planner the golden was written from (no GPU): the SHA-256 of every
plan of tests/tflite_plan_digest.py's corpus -- whole-network stand-ins and single-operator graphs, float32 and
quantised, crossed with the planner's options -- against tests/golden/tflite_plan_digests.json, and the text of every
refusal the corpus holds."""
import importlib.util
import json
import os

import pytest

import tflite_plan_digest as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "tflite_plan_digests.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def computed():
    return pd.compute()


@pytest.fixture(scope="module")
def refused_by_name():
    spec = importlib.util.spec_from_file_location("make_golden_plan_digests", os.path.join(GOLDEN, "make_golden_plan_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.REFUSED


def test_the_corpus_is_the_goldens(golden, computed):
    assert list(computed) == [key for key, _, _ in pd.entries()]
    assert set(computed) == set(golden), sorted(set(computed) ^ set(golden))


def test_every_plan_is_the_goldens(golden, computed):
    differ = [key for key in golden if computed.get(key) != golden[key]]
    assert not differ, "%d of %d plans differ from the golden's: %s" % (len(differ), len(golden), differ)


def test_refusals_are_the_named_ones(golden, refused_by_name):
    assert {key for key, v in golden.items() if "refused" in v} == set(refused_by_name)
    assert all(set(v) == {"refused"} or (set(v) == {"digest"} and len(v["digest"]) == 64) for v in golden.values())
    for name in pd.GRAPHS:
        assert any("digest" in v for key, v in golden.items() if key.split("|")[0] == name), name
