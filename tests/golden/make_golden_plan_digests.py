#!/usr/bin/env python3
"""The digest of every plan of tests/tflite_plan_digest.py's corpus -> tflite_plan_digests.json.  Host work: no GPU, no
reference.  The golden pins what build_plan hands to the device, so it is written from a planner that is trusted -- the
one before a change to cpx/ml_tools/tflite_graph.py -- and never refreshed from the code under test: an entry that would
have to be regenerated is a behaviour that changed.

    python tests/golden/make_golden_plan_digests.py [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in ("tests", "classifier-pipeline_amd"):
    sys.path.insert(0, os.path.join(REPO, p))
import tflite_plan_digest as pd  # noqa: E402

# the entries the planner refuses, and which refusal each pins; every other entry has to plan
REFUSED = {
    # input_mode on a graph that does not read three colour channels (the WR-ResNet reads two)
    "wrresnet|caffe",
    "wrresnet_q8|caffe",
    # grouped_convolutions=False: a grouped CONV_2D is refused by operator index and name, float32 and INT8 alike
    "wrresnet|ungrouped",
    "wrresnet_q8|ungrouped",
    # output= naming a CONCATENATION: its inputs would be second views of the graph's output
    "inception_v3|output_concatenation",
}


def main(path):
    out = pd.compute()
    refused = {k for k, v in out.items() if "refused" in v}
    assert refused == REFUSED, sorted(refused ^ REFUSED)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=False)
        fh.write("\n")
    print(len(out), "entries,", len({v["digest"] for v in out.values() if "digest" in v}), "distinct digests,",
          len(refused), "refusals ->", path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tflite_plan_digests.json"))
