#!/usr/bin/env python3
"""One step of the glancer's training walk as bits: one JSON object {"cus": the device's CU count, "cases": {case: {tensor: sha256}}} over
tests/glancer_walk_bits_cases.py -- the features, every parameter gradient and every running statistic after the step.  Two versions of
adafocus_amd/glancer_train.py that compute the same thing print the same "cases".  The recording of the walk before its layer treatment moved
into the core it shares with the trunk is tests/golden/glancer_walk_bits.json; it is not regenerated from later code.
Usage: python tools/glancer_walk_bits.py > bits.json"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests import glancer_walk_bits_cases as T  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    print(json.dumps(dict(cus=T.device_cus(dev), cases=T.digests(dev)), indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
