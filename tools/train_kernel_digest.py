#!/usr/bin/env python3
"""The training kernels' outputs as bits: one JSON line {"cus": the device's CU count, "cases": {case: {output: sha256}}, "one_core":
{"cin x cout": conv2d_wgrad and ppo_wenc_grad agree bit for bit}} over tests/train_kernel_cases.py.  Two builds of the library that
compute the same thing print the same "cases" (ADAF_LIB=<other build> for the other side).  The recording of the build before the
split-K kernels were merged into one core is tests/golden/g21_train_kernel_bits.json; it is not regenerated from later builds.
Usage: python tools/train_kernel_digest.py > bits.json"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests import train_kernel_cases as T  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    one = {"%dx%d" % s: bool(torch.equal(*T.one_core_pair(*s, dev))) for s in T.ONE_CORE_SHAPES}
    print(json.dumps(dict(cus=T.device_cus(dev), cases=T.digests(dev), one_core=one), sort_keys=True))


if __name__ == "__main__":
    main()
