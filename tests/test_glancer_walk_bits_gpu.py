"""One step of the glancer's training walk computes, bit for bit, what it computed when it stated its own conv + BatchNorm layer
treatment, before that moved into the core it shares with the trunk (adafocus_amd/layer_train.py): tests/golden/glancer_walk_bits.json holds
one sha256 per tensor -- the features, every parameter gradient and every running statistic after the step -- over
tests/glancer_walk_bits_cases.py, recorded from that code on an MI355X (tools/glancer_walk_bits.py) and never regenerated from the code under
test.  On a mismatch the launch trace of the nearest host case (tools/glancer_walk_launches.py --dump) names the operand that differs."""
import json
import os

import pytest
import torch

from tests import glancer_walk_bits_cases as T
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "glancer_walk_bits.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def test_the_recording_covers_the_case_list():
    assert set(RECORDED["cases"]) == set(T.CASES)


@pytest.mark.parametrize("name", list(T.CASES))
def test_bits_equal_the_recorded_walk(dev, name):
    if T.device_cus(dev) != RECORDED["cus"]:
        pytest.skip("the conv engine plans its tiles for the device's %d CUs; the recording is from %d" % (T.device_cus(dev), RECORDED["cus"]))
    got, want = T.digest(name, dev), RECORDED["cases"][name]
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, (name, len(differ), differ[:8])
