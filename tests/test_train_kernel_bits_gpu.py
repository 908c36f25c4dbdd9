"""G21: the training kernels compute, bit for bit, what the build before the split-K weight gradients were merged into one core
(csrc/splitk_wgrad.h) and the shared launchers moved to csrc/train_common.hip computed: tests/golden/g21_train_kernel_bits.json holds
sha256 digests of every output over tests/train_kernel_cases.py, recorded from that build (tools/train_kernel_digest.py) and never
regenerated from the code under test.  And the two callers of the core agree with each other where their plans coincide."""
import json
import os

import pytest
import torch

from tests import train_kernel_cases as T
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "g21_train_kernel_bits.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def test_the_recording_covers_the_case_list():
    assert set(RECORDED["cases"]) == set(T.CASES)


@pytest.mark.parametrize("name", list(T.CASES))
def test_bits_equal_the_recorded_build(dev, name):
    if T.CASES[name][1] and T.device_cus(dev) != RECORDED["cus"]:
        pytest.skip("the PPO split-K launch plans its slices for the device's %d CUs; the recording is from %d" % (T.device_cus(dev), RECORDED["cus"]))
    got = T.digest(name, dev)
    assert got == RECORDED["cases"][name], name


@pytest.mark.parametrize("cin,cout", T.ONE_CORE_SHAPES)
def test_conv_and_ppo_weight_gradients_are_one_core(dev, cin, cout):
    """A 1x1 stride-1 convolution over (1, 7, 143, cin) and the PPO encoder's ungated gradient over the same 1001 pixels: the same tiles,
    slices and product order on 256 CUs, hence the same bits.  (No shape with 32 outputs and cin % 256 == 0: the PPO path takes
    256-channel tiles there and its slice count differs by design.)"""
    if T.device_cus(dev) < 256:
        pytest.skip("the PPO launch plans for the device's %d CUs, the convolution's for 256" % T.device_cus(dev))
    conv, ppo = T.one_core_pair(cin, cout, dev)
    assert torch.equal(conv, ppo)
