"""CPU checks of the opt-in fp16 ResNet-50 trunk's host surface (ADAF_MATH_F16): the header's enum value, the Python constant, and the
build-specific ``args.local_math`` of both GFV models (no GPU needed: the math mode is recorded on the module and handed to the trunk when
it is built)."""
import os
import re

import pytest

from adafocus_amd import _lib, resnet
from tests.test_state_dict_compat import act_args, sth_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_math_f16():
    header = open(os.path.join(ROOT, "include", "adafocus.h")).read()
    m = re.search(r"enum\s*\{\s*ADAF_MATH_F32\s*=\s*0\s*,\s*ADAF_MATH_F32_SPLIT_BF16\s*=\s*1\s*,\s*ADAF_MATH_F16\s*=\s*(\d+)\s*\}", header)
    assert m and int(m.group(1)) == 2
    assert _lib.MATH_F16 == 2
    from adafocus_amd import hip_ops
    assert hip_ops.MATH_F16 == 2


def test_resnet_set_math_accepts_f16_and_rejects_unknown():
    net = resnet.resnet50()
    assert net.math == resnet.DEFAULT_MATH == "f32"
    net.set_math("f16")
    assert net.math == "f16"
    net.set_math("split_bf16")
    assert net.math == "split_bf16"
    with pytest.raises(ValueError):
        net.set_math("bf16")


def _act(**kw):
    from adafocus_amd.gfv_net import GFV
    a = act_args()
    a.__dict__.update(kw)
    return GFV(a)


def _sth(**kw):
    from adafocus_amd.gfv_net_sth import GFV
    a = sth_args()
    a.__dict__.update(kw)
    return GFV(a)


@pytest.mark.parametrize("build,local", [(_act, lambda m: m.focuser.net), (_sth, lambda m: m.focuser.net.base_model)], ids=["act", "sth"])
def test_local_math_reaches_the_resnet_local_cnn(build, local):
    assert local(build()).math == "f32"                      # default: unchanged
    assert local(build(local_math="f32")).math == "f32"
    assert local(build(local_math="f16")).math == "f16"
    assert local(build(local_math="split_bf16")).math == "split_bf16"
    with pytest.raises(ValueError):
        build(local_math="bogus")


@pytest.mark.parametrize("build", [_act, _sth], ids=["act", "sth"])
def test_local_math_is_refused_for_an_efficientnet_local_cnn(build):
    with pytest.raises(ValueError):
        build(local_arch="efficientnet-b3", local_math="f16")


def test_efficientnet_keeps_local_dtype_with_default_local_math():
    m = _act(local_arch="efficientnet-b3", local_math="f32")
    assert not isinstance(m.focuser.net, resnet.ResNet)


def test_glancer_policy_and_classifier_are_untouched_by_local_math():
    """Only the local CNN changes: everything outside the trunk keeps its fp32 parameters."""
    import torch
    m = _act(local_math="f16")
    for name, p in m.named_parameters():
        assert p.dtype == torch.float32, name
