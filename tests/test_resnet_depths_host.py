"""CPU checks of the ResNet-101 / ResNet-152 local CNN (base_model = 'resnet101' / 'resnet152', STH/models/tsn.py:109-145): the
state-dict spellings the reference's TSN gives per block (tests/golden/g16_resnet_depths.npz key lists), make_temporal_shift's n_round
rule, the base_model names TSN accepts and refuses, local_math at every depth and the unchanged workspace size.  No forward pass."""
import ctypes

import pytest
import torch

from adafocus_amd import _lib
from adafocus_amd.resnet import DEPTHS, ResNet, check_local_math, resnet50, resnet101, resnet152
from adafocus_amd.tsn import TSN
from tests.helpers import golden


def _tsn(arch, place="blockres", div=8, stripped=False):
    net = TSN(4, "RGB", base_model=arch, is_shift=True, shift_div=div, shift_place=place)
    if stripped:
        net.base_model = torch.nn.Sequential(*list(net.base_model.children())[:-1])       # STH/evaluate.py:83
    return net


def test_tsn_resnet101_constructs():
    net = TSN(8, base_model="resnet101")
    assert net.base_model.layers == (3, 4, 23, 3) and len(net.base_model.layer3) == 23
    assert net.feature_dim == 2048 and net.base_model.fc.weight.shape == (1000, 2048)


@pytest.mark.parametrize("arch", ["resnet50", "resnet101", "resnet152"])
def test_tsn_accepts_the_bottleneck_depths(arch):
    net = TSN(8, base_model=arch, is_shift=True)
    assert net.base_model.layers == DEPTHS[arch] and net.feature_dim == 2048


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnext50_32x4d", "resnext101_32x8d", "wide_resnet50_2", "wide_resnet101_2",
                                  "resnet", "resnet1010"])
def test_tsn_refuses_other_base_models(arch):
    with pytest.raises(NotImplementedError, match="resnet50, resnet101, resnet152"):
        TSN(8, base_model=arch)


def test_constructors_and_layer_counts():
    assert resnet50().layers == (3, 4, 6, 3)
    assert resnet101().layers == (3, 4, 23, 3) and len(resnet101().layer3) == 23
    net = resnet152()
    assert [len(getattr(net, "layer%d" % i)) for i in range(1, 5)] == [3, 8, 36, 3]
    assert net.feature_dim == 2048
    with pytest.raises(NotImplementedError):
        ResNet(layers=(2, 2, 2, 2))


def test_n_round_rule():
    """temporal_shift.py:123-136: n_round = 2 iff layer3 has >= 23 blocks; blocks i % n_round == 0 of EVERY stage are shifted."""
    assert resnet50().n_round == 1 and resnet101().n_round == 2 and resnet152().n_round == 2
    assert resnet50().shifted_blocks(3) == list(range(6))
    assert resnet101().shifted_blocks(1) == [0, 2] and resnet101().shifted_blocks(2) == [0, 2]
    assert resnet101().shifted_blocks(3) == list(range(0, 23, 2)) and resnet101().shifted_blocks(4) == [0, 2]
    assert resnet152().shifted_blocks(2) == [0, 2, 4, 6] and resnet152().shifted_blocks(3) == list(range(0, 36, 2))


@pytest.mark.parametrize("d,arch", [("r101", "resnet101"), ("r152", "resnet152")])
def test_state_dict_keys_match_reference(d, arch):
    """Per block: a shifted block's conv1 is `conv1.net.weight`, an unshifted one `conv1.weight` -- full and Sequential-stripped."""
    g = golden("g16_resnet_depths")
    full, stripped = _tsn(arch), _tsn(arch, stripped=True)
    assert sorted(full.state_dict()) == list(g[d + "_keys_full"])
    assert sorted(stripped.state_dict()) == list(g[d + "_keys_stripped"])
    keys = set(stripped.state_dict())
    assert "base_model.6.0.conv1.net.weight" in keys and "base_model.6.1.conv1.weight" in keys
    assert "base_model.6.1.conv1.net.weight" not in keys and "base_model.6.0.conv1.weight" not in keys
    assert "base_model.layer3.0.conv1.net.weight" in full.state_dict() and "base_model.layer3.1.conv1.weight" in full.state_dict()


@pytest.mark.parametrize("arch", ["resnet101", "resnet152"])
@pytest.mark.parametrize("stripped", [False, True], ids=["full", "stripped"])
def test_mixed_spellings_round_trip(arch, stripped):
    """A reference checkpoint with both spellings in one net loads strict and saves back to the same keys and values."""
    src = _tsn(arch, stripped=stripped)
    gen = torch.Generator().manual_seed(7)
    sd = {k: (torch.randn(v.shape, generator=gen) if v.is_floating_point() else v.clone()) for k, v in src.state_dict().items()}
    dst = _tsn(arch, stripped=stripped)
    dst.load_state_dict(sd, strict=True)
    back = dst.state_dict()
    assert sorted(back) == sorted(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    # the canonical (torchvision) name of an unshifted block's conv1 holds the tensor its reference spelling carried
    pre = "base_model.6." if stripped else "base_model.layer3."
    assert torch.equal(dst.base_model.layer3[1].conv1.weight, sd[pre + "1.conv1.weight"])
    assert torch.equal(dst.base_model.layer3[2].conv1.weight, sd[pre + "2.conv1.net.weight"])


def test_block_placement_wraps_every_block():
    keys = set(_tsn("resnet101", place="block").state_dict())
    assert all(("base_model.layer3.%d.net.conv1.weight" % i) in keys for i in range(23))


@pytest.mark.parametrize("arch", ["resnet50", "resnet101", "resnet152"])
@pytest.mark.parametrize("mode", ["f32", "split_bf16", "f16"])
def test_check_local_math_every_depth(arch, mode):
    assert check_local_math(mode, arch) == mode
    net = TSN(8, base_model=arch, is_shift=True).base_model
    net.set_math(mode)
    assert net.math == mode


def test_check_local_math_still_refuses_other_local_cnns():
    with pytest.raises(ValueError):
        check_local_math("f16", "efficientnet-b3")
    with pytest.raises(ValueError):
        check_local_math("bf16", "resnet101")


def test_sth_gfv_builds_with_resnet101():
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.base_model = "resnet101"
    m = GFV(a)
    keys = set(m.state_dict())
    assert "focuser.net.base_model.layer3.22.conv1.weight" not in keys and "focuser.net.base_model.layer3.22.conv1.net.weight" in keys
    assert "focuser.net.base_model.layer3.21.conv1.weight" in keys


def test_workspace_bytes_unchanged():
    """Every depth has the same largest map: the NULL-net workspace size is ResNet-50's (tests/test_abi.py pins the same numbers)."""
    lib = _lib.load_library()
    assert lib.adaf_resnet50_workspace_bytes.restype is ctypes.c_size_t
    assert lib.adaf_resnet50_workspace_bytes(None, 4, 96) == 5 * 4 * 48 * 48 * 64 * 4
    assert lib.adaf_resnet50_workspace_bytes(None, 1, 98) == 5 * 25 * 25 * 256 * 4

