"""Stage-0 training surface without a device: the opt-in's default, the mode table of GFV.backbone_train_mode, the refusal
that stays when the opt-in is off, the new exports, and the G21 fixture (tests/golden/g21_act_stage0.npz): it parses, and the torch-CPU
restatement of the step (tests/stage0_reference.py, float64) reproduces what the reference model produced."""
import re
import os
import types

import numpy as np
import pytest
import torch

from adafocus_amd import _lib, resnet, synth
from adafocus_amd.gfv_net import GFV
from tests import stage0_reference as R
from tests.helpers import golden, rnd
from tests.test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adaf_bn_map_workspace_bytes", "adaf_bn_map_train_forward_f32", "adaf_bn_map_train_backward_f32")
STORED = 2.0 ** -22         # the fixture holds float64 results rounded to fp32: a few units in the last place of the largest entry


def _args(g):
    b, t, s, c = (int(v) for v in g["dims"])
    return types.SimpleNamespace(num_segments=t, num_classes=c, reward="random", dataset="actnet", input_size=s, batch_size=b, patch_size=32,
                                 with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024,
                                 policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.5,
                                 consensus="gru", hidden_dim=1024, train_stage=0)


@pytest.fixture(scope="module")
def g21():
    return golden("g21_act_stage0")


@pytest.fixture(scope="module")
def model(g21):
    return GFV(_args(g21))


def test_opt_in_is_off_by_default():
    net = resnet.resnet50()
    assert net.bn_batch_stats is False and net.trainable is False
    net.set_bn_batch_stats(True)
    assert net.bn_batch_stats is True and net.trainable is False          # the opt-in does not switch the training walk on by itself
    net.set_bn_batch_stats(False)
    assert net.bn_batch_stats is False


def test_opt_in_off_still_refuses_train_mode():
    net = resnet.resnet50()
    net.set_trainable(True)
    net.train()
    with pytest.raises(RuntimeError, match="batch-statistics"):
        net.features_train_nhwc4(torch.zeros(1, 32, 32, 4))
    net.set_bn_batch_stats(True)
    net.set_bn_batch_stats(False)
    with pytest.raises(RuntimeError, match="batch-statistics"):
        net.features_train_nhwc4(torch.zeros(1, 32, 32, 4))


def test_backbone_train_mode_table(model):
    model.train()
    model.backbone_train_mode()
    net = model.focuser.net
    assert net.training and all(m.training for m in net.modules())
    assert net.trainable and net.bn_batch_stats
    assert not model.training and not model.focuser.training
    for m in (model.glancer, model.classifier, model.focuser.policy.policy, model.focuser.policy.policy_old):
        assert not any(x.training for x in m.modules())
    with pytest.raises(NotImplementedError, match="MobileNetV2"):
        model.backbone_train_mode(glancer=True)
    # the other stages' entries are what they were
    for stage in (0, 1, 2):
        with pytest.raises(NotImplementedError):
            model.train_mode(types.SimpleNamespace(train_stage=stage))
    model.eval()
    assert not net.training


def test_new_exports_declared_everywhere():
    _ensure_built()
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.adaf_version() == 303
    # the workspace: two double sums per (slice, column); the slice count is a function of the column count alone
    for rows in (2, 1000, 4_200_000):
        assert lib.adaf_bn_map_workspace_bytes(rows, 64) == 2 * 2048 * 64 * 8
        assert lib.adaf_bn_map_workspace_bytes(rows, 256) == 2 * 2048 * 256 * 8
        assert lib.adaf_bn_map_workspace_bytes(rows, 2048) == 2 * 256 * 2048 * 8
    for bad in ((0, 64), (64, 0), (-3, 64), (64, 62)):
        assert lib.adaf_bn_map_workspace_bytes(*bad) == 0
    # refused before anything touches a device
    assert lib.adaf_bn_map_train_forward_f32(None, None, 2, 64, None, None, 1e-5, 0.1, None, None, None, 1, None, None, None, None, 0, None) == -1
    assert lib.adaf_bn_map_train_backward_f32(None, None, None, None, 2, 64, *([None] * 7), 0, None) == -1


def test_g21_fixture_parses(g21):
    g = g21
    b, t, s, c = (int(v) for v in g["dims"])
    assert (b, t, s) == (2, 2, 64) and 2 <= c <= 16
    assert g["logits"].shape == (b * t, c) and g["pred"].shape == (b, c) and g["logits_after"].shape == (b * t, c)
    assert np.allclose(g["pred"], g["logits"].reshape(b, t, c).mean(1), atol=1e-6)
    assert len(g["names_bn"]) == 106 and len(g["names_conv"]) == 53 and len(g["names_stat"]) == 106
    assert g["bn"].size == g["stat"].size == 2 * 26560
    assert abs(g["fc_bias"].sum()) < 1e-6                # softmax - onehot sums to zero over the classes
    for k in ("logits", "pred", "loss", "fc_weight", "fc_bias", "logits_after", "bn", "conv_Gv", "conv_uG", "stat"):
        sp = g["spread_" + k]
        assert np.isfinite(sp).all() and 0 < sp.max() < 1e-4, k       # no ReLU branch changed between the stored fp32 and fp64 runs
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g21_act_stage0.npz")) < 1 << 20


def test_cpu_restatement_reproduces_g21(g21, model):
    g = g21
    b, t, s, c = (int(v) for v in g["dims"])
    lr, momentum, wd = (float(v) for v in g["sgd"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    prefix = "focuser.net."
    sd = {k[len(prefix):]: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, int(g["seeds"][0])).items() if k.startswith(prefix)}
    name, ch = str(g["zero_gamma_name"][0]), int(g["zero_gamma_channel"][0])
    sd[name[len(prefix):]][ch] = 0.0
    images = torch.from_numpy(synth.synth_frames(b, t, s, seed=int(g["seeds"][1])))
    r = R.stage0_step(sd, images, torch.from_numpy(g["target"]), resnet.DEPTHS["resnet50"], lr, momentum, wd, torch.float64)

    def close(tag, got, ref):
        ref = np.asarray(ref, dtype=np.float64)
        err = np.abs(got.double().numpy().reshape(ref.shape) - ref).max() / np.abs(ref).max()
        assert err <= STORED, (tag, err)

    close("logits", r["logits"], g["logits"])
    close("pred", r["pred"], g["pred"])
    close("loss", r["loss"], g["loss"])
    close("fc.weight", r["grads"]["fc.weight"], g["fc_weight"])
    close("fc.bias", r["grads"]["fc.bias"], g["fc_bias"])
    close("logits_after", r["logits_after"], g["logits_after"])
    off = 0
    for n in g["names_bn"].tolist():
        grad = r["grads"][n[len(prefix):]]
        close(n, grad, g["bn"][off:off + grad.numel()])
        off += grad.numel()
    off_v = off_u = 0
    for n in g["names_conv"].tolist():
        gv, ug = R.project(r["grads"][n[len(prefix):]], rnd)
        close(n + "@v", gv, g["conv_Gv"][off_v:off_v + gv.numel()])
        close("u@" + n, ug, g["conv_uG"][off_u:off_u + ug.numel()])
        off_v, off_u = off_v + gv.numel(), off_u + ug.numel()
    off = 0
    for n in g["names_stat"].tolist():
        v = r["state"][n[len(prefix):]]
        close(n, v, g["stat"][off:off + v.numel()])
        off += v.numel()
    assert all(int(v) == 1 for k, v in r["state"].items() if k.endswith("num_batches_tracked"))
