"""Stage-0 training of the glancer without a device: the opt-in's default, the mode table of GFV.glancer_train_mode, its
refusals, the raise that backbone_train_mode(glancer=True) keeps, the new exports, the CPU restatement's layer plan against the model's
own keys, and the G23 fixture (tests/golden/g23_act_stage0_glancer.npz): it parses, and the torch-CPU restatement of the step
(tests/glancer_reference.py, float64, the stored dropout mask) reproduces what the reference model produced."""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib, mobilenet, synth
from adafocus_amd.gfv_net import GFV
from tests import glancer_reference as R
from tests.helpers import golden, rnd
from tests.stage0_reference import project
from tests.test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adaf_dwconv3x3_dgrad_f32", "adaf_dwconv3x3_wgrad_workspace_bytes", "adaf_dwconv3x3_wgrad_f32", "adaf_bn_map_train_forward_act_f32",
       "adaf_bn_map_train_backward_act_f32", "adaf_conv2d_wgrad_rows_workspace_bytes", "adaf_conv2d_wgrad_rows_f32", "adaf_add_f32")
STORED = 2.0 ** -22         # the fixture holds float64 results rounded to fp32: a few units in the last place of the largest entry
PREFIX = "glancer.net."


def _args(g):
    b, t, s, c = (int(v) for v in g["dims"])
    return types.SimpleNamespace(num_segments=t, num_classes=c, reward="random", dataset="actnet", input_size=s, batch_size=b, patch_size=32,
                                 with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024,
                                 policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.5,
                                 consensus="gru", hidden_dim=1024, train_stage=0)


@pytest.fixture(scope="module")
def g23():
    return golden("g23_act_stage0_glancer")


@pytest.fixture(scope="module")
def model(g23):
    return GFV(_args(g23))


def test_opt_in_is_off_by_default():
    net = mobilenet.mobilenet_v2()
    assert net.trainable is False and net.bn_batch_stats is False
    net.set_bn_batch_stats(True)
    assert net.bn_batch_stats is True and net.trainable is False          # the opt-in does not switch the training walk on by itself
    net.train()
    with pytest.raises(RuntimeError, match="set_trainable"):
        net.features_train_nhwc4(torch.zeros(2, 32, 32, 4))
    with pytest.raises(RuntimeError, match="eval mode only"):
        net.features_from_nhwc4(torch.zeros(2, 32, 32, 4))
    net.set_trainable(True)
    net.set_bn_batch_stats(False)
    with pytest.raises(NotImplementedError, match="batch statistics"):
        net.features_train_nhwc4(torch.zeros(2, 32, 32, 4))


def test_glancer_train_mode_table(model):
    model.train()
    model.glancer_train_mode()
    net = model.glancer.net
    assert net.training and all(m.training for m in net.modules())
    assert net.trainable and net.bn_batch_stats
    assert not model.training and not model.glancer.training
    for m in (model.focuser, model.classifier):
        assert not any(x.training for x in m.modules())
    assert not model.focuser.net.trainable
    with pytest.raises(NotImplementedError, match="MobileNetV2") as e:
        model.backbone_train_mode(glancer=True)
    assert "glancer_train_mode()" in str(e.value)
    model.eval()
    assert not net.training


def test_glancer_train_mode_refuses_another_glancer(model):
    keep = model.glancer.net
    try:
        model.glancer.net = torch.nn.Linear(2, 2)
        with pytest.raises(NotImplementedError, match="MobileNetV2"):
            model.glancer_train_mode()
    finally:
        model.glancer.net = keep


def test_new_exports_declared_everywhere():
    _ensure_built()
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.adaf_version() == 303          # additions only
    # the depthwise weight gradient's workspace: nine double sums per (slice, channel)
    assert lib.adaf_dwconv3x3_wgrad_workspace_bytes(1, 1, 1, 16, 1) == 9 * 1 * 16 * 8
    assert lib.adaf_dwconv3x3_wgrad_workspace_bytes(1024, 112, 112, 96, 1) == 9 * 1024 * 96 * 8
    for bad in ((0, 8, 8, 16, 1), (1, 8, 8, 18, 1), (1, 8, 8, 16, 3), (1, 0, 8, 16, 1)):
        assert lib.adaf_dwconv3x3_wgrad_workspace_bytes(*bad) == 0
    # refused before anything touches a device
    assert lib.adaf_dwconv3x3_dgrad_f32(None, None, 1, 8, 8, 16, 1, None, None, None) == -1
    assert lib.adaf_dwconv3x3_wgrad_f32(None, None, None, 1, 8, 8, 16, 1, None, None, 0, None) == -1
    assert lib.adaf_add_f32(None, None, None, 4, None, None) == -1
    prm = _lib.ConvParams(n=1, h=7, w=7, cin=32, cout=24, kh=1, kw=1, stride=1, pad=0, act=0, tsm_segments=0, tsm_div=0, ldx=0, ldo=0, ldr=0, tile=0)
    import ctypes
    assert lib.adaf_conv2d_wgrad_workspace_bytes(ctypes.byref(prm)) == 0 < lib.adaf_conv2d_wgrad_rows_workspace_bytes(ctypes.byref(prm))


def test_reference_plan_names_the_models_own_keys(model):
    keys = set(k[len(PREFIX):] for k in model.state_dict() if k.startswith(PREFIX + "features."))
    named = set()
    for _, conv, bn, _, _, _, _ in R.plan():
        named.add(conv + ".weight")
        named.update(bn + "." + leaf for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"))
    assert named == keys
    assert len(R.relu6_names()) == 35 and sum(1 for l in R.plan() if l[6] == "res") == 10


def test_g23_fixture_parses(g23, model):
    g = g23
    b, t, s, c = (int(v) for v in g["dims"])
    assert (b, t, s) == (2, 2, 64) and 2 <= c <= 16
    assert g["logits"].shape == (b * t, c) and g["pred"].shape == (b, c) and g["logits_after"].shape == (b * t, c)
    assert np.allclose(g["pred"], g["logits"].reshape(b, t, c).mean(1), atol=1e-6)
    assert len(g["names_bn"]) == 104 and len(g["names_conv"]) == 52 and len(g["names_stat"]) == 104
    assert g["bn"].size == g["stat"].size == 2 * 17056
    assert g["dropout_mask"].shape == (b * t, 1280) and set(np.unique(g["dropout_mask"])) == {0, 1}
    assert abs(g["cls_bias"].sum()) < 1e-6                # softmax - onehot sums to zero over the classes
    assert float(g["relu_margin"][0]) > 0
    # the 17 project BatchNorm biases, whose gradient cancels exactly, are held on their weight gradient's scale; the others on their own
    sizes = [model.state_dict()[n].numel() for n in g["names_bn"].tolist()]
    own = np.array([np.abs(c).max() for c in np.split(g["bn"], np.cumsum(sizes)[:-1])])
    lifted = [n for n, o, sc in zip(g["names_bn"].tolist(), own, g["scale_bn"]) if sc > 2 * o]
    assert len(lifted) == 17 and all(n.endswith(".bias") and len(n.split(".")) == 7 for n in lifted)      # glancer.net.features.i.conv.k.bias
    assert all(abs(sc - o) <= 1e-6 * o for o, sc in zip(own, g["scale_bn"]) if not sc > 2 * o)
    for k in ("logits", "pred", "loss", "cls_weight", "cls_bias", "logits_after", "bn", "conv_Gv", "conv_uG", "stat"):
        sp = g["spread_" + k]
        assert np.isfinite(sp).all() and 0 < sp.max() < 1e-4, k       # no ReLU6 branch changed between the stored fp32 and fp64 runs
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g23_act_stage0_glancer.npz")) < 1 << 20


def test_cpu_restatement_reproduces_g23(g23, model):
    g = g23
    b, t, s, c = (int(v) for v in g["dims"])
    lr, momentum, wd = (float(v) for v in g["sgd"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = {k[len(PREFIX):]: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, int(g["seeds"][0])).items() if k.startswith(PREFIX)}
    name, ch = str(g["zero_gamma_name"][0]), int(g["zero_gamma_channel"][0])
    sd[name[len(PREFIX):]][ch] = 0.0
    images = torch.from_numpy(synth.synth_frames(b, t, s, seed=int(g["seeds"][1])))
    mask = torch.from_numpy(g["dropout_mask"]).double() / float(g["dropout_keep"][0])
    p = R.cast(sd, torch.float64)
    x = images.double().view(b * t, 3, s, s)
    logits = F.linear(R.features(p, x, True) * mask, p["classifier.1.weight"], p["classifier.1.bias"])
    pred = logits.view(b, t, -1).mean(1, keepdim=True).squeeze(1)
    loss = F.cross_entropy(pred, torch.from_numpy(g["target"]))
    names = [k for k, v in p.items() if v.requires_grad]
    grads = dict(zip(names, torch.autograd.grad(loss, [p[k] for k in names])))
    opt = torch.optim.SGD([p[k] for k in names], lr=lr, momentum=momentum, weight_decay=wd)
    for k in names:
        p[k].grad = grads[k].clone()
    opt.step()
    with torch.no_grad():
        after = F.linear(R.features(p, x, False), p["classifier.1.weight"], p["classifier.1.bias"])

    def close(tag, got, ref, scale=None):
        ref = np.asarray(ref, dtype=np.float64)
        err = np.abs(got.detach().double().numpy().reshape(ref.shape) - ref).max() / (np.abs(ref).max() if scale is None else float(scale))
        assert err <= STORED, (tag, err)

    close("logits", logits, g["logits"])
    close("pred", pred, g["pred"])
    close("loss", loss, g["loss"])
    close("classifier.1.weight", grads["classifier.1.weight"], g["cls_weight"])
    close("classifier.1.bias", grads["classifier.1.bias"], g["cls_bias"])
    close("logits_after", after, g["logits_after"])
    off = 0
    for i, n in enumerate(g["names_bn"].tolist()):
        grad = grads[n[len(PREFIX):]]
        close(n, grad, g["bn"][off:off + grad.numel()], g["scale_bn"][i])
        off += grad.numel()
    off_v = off_u = 0
    for n in g["names_conv"].tolist():
        gv, ug = project(grads[n[len(PREFIX):]], rnd)
        close(n + "@v", gv, g["conv_Gv"][off_v:off_v + gv.numel()])
        close("u@" + n, ug, g["conv_uG"][off_u:off_u + ug.numel()])
        off_v, off_u = off_v + gv.numel(), off_u + ug.numel()
    off = 0
    for n in g["names_stat"].tolist():
        v = p[n[len(PREFIX):]]
        close(n, v, g["stat"][off:off + v.numel()])
        off += v.numel()
    assert all(int(v) == 1 for k, v in p.items() if k.endswith("num_batches_tracked"))
