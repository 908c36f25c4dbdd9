"""Stage-1 training surface without a device: the new exports, the workspace query's arithmetic, the NULL-handle refusals,
the module-state table of GFV.stage1_train_mode and its refusals, and the G22 fixtures (tests/golden/g22_act_stage1_*.npz): they parse,
and the torch-CPU restatement of the step (tests/stage1_reference.py, float64) reproduces what the reference model produced -- every
stored quantity within max(2^-22, its stored fp32-vs-fp64 spread) of the fixture, relative to its largest entry (2^-22: the fixture holds
float64 results rounded to fp32, and the running statistics' spreads lie below that rounding)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from adafocus_amd import _lib, resnet, synth, train
from adafocus_amd.gfv_net import GFV
from tests import stage1_reference as R
from tests.helpers import golden, rnd
from tests.test_abi import _ensure_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adaf_ce_steps_workspace_bytes", "adaf_ce_steps_f32")
STORED = 2.0 ** -22
CASES = ("g22_act_stage1_p0", "g22_act_stage1_mask")


def args_of(g, **over):
    b, t, s, p, glance, c, hidden = (int(v) for v in g["dims"])
    a = dict(num_segments=t, num_classes=c, reward="random", dataset="actnet", input_size=s, batch_size=b, patch_size=p, with_glancer=True,
             feature_map_channels=1280, glance_size=glance, action_dim=49, hidden_state_dim=1024, policy_conv=True, gpu=0, continuous=False,
             gamma=0.7, policy_lr=0.0003, random_patch=True, dropout=float(g["dropout"][0]), consensus="gru", hidden_dim=hidden, train_stage=1,
             local_math="f32")          # (said, not left to resnet.DEFAULT_MATH: the parity modules run the suite under both defaults)
    a.update(over)
    return types.SimpleNamespace(**a)


def state_dict_of(g, model):
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    return {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, int(g["seeds"][0])).items()}


@pytest.fixture(scope="module")
def model():
    return GFV(args_of(golden(CASES[0])))


def test_new_exports_declared_everywhere():
    _ensure_built()
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name)
    assert lib.adaf_version() == 303
    # the workspace: one float per row
    for b, t in ((1, 1), (2, 3), (32, 16), (129, 2), (40000, 60000)):
        assert lib.adaf_ce_steps_workspace_bytes(b, t) == b * t * 4
    for bad in ((0, 4), (4, 0), (-1, 4), (4, -7)):
        assert lib.adaf_ce_steps_workspace_bytes(*bad) == 0
    # refused before anything touches a device
    assert lib.adaf_ce_steps_f32(None, None, None, 2, 3, 10, None, None, None, 0, None) == -1


def test_train_stage1_batch_is_exported():
    assert "train_stage1_batch" in train.__all__ and callable(train.train_stage1_batch)
    from adafocus_amd import hip_ops
    assert callable(hip_ops.ce_steps) and issubclass(hip_ops.CeStepsFn, torch.autograd.Function)


def test_stage1_train_mode_table(model):
    model.eval()
    assert not model._in_stage1_train_state()
    model.train()
    assert not model._in_stage1_train_state()              # a plain .train(): the glancer is in train mode
    x = torch.zeros(1, 6, 8, 8)
    with pytest.raises(NotImplementedError):
        model(input=x, scan=x, backbone_pred=False, one_step=False)
    model.stage1_train_mode()
    net = model.focuser.net
    assert model.training and model.focuser.training and model.classifier.training and model.dropout.training
    assert net.training and all(m.training for m in net.modules()) and net.trainable and net.bn_batch_stats
    assert not any(m.training for m in model.glancer.modules())
    assert model._in_stage1_train_state()
    model.glancer.train()
    assert not model._in_stage1_train_state()
    model.stage1_train_mode()
    net.set_bn_batch_stats(False)
    assert not model._in_stage1_train_state()
    model.stage1_train_mode()
    model.eval()
    assert not model._in_stage1_train_state() and not net.training
    with pytest.raises(NotImplementedError, match="training=False"):
        model(input=x, scan=x, backbone_pred=False, one_step=False, training=True)


def test_train_mode_still_raises_for_stages_0_to_2(model):
    for stage in (0, 1, 2):
        with pytest.raises(NotImplementedError, match="policy_train_mode"):
            model.train_mode(types.SimpleNamespace(train_stage=stage))
    with pytest.raises(NotImplementedError, match="stage1_train_mode"):
        model.train_mode(types.SimpleNamespace(train_stage=1))
    model.eval()


def test_stage1_train_mode_refusals():
    g = golden(CASES[0])
    with pytest.raises(NotImplementedError, match="policy-driven"):
        GFV(args_of(g, random_patch=False)).stage1_train_mode()
    with pytest.raises(NotImplementedError, match="consensus='fc'"):
        GFV(args_of(g, consensus="fc")).stage1_train_mode()
    with pytest.raises(NotImplementedError, match="ResNet local CNN only"):
        GFV(args_of(g, local_arch="efficientnet-b0", local_dtype="f32")).stage1_train_mode()
    for math in ("f16", "split_bf16"):
        m = GFV(args_of(g, local_math=math))
        with pytest.raises(NotImplementedError, match="fp32 only"):
            m.stage1_train_mode()
        assert not m.training or not m._in_stage1_train_state()


@pytest.mark.parametrize("case", CASES)
def test_g22_fixture_parses(case):
    g = golden(case)
    b, t, s, p, glance, c, hidden = (int(v) for v in g["dims"])
    assert (b, t, s, p, glance, c, hidden) == (2, 2, 96, 64, 64, 10, 1024)
    assert g["logits"].shape == (b * t, c) and g["last"].shape == (b, c) and g["logits_after"].shape == (b * t, c)
    assert np.array_equal(g["last"], g["logits"].reshape(b, t, c)[:, -1])
    assert g["origins"].shape == (b * t, 2) and g["origins"].min() >= 0 and g["origins"].max() < s - p
    np.random.seed(int(g["seeds"][2]))
    assert np.array_equal(g["origins"], [[np.random.randint(0, s - p), np.random.randint(0, s - p)] for _ in range(b * t)])
    assert len(g["names_bn"]) == 106 and len(g["names_conv"]) == 53 and len(g["names_stat"]) == 106
    assert g["bn"].size == g["stat"].size == 2 * 26560
    assert abs(g["fc_bias"].sum()) < 1e-6                # softmax - onehot sums to zero over the classes
    if case.endswith("mask"):
        assert g["dropout"][0] == 0.5 and g["mask"].shape == (b, t, hidden) and set(np.unique(g["mask"])) == {0.0, 2.0}
    else:
        assert g["dropout"][0] == 0.0 and "mask" not in g.files
    for k in g.files:
        if k.startswith("spread_"):
            sp = g[k]
            assert np.isfinite(sp).all() and 0 < sp.max() < 1e-4, k       # no ReLU branch changed between the stored fp32 and fp64 runs
    assert g["relu_margin"][0] > 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", case + ".npz")) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_cpu_restatement_reproduces_g22(case, model):
    g = golden(case)
    b, t, s, p, glance, c, hidden = (int(v) for v in g["dims"])
    lr, momentum, wd = (float(v) for v in g["sgd"])
    images = torch.from_numpy(synth.synth_frames(b, t, s, seed=int(g["seeds"][1])))
    mask = torch.from_numpy(g["mask"]) if "mask" in g.files else None
    r = R.stage1_step(state_dict_of(g, model), images, torch.from_numpy(g["target"]), g["origins"], p, glance, resnet.DEPTHS["resnet50"], lr,
                      momentum, wd, torch.float64, mask)
    rows = R.fixture_rows(g, r, rnd)
    assert len(rows) == 12 + 106 + 2 * 53 + 106
    bad = [row for row in rows if not row[0] <= max(STORED, row[1])]
    assert not bad, bad[:8]
    assert all(int(v) == 1 for k, v in r["state"].items() if k.endswith("num_batches_tracked"))
    assert not any(k.startswith(("glancer.", "focuser.net.fc.")) for k in r["grads"])
