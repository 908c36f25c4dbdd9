"""train_stage0_glancer_batch on the MI355X against the reference's own step (G23, tests/golden/g23_act_stage0_glancer.npz, made by
tools/gen_golden_stage0_glancer.py from ACT/main_dist.py:544-548 with pretrain_glancer=True): logits, prediction, loss, the classifier's
gradients, every BatchNorm gradient, every conv weight gradient as G17's two projections, the running statistics and the eval logits
after the SGD step.  A project BatchNorm's bias gradient is exactly zero in exact arithmetic (a 1x1 convolution and a BatchNorm on batch
statistics read every block output); it is held on the scale of the same BatchNorm's weight gradient (`scale_bn` of the fixture).  The Dropout(0.2) mask the reference drew is injected through `dropout_mask`.

Tolerance (G17's rule, tests/test_stage3_gpu.py; SPREAD_FACTOR of tests/trunk_walk_harness.py): the error against the stored float64
result, relative to the quantity's largest entry, is at most 50x the stored distance of the reference's fp32 run from its float64 run."""
import types

import numpy as np
import pytest
import torch

from adafocus_amd import synth
from adafocus_amd.train import train_stage0_glancer_batch
from tests import stage0_reference as R
from tests.helpers import golden, rnd
from tests.trunk_walk_harness import SPREAD_FACTOR

pytestmark = pytest.mark.gpu
PREFIX = "glancer.net."


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _args(g):
    b, t, s, c = (int(v) for v in g["dims"])
    return types.SimpleNamespace(num_segments=t, num_classes=c, reward="random", dataset="actnet", input_size=s, batch_size=b, patch_size=32,
                                 with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024,
                                 policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.5,
                                 consensus="gru", hidden_dim=1024, train_stage=0)


def _model(g, dev):
    from adafocus_amd.gfv_net import GFV
    m = GFV(_args(g))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, int(g["seeds"][0])).items()}, strict=True)
    with torch.no_grad():
        m.state_dict(keep_vars=True)[str(g["zero_gamma_name"][0])][int(g["zero_gamma_channel"][0])] = 0.0
    return m.to(dev)


def _check(tag, got, ref, spread, scale=None):
    """scale: what the error is relative to (None: the reference's largest entry)."""
    ref = np.asarray(ref, dtype=np.float64)
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    return np.abs(got.reshape(ref.shape) - ref).max() / (np.abs(ref).max() if scale is None else float(scale)), float(spread), tag


def test_train_stage0_glancer_batch_matches_the_reference_g23(dev):
    g = golden("g23_act_stage0_glancer")
    b, t, s, c = (int(v) for v in g["dims"])
    lr, momentum, wd = (float(v) for v in g["sgd"])
    images = torch.from_numpy(synth.synth_frames(b, t, s, seed=int(g["seeds"][1]))).to(dev)
    target = torch.from_numpy(g["target"]).to(dev)
    mask = (torch.from_numpy(g["dropout_mask"]).float() / float(g["dropout_keep"][0])).to(dev)
    twin = _model(g, dev)
    twin.glancer_train_mode()
    with torch.no_grad():
        frames = twin.glancer.net.forward_train(images.view(b * t, 3, s, s), dropout_mask=mask)
    m = _model(g, dev)
    m.glancer_train_mode()
    net = m.glancer.net
    assert net.training and not m.focuser.training and not m.classifier.training
    opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    pred, loss = train_stage0_glancer_batch(m, images, target, _args(g), opt, dropout_mask=mask)
    assert not pred.requires_grad and not loss.requires_grad
    for k, p in m.named_parameters():
        if not k.startswith(PREFIX):
            assert p.grad is None, k
    params = m.state_dict(keep_vars=True)
    lin = net.classifier[1]
    rows = [_check("logits", frames, g["logits"], g["spread_logits"][0]), _check("pred", pred, g["pred"], g["spread_pred"][0]),
            _check("loss", loss.reshape(1), g["loss"], g["spread_loss"][0]),
            _check("classifier.1.weight", lin.weight.grad, g["cls_weight"], g["spread_cls_weight"][0]),
            _check("classifier.1.bias", lin.bias.grad, g["cls_bias"], g["spread_cls_bias"][0])]
    off = 0
    for i, n in enumerate(g["names_bn"].tolist()):
        grad = params[n].grad
        assert grad is not None and torch.isfinite(grad).all(), n
        # (scale_bn: the gradient's own largest entry, or for a project BatchNorm's bias, whose gradient cancels exactly, its weight gradient's)
        rows.append(_check(n, grad, g["bn"][off:off + grad.numel()], g["spread_bn"][i], g["scale_bn"][i]))
        off += grad.numel()
    assert off == g["bn"].size
    off_v = off_u = 0
    for i, n in enumerate(g["names_conv"].tolist()):
        grad = params[n].grad
        assert grad is not None and torch.isfinite(grad).all(), n
        gv, ug = R.project(grad.double().cpu(), rnd)
        rows.append(_check(n + "@v", gv, g["conv_Gv"][off_v:off_v + gv.numel()], g["spread_conv_Gv"][i]))
        rows.append(_check("u@" + n, ug, g["conv_uG"][off_u:off_u + ug.numel()], g["spread_conv_uG"][i]))
        off_v, off_u = off_v + gv.numel(), off_u + ug.numel()
    assert off_v == g["conv_Gv"].size and off_u == g["conv_uG"].size
    off = 0
    for i, n in enumerate(g["names_stat"].tolist()):
        v = params[n]
        rows.append(_check(n, v, g["stat"][off:off + v.numel()], g["spread_stat"][i]))
        off += v.numel()
    assert off == g["stat"].size
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
        elif not k.endswith(("running_mean", "running_var")):
            assert not torch.equal(v, before[k]), k                   # the optimizer stepped every parameter
    # the eval forward after the step: the new weights AND the moved running statistics reach the engine
    m.eval()
    with torch.no_grad():
        after = net(images.view(b * t, 3, s, s))
    rows.append(_check("logits_after", after, g["logits_after"], g["spread_logits_after"][0]))
    rows.sort(key=lambda r: -(r[0] / r[1]))
    print("G23: %d quantities; worst err / spread: %s" % (len(rows), ", ".join("%s %.2e / %.2e = %.2f" % (r[2], r[0], r[1], r[0] / r[1]) for r in rows[:5])))
    bad = [r for r in rows if not r[0] <= SPREAD_FACTOR * r[1]]
    assert not bad, bad[:8]


def test_dropout_is_drawn_when_no_mask_is_given(dev):
    """Without `dropout_mask` the multipliers come from torch's device generator: the same seed gives the same step, another seed
    another one."""
    g = golden("g23_act_stage0_glancer")
    b, t, s, c = (int(v) for v in g["dims"])
    images = torch.from_numpy(synth.synth_frames(b, t, s, seed=int(g["seeds"][1]))).to(dev)
    target = torch.from_numpy(g["target"]).to(dev)
    losses = []
    for seed in (5, 5, 6):
        m = _model(g, dev)
        m.glancer_train_mode()
        opt = torch.optim.SGD(m.glancer.net.parameters(), lr=0.01)
        torch.manual_seed(seed)
        losses.append(train_stage0_glancer_batch(m, images, target, _args(g), opt)[1].item())
    assert losses[0] == losses[1] != losses[2]
