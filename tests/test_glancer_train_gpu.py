"""The training walk of the glancer's MobileNetV2 on the MI355X (adafocus_amd/glancer_train.py) against the float64 CPU
restatement of tests/glancer_reference.py: N = 4 frames of 64 x 64 (the head map is 2 x 2: 16 rows per channel), synthetic weights, one
BatchNorm gamma set to 0.

Features, every parameter gradient and every running statistic are compared ON THE BRANCHES THE DEVICE TOOK at both kinks of every ReLU6.
First the branches themselves are checked, as tests/trunk_walk_harness._device_branches does for the trunk: a unit on another branch than
float64's own must have its float64 pre-activation within 50x the fp32 forward error of its map from the kink it crossed, and at most
0.1 % of a map's units may differ; the test fails otherwise, it does not follow them.

Tolerance (G17's rule, tests/test_stage3_gpu.py; SPREAD_FACTOR of tests/trunk_walk_harness.py): the error against float64, relative to the
quantity's largest entry, is at most 50x the distance between the same CPU computation in fp32 and in fp64.  The CPU references are
computed once and shared."""
import functools

import pytest
import torch

from adafocus_amd import synth
from adafocus_amd.utils import nchw_to_nhwc4
from tests import glancer_reference as R
from tests.helpers import manifest, rnd
from tests.trunk_walk_harness import SPREAD_FACTOR

pytestmark = pytest.mark.gpu

N, SIZE, SEED = 4, 64, 2301
ZERO = ("features.3.conv.1.1", 5)          # a depthwise BatchNorm whose gamma is exactly 0 in one channel
MAX_SHARE = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _state():
    shapes = {k[len("glancer.net."):]: s for k, s in manifest()["ACT"].items() if k.startswith("glancer.net.")}
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, SEED).items()}
    # (the synthetic BatchNorms put their outputs near N(0, 1), far below 6: every third ReLU6 layer gets a wider, shifted affine so that
    #  the upper kink is met -- about a sixth of its units above 6 and a sixth below 0)
    for _, _, bn, _, _, _, _ in [l for l in R.plan() if l[5]][::3]:
        sd[bn + ".weight"] = sd[bn + ".weight"] * 3.0
        sd[bn + ".bias"] = sd[bn + ".bias"] + 3.0
    sd[ZERO[0] + ".weight"][ZERO[1]] = 0.0
    sd[ZERO[0] + ".bias"][ZERO[1]] = 0.5          # (inside (0, 6): the channel's constant output passes its gradient on to dgamma)
    return sd


@functools.lru_cache(maxsize=None)
def _inputs():
    return rnd((N, 3, SIZE, SIZE), SEED + 1), rnd((N, 1280), SEED + 2)


def _net(dev, sd=None):
    from adafocus_amd.mobilenet import MobileNetV2
    net = MobileNetV2(num_classes=200)
    net.load_state_dict(_state() if sd is None else sd, strict=True)
    return net.to(dev).eval()


def _train(net):
    net.train()
    net.set_trainable(True)
    net.set_bn_batch_stats(True)
    return net


def _rel(got, ref64):
    return ((got.double().cpu() - ref64).abs().max() / ref64.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _own_branches():
    """The fp64 and the fp32 CPU forward on their own branches: every ReLU6's input."""
    x, dfeat = _inputs()
    pre64, pre32 = {}, {}
    R.walk(_state(), x, dfeat, torch.float64, pre=pre64)
    R.walk(_state(), x, dfeat, torch.float32, pre=pre32)
    return pre64, pre32


def _branch(z):
    return (z > 0) & (z < 6), z >= 6


def test_torch_fp32_stays_within_the_share_on_the_cpu():
    """What fixing the seed confirmed: torch's own fp32 run differs from float64 in at most 0.1 % of any map's ReLU6 branches."""
    pre64, pre32 = _own_branches()
    for k, z64 in pre64.items():
        p64, a64 = _branch(z64)
        p32, a32 = _branch(pre32[k])
        assert int(((p64 != p32) | (a64 != a32)).sum()) <= MAX_SHARE * z64.numel(), k


def _device_masks(net, dev):
    """The ReLU6 branches of the device's walk, checked against the fp64 forward's pre-activations (module docstring)."""
    from adafocus_amd import glancer_train
    x, _ = _inputs()
    pre64, pre32 = _own_branches()
    with torch.no_grad():
        wk = glancer_train.walk_forward(net, nchw_to_nhwc4(x.to(dev)))
    layers = [wk.stem] + [l for ls, _ in wk.blocks for l in ls] + [wk.head]
    outs = {l.name: wk.kept[id(l)].y for l in layers if l.act != 0}
    assert set(outs) == set(pre64) == set(R.relu6_names())
    masks, differ = {}, 0
    for k, z64 in pre64.items():
        y = outs[k].permute(0, 3, 1, 2).cpu()
        masks[k] = ((y > 0) & (y < 6), y >= 6)
        p64, a64 = _branch(z64)
        d = (masks[k][0] != p64) | (masks[k][1] != a64)
        if d.any():
            err = (pre32[k].double() - z64).abs().max().item()
            worst = torch.minimum(z64[d].abs(), (z64[d] - 6).abs()).max().item()
            print("%s: %d unit(s) of %d on the other branch, within %.2e of a kink, fp32 forward error of the map %.2e" % (
                k, int(d.sum()), d.numel(), worst, err))
            assert worst <= SPREAD_FACTOR * err, (k, worst, err)
            assert int(d.sum()) <= MAX_SHARE * d.numel(), (k, int(d.sum()), d.numel())
            differ += int(d.sum())
    return masks, differ


@functools.lru_cache(maxsize=None)
def _device_run():
    """One device walk for the branches (it moves the statistics of its own net), one training step's forward and backward on a fresh
    net, and the CPU references on the device's branches -- computed once, shared by the tests below."""
    dev = torch.device("cuda:0")
    x, dfeat = _inputs()
    masks, differ = _device_masks(_train(_net(dev)), dev)
    net = _train(_net(dev))
    feat = net.features_train_nhwc4(nchw_to_nhwc4(x.to(dev)))
    feat.backward(dfeat.to(dev))
    ref64 = R.walk(_state(), x, dfeat, torch.float64, masks=masks)
    ref32 = R.walk(_state(), x, dfeat, torch.float32, masks=masks)
    return net, feat.detach(), masks, differ, ref64, ref32


def test_features_gradients_and_statistics_on_the_devices_branches(dev):
    net, feat, masks, differ, (f64, g64, b64), (f32, g32, b32) = _device_run()
    for k, (passes, above) in masks.items():
        assert passes.any() and above.shape == passes.shape, k
    assert any(above.any() for _, above in masks.values()) and any((~p & ~a).any() for p, a in masks.values())      # both kinks are met
    spread, err = _rel(f32, f64), _rel(feat, f64)
    print("features: err %.2e spread %.2e ratio %.3f; %d unit(s) on another branch than float64's" % (err, spread, err / spread, differ))
    assert err <= SPREAD_FACTOR * spread
    params = dict(net.named_parameters())
    worst = []
    for k, r64 in g64.items():
        g = params[k].grad
        assert g is not None and g.shape == r64.shape and torch.isfinite(g).all(), k
        scale = R.grad_scale(g64, k)          # (its own largest entry; a project BatchNorm's bias, which cancels exactly: its weight's)
        assert scale > 0, k
        spread, err = ((g32[k].double() - r64).abs().max() / scale).item(), ((g.double().cpu() - r64).abs().max() / scale).item()
        worst.append((err / spread if spread > 0 else float("inf"), k, err, spread))
    worst.sort(reverse=True)
    print("%d gradients; worst err / spread: %s" % (len(worst), ", ".join("%s %.2e / %.2e = %.2f" % (w[1], w[2], w[3], w[0]) for w in worst[:5])))
    bad = [w for w in worst if not w[2] <= SPREAD_FACTOR * w[3]]
    assert not bad, bad[:8]
    assert params["classifier.1.weight"].grad is None
    # the gamma = 0 channel: a dgamma, no gradient to its filter
    assert params[ZERO[0] + ".weight"].grad[ZERO[1]].item() != 0.0
    assert not params[ZERO[0][:-1] + "0.weight"].grad[ZERO[1]].any()
    buffers = dict(net.named_buffers())
    worst = []
    for k, r64 in b64.items():
        if k.endswith("num_batches_tracked"):
            assert buffers[k].item() == 1 and r64.item() == 1, k
            continue
        spread, err = _rel(b32[k], r64), _rel(buffers[k], r64)
        worst.append((err / spread if spread > 0 else float("inf"), k, err, spread))
    worst.sort(reverse=True)
    print("%d running statistics; worst err / spread: %s" % (len(worst), ", ".join("%s %.2e / %.2e = %.2f" % (w[1], w[2], w[3], w[0]) for w in worst[:3])))
    bad = [w for w in worst if not w[2] <= SPREAD_FACTOR * w[3]]
    assert not bad, bad[:8]


def test_only_the_last_block_and_the_head_trainable(dev):
    """features.17 and features.18 alone: the full run's bits for their gradients, None everywhere else (and the chain stops there)."""
    full = dict(_device_run()[0].named_parameters())
    x, dfeat = _inputs()
    net = _train(_net(dev))
    for k, p in net.named_parameters():
        p.requires_grad_(k.startswith(("features.17.", "features.18.")))
    net.features_train_nhwc4(nchw_to_nhwc4(x.to(dev))).backward(dfeat.to(dev))
    seen = 0
    for k, p in net.named_parameters():
        if k.startswith(("features.17.", "features.18.")):
            assert torch.equal(p.grad, full[k].grad), k
            seen += 1
        else:
            assert p.grad is None, k
    assert seen == 12


def test_the_step_repacks_the_eval_engine(dev):
    """After optimizer.step() the eval forward equals that of a fresh model loaded from the stepped state dict, bit for bit: the walk
    marked the engine stale (a kernel's write to the running statistics moves no tensor version) and the step moved the versions."""
    x, dfeat = _inputs()
    net = _train(_net(dev))
    xd = x.to(dev)
    net.eval()
    before = net.features_nhwc(xd)[1].clone()                       # the engine is packed with the initial statistics
    net.train()
    net.features_train_nhwc4(nchw_to_nhwc4(xd)).backward(dfeat.to(dev))
    net.eval()
    moved = net.features_nhwc(xd)[1].clone()                        # statistics moved by the kernels, parameters untouched
    fresh = _net(dev, {k: v.cpu() for k, v in net.state_dict().items()})
    assert torch.equal(moved, fresh.features_nhwc(xd)[1]) and not torch.equal(moved, before)
    opt = torch.optim.SGD([p for k, p in net.named_parameters() if k.startswith("features.")], lr=0.01, momentum=0.9, weight_decay=1e-4)
    opt.step()
    after = net.features_nhwc(xd)[1]
    fresh = _net(dev, {k: v.cpu() for k, v in net.state_dict().items()})
    assert torch.equal(after, fresh.features_nhwc(xd)[1]) and not torch.equal(after, moved)


def test_opt_in_untouched_and_switched_off_again(dev):
    x, _ = _inputs()
    xd = x.to(dev)
    ref = _net(dev).features_nhwc(xd)[1]
    net = _net(dev)
    assert torch.equal(net.features_nhwc(xd)[1], ref)
    net.train()
    with pytest.raises(RuntimeError, match="eval mode only"):
        net.features_nhwc(xd)
    with pytest.raises(RuntimeError, match="set_trainable"):
        net.features_train_nhwc4(nchw_to_nhwc4(xd))
    net.set_trainable(True)
    net.set_bn_batch_stats(True)
    net.set_trainable(False)
    net.set_bn_batch_stats(False)
    with pytest.raises(RuntimeError, match="eval mode only"):
        net.features_nhwc(xd)
    with pytest.raises(RuntimeError, match="set_trainable"):
        net.features_train_nhwc4(nchw_to_nhwc4(xd))
    net.eval()
    assert torch.equal(net.features_nhwc(xd)[1], ref)
    net.set_trainable(True)
    with pytest.raises(NotImplementedError, match="batch statistics"):
        net.features_train_nhwc4(nchw_to_nhwc4(xd))                # eval mode: a walk on frozen statistics is not built


def test_forward_train_with_a_given_dropout_mask(dev):
    """forward_train = the walk, the mask, the Linear: against the CPU Linear in float64 on the device's features; gradients reach the
    classifier."""
    x, _ = _inputs()
    net = _train(_net(dev))
    mask = ((rnd((N, 1280), SEED + 3) > -0.8).float() / 0.8)
    logits = net.forward_train(x.to(dev), dropout_mask=mask.to(dev))
    assert logits.shape == (N, 200)
    logits.backward(rnd((N, 200), SEED + 4).to(dev))
    lin = net.classifier[1]
    assert lin.weight.grad is not None and lin.bias.grad is not None and net.features[0][0].weight.grad is not None
    net2 = _train(_net(dev))
    with torch.no_grad():
        feat = net2.features_train_nhwc4(nchw_to_nhwc4(x.to(dev)))
    f, w, b = feat.cpu(), lin.weight.detach().cpu(), lin.bias.detach().cpu()
    want64 = (f.double() * mask.double()) @ w.double().t() + b.double()
    want32 = (f * mask) @ w.t() + b
    spread, err = _rel(want32, want64), _rel(logits.detach(), want64)
    print("logits: err %.2e spread %.2e" % (err, spread))
    assert spread > 0 and err <= SPREAD_FACTOR * spread
