"""Stage-0 training of the local CNN on the MI355X: the batch-statistics walk of adafocus_amd/trunk_train.py against a
float64 CPU restatement of the same network in train mode (tests/stage0_reference.py), the opt-in's surface, and
``train.train_stage0_batch`` against the reference's own step (G21: tests/golden/g21_act_stage0.npz, tools/gen_golden_stage0.py).

Tolerance: G17's rule (tests/test_stage3_gpu.py) -- the error against the float64 result, relative to that quantity's largest entry, is
at most 50x the distance between the same CPU computation in fp32 and in fp64 (both on the same ReLU branches: _case).

The branch at a ReLU whose input is zero to within fp32 rounding is treated as tests/test_trunk_backward_gpu.py treats it (its docstring):
the whole-trunk cases evaluate the float64 gradient ON THE BRANCHES THE DEVICE TOOK, after checking that every unit on the other branch
has a float64 input within 50x the fp32 forward error of its map.  With 4 patches of 64 x 64 layer4 is 2 x 2: 16 rows per column, at
which torch's own fp32 run stays within its bound (checked on the CPU when the cases were fixed).  The fixture of the last test cannot
follow the device's branches; its generator says how its weights were chosen for that."""
import types

import numpy as np
import pytest
import torch

from adafocus_amd import resnet, synth
from adafocus_amd.train import train_stage0_batch
from adafocus_amd.utils import nchw_to_nhwc4
from tests import stage0_reference as R
from tests.helpers import golden, rnd
from tests.trunk_walk_harness import SPREAD_FACTOR, _device_branches, _rel, _run, check_features_and_gradients

pytestmark = pytest.mark.gpu

N, SIZE = 4, 64
# tag -> (arch, temporal shift segments (0 = none; the statistics run over all frames), placement, a (BatchNorm, channel) with gamma = 0)
CASES = {
    "r50": ("resnet50", 0, "blockres", ("layer2.0.bn2", 3)),
    "r101": ("resnet101", 0, "blockres", None),
    "r50_shift": ("resnet50", 2, "blockres", None),
    "r50_block": ("resnet50", 2, "block", None),
}
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _inputs(tag):
    if ("in", tag) not in _CACHE:
        arch, tsm, place, zero = CASES[tag]
        shapes = {k: tuple(v.shape) for k, v in getattr(resnet, arch)().state_dict().items()}
        sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 2100 + len(tag)).items()}
        if zero is not None:        # (a positive beta: the channel's output is the constant beta, and under the ReLU only that passes a gradient)
            sd[zero[0] + ".weight"][zero[1]], sd[zero[0] + ".bias"][zero[1]] = 0.0, 0.5
        _CACHE["in", tag] = (sd, rnd((N, 3, SIZE, SIZE), 2110 + len(tag)), rnd((N, 2048), 2120 + len(tag)))
    return _CACHE["in", tag]


def _reference(tag, dt, masks=None):
    """CPU autograd of the case in `dt`, train mode: (features, {param: grad}, {ReLU: input}, the state after the forward)."""
    arch, tsm, place, _ = CASES[tag]
    sd, x, dfeat = _inputs(tag)
    p = R.cast(sd, dt)
    pre = {}
    feat = R.trunk(p, x.to(dt), resnet.DEPTHS[arch], tsm, 8, place, training=True, pre=pre, masks=masks)
    names = [k for k in p if R.is_trunk_param(k)]
    grads = torch.autograd.grad(feat, [p[k] for k in names], dfeat.to(dt))
    return feat.detach(), dict(zip(names, grads)), pre, {k: v.detach() for k, v in p.items()}


def _case(tag):
    """The CPU reference in both precisions, computed once.  The fp32 run is evaluated on the float64 run's ReLU branches: left to
    itself it takes another branch at one to seven units in three of the four cases, and the spread would then measure that branch
    change (1e-3 ... 1e-1 of a gradient's largest entry) in place of fp32 rounding."""
    if tag not in _CACHE:
        r64 = _reference(tag, torch.float64)
        _CACHE[tag] = {torch.float64: r64, torch.float32: _reference(tag, torch.float32, {k: v > 0 for k, v in r64[2].items()})}
    return _CACHE[tag]


def _net(tag, dev, batch_stats=True, train=True):
    arch, tsm, place, _ = CASES[tag]
    net = getattr(resnet, arch)()
    net.load_state_dict(_inputs(tag)[0], strict=True)
    net = net.train(train).to(dev)
    net.set_math("f32")
    net.tsm_segments, net.tsm_div, net.tsm_place = tsm, 8, place
    net.set_trainable(True)
    if batch_stats is not None:
        net.set_bn_batch_stats(batch_stats)
    return net


@pytest.mark.parametrize("tag", list(CASES))
def test_features_gradients_and_statistics_against_fp64(dev, tag):
    sd, x, dfeat = _inputs(tag)
    ref = _case(tag)
    net = _net(tag, dev)
    feat, grads = _run(net, x, dfeat, dev)
    f64, g64, pre64, s64 = ref[torch.float64]
    f32, g32, pre32, s32 = ref[torch.float32]
    # (a second net from the same state dict: the walk moves running statistics)
    masks, differ = _device_branches(tag, _net(tag, dev), x, dev, pre64, pre32)
    if differ:
        f64, g64, _, _ = _reference(tag, torch.float64, masks)
    check_features_and_gradients(tag, feat, grads, (f32, g32), (f64, g64), CASES[tag][3])
    # the running statistics moved once, as the module in train mode moves them
    stats = []
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
        elif "running" in k:
            assert not torch.equal(v.cpu(), sd[k]), k
            spread, err = _rel(s32[k], s64[k]), _rel(v, s64[k])
            stats.append((err / spread if spread > 0 else float("inf"), k, err, spread))
    stats.sort(reverse=True)
    print("%s: %d running statistics; worst err / spread: %s" % (tag, len(stats), ", ".join("%s %.2e / %.2e" % w[1:] for w in stats[:3])))
    bad = [(k, err, spread) for ratio, k, err, spread in stats if not err <= SPREAD_FACTOR * spread]
    assert not bad, bad[:8]


def test_only_layer4_trainable_stops_the_chain(dev):
    tag = "r50_shift"
    _, x, dfeat = _inputs(tag)
    net = _net(tag, dev)
    f_full, full = _run(net, x, dfeat, dev)
    full = {k: v.clone() for k, v in full.items() if v is not None}
    for k, p in net.named_parameters():
        p.requires_grad_(k.startswith("layer4."))
    f_part, part = _run(net, x, dfeat, dev)
    assert torch.equal(f_part, f_full)             # (batch statistics: the features do not depend on the running statistics that moved)
    for k, g in part.items():
        if k.startswith("layer4."):
            assert torch.equal(g, full[k]), k
        else:
            assert g is None, k


def test_opt_in_off_and_eval_mode_are_the_frozen_walk(dev):
    """With the opt-in off -- never touched, or switched on and off again -- and with the opt-in on but the module in eval mode, the eval
    features and the frozen walk's features and gradients are what a net that never saw the new code gives, bit for bit; off and in
    train mode the walk still refuses."""
    tag = "r50_shift"
    sd, x, dfeat = _inputs(tag)
    x4 = nchw_to_nhwc4(x.to(dev))

    def frozen(net):
        with torch.no_grad():
            engine = net.features_nhwc4(x4).clone()
        feat, grads = _run(net, x, dfeat, dev)
        return engine, feat, grads

    plain = _net(tag, dev, batch_stats=None, train=False)                # a net on which set_bn_batch_stats was never called
    assert plain.bn_batch_stats is False
    toggled = _net(tag, dev, batch_stats=True, train=False)
    toggled.set_bn_batch_stats(False)
    on_eval = _net(tag, dev, batch_stats=True, train=False)
    want = frozen(plain)
    for other in (toggled, on_eval):
        got = frozen(other)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        for k, g in want[2].items():
            assert (g is None and got[2][k] is None) or torch.equal(got[2][k], g), k
        for k, v in other.state_dict().items():
            assert torch.equal(v.cpu(), sd[k]), k                       # nothing moved
    toggled.train()
    with pytest.raises(RuntimeError, match="batch-statistics"):
        toggled.features_train_nhwc4(x4)


def test_eval_engine_sees_the_moved_statistics(dev):
    """Staleness: the eval engine has folded the old running statistics; after a train-mode forward (no optimizer step, no parameter
    version changes) its features are those of a fresh net loaded from the state dict."""
    tag = "r50"
    sd, x, _ = _inputs(tag)
    x4 = nchw_to_nhwc4(x.to(dev))
    net = _net(tag, dev)
    net.eval()
    with torch.no_grad():
        before = net.features_nhwc4(x4).clone()
    net.train()
    with torch.no_grad():
        net.features_train_nhwc4(x4)
    net.eval()
    with torch.no_grad():
        after = net.features_nhwc4(x4).clone()
    fresh = getattr(resnet, CASES[tag][0])()
    fresh.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()}, strict=True)
    fresh = fresh.eval().to(dev)
    fresh.set_math("f32")
    with torch.no_grad():
        assert torch.equal(after, fresh.features_nhwc4(x4))
    assert not torch.equal(after, before)


def test_batch_walk_is_fp32_only(dev):
    tag = "r50"
    net = _net(tag, dev)
    x4 = nchw_to_nhwc4(_inputs(tag)[1].to(dev))
    for mode in ("f16", "split_bf16"):
        net.set_math(mode)
        with pytest.raises(NotImplementedError, match=mode):
            net.features_train_nhwc4(x4)
    bn = net.layer1[0].bn1
    net.set_math("f32")
    bn.momentum = None
    with pytest.raises(NotImplementedError, match="momentum"):
        net.features_train_nhwc4(x4)


# ---- train_stage0_batch against the reference's step (G21) ------------------------------------------------------------------------------
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
    m.focuser.net.set_math("f32")
    return m.to(dev)


def _check(tag, got, ref, spread):
    ref = np.asarray(ref, dtype=np.float64)
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    return np.abs(got.reshape(ref.shape) - ref).max() / np.abs(ref).max(), float(spread), tag


def test_backbone_train_mode_refuses_the_glancer(dev):
    m = _model(golden("g21_act_stage0"), dev)
    with pytest.raises(NotImplementedError, match="MobileNetV2"):
        m.backbone_train_mode(glancer=True)


def test_train_stage0_batch_matches_the_reference_g21(dev):
    g = golden("g21_act_stage0")
    b, t, s, c = (int(v) for v in g["dims"])
    lr, momentum, wd = (float(v) for v in g["sgd"])
    images = torch.from_numpy(synth.synth_frames(b, t, s, seed=int(g["seeds"][1]))).to(dev)
    target = torch.from_numpy(g["target"]).to(dev)
    twin = _model(g, dev)
    twin.backbone_train_mode()
    with torch.no_grad():
        frames = twin.focuser.net.forward_train(images.view(b * t, 3, s, s))
    m = _model(g, dev)
    m.backbone_train_mode()
    net = m.focuser.net
    opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=momentum, weight_decay=wd)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    pred, loss = train_stage0_batch(m, images, target, _args(g), opt)
    assert not pred.requires_grad and not loss.requires_grad
    for k, p in m.named_parameters():
        if not k.startswith("focuser.net."):
            assert p.grad is None, k
    params = m.state_dict(keep_vars=True)
    rows = [_check("logits", frames, g["logits"], g["spread_logits"][0]), _check("pred", pred, g["pred"], g["spread_pred"][0]),
            _check("loss", loss.reshape(1), g["loss"], g["spread_loss"][0]),
            _check("fc.weight", net.fc.weight.grad, g["fc_weight"], g["spread_fc_weight"][0]),
            _check("fc.bias", net.fc.bias.grad, g["fc_bias"], g["spread_fc_bias"][0])]
    off = 0
    for i, n in enumerate(g["names_bn"].tolist()):
        grad = params[n].grad
        assert grad is not None and torch.isfinite(grad).all(), n
        rows.append(_check(n, grad, g["bn"][off:off + grad.numel()], g["spread_bn"][i]))
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
    zero_name, ch = str(g["zero_gamma_name"][0]), int(g["zero_gamma_channel"][0])
    assert params[zero_name].grad[ch].item() != 0.0
    # the eval forward after the step: the new weights AND the moved running statistics reach the engine
    m.eval()
    with torch.no_grad():
        after = net(images.view(b * t, 3, s, s))
    rows.append(_check("logits_after", after, g["logits_after"], g["spread_logits_after"][0]))
    rows.sort(key=lambda r: -(r[0] / r[1]))
    print("G21: %d quantities; worst err / spread: %s" % (len(rows), ", ".join("%s %.2e / %.2e" % (r[2], r[0], r[1]) for r in rows[:5])))
    bad = [r for r in rows if not r[0] <= SPREAD_FACTOR * r[1]]
    assert not bad, bad[:8]
