"""The device side of the two tests of the trunk's training walk (tests/test_trunk_backward_gpu.py: frozen BatchNorm statistics;
tests/test_stage0_gpu.py: batch statistics): one step on the device, the ReLU branches the device took, and the comparison of every
gradient with the float64 reference under G17's rule.  The CPU restatements stay with their tests: each is the yardstick its bounds were
measured against."""
import torch

from adafocus_amd import trunk_train
from adafocus_amd.utils import nchw_to_nhwc4

SPREAD_FACTOR = 50


def _run(net, x, dfeat, dev):
    net.zero_grad(set_to_none=True)
    net.set_trainable(True)
    feat = net.features_train_nhwc4(nchw_to_nhwc4(x.to(dev)))
    feat.backward(dfeat.to(dev))
    return feat.detach(), {k: v.grad for k, v in net.named_parameters()}


def _rel(got, ref64):
    return ((got.double().cpu() - ref64).abs().max() / ref64.abs().max()).item()


def _device_branches(tag, net, x, dev, pre64, pre32):
    """The ReLU masks of the device's walk of `net` (in the form its mode selects; the batch-statistics form moves its running statistics),
    checked against the fp64 forward's ReLU inputs pre64: ({ReLU name: bool NCHW map}, units that differ).  A unit may differ only where
    the fp64 pre-activation is within SPREAD_FACTOR x the fp32-vs-fp64 forward error of its map (pre32: the fp32 forward's)."""
    with torch.no_grad():
        walk = trunk_train.walk_forward(net, nchw_to_nhwc4(x.to(dev)))
    outs = {"stem": walk.stem_out}
    for (c1, _, _, _, _), (_, z1, z2, y) in zip(walk.blocks, walk.acts):
        q = c1.name.rsplit(".", 1)[0]
        outs[q + ".z1"], outs[q + ".z2"], outs[q + ".y"] = z1, z2, y
    assert set(outs) == set(pre64)
    masks, differ = {}, 0
    for k, z64 in pre64.items():
        masks[k] = outs[k].permute(0, 3, 1, 2).cpu() > 0
        d = masks[k] != (z64 > 0)
        if d.any():
            err = (pre32[k].double() - z64).abs().max().item()
            worst = z64[d].abs().max().item()
            print("%s %s: %d unit(s) on the other branch, |fp64 input| <= %.2e, fp32 forward error of the map %.2e" % (tag, k, int(d.sum()), worst, err))
            assert worst <= SPREAD_FACTOR * err, (tag, k, worst, err)
            differ += int(d.sum())
    return masks, differ


def check_features_and_gradients(tag, feat, grads, ref32, ref64, zero):
    """The features and every gradient of the device against ref64 = (features, {param: grad}) in fp64, within SPREAD_FACTOR x the
    distance of ref32 from it; fc takes no gradient; zero = (BatchNorm, channel) whose gamma is exactly 0, or None."""
    (f32, g32), (f64, g64) = ref32, ref64
    spread, err = _rel(f32, f64), _rel(feat, f64)
    assert err <= SPREAD_FACTOR * spread, ("features", err, spread)
    worst = []
    for k, r64 in g64.items():
        g = grads[k]
        assert g is not None and torch.isfinite(g).all(), k
        assert r64.abs().max() > 0, k
        spread, err = _rel(g32[k], r64), _rel(g, r64)
        worst.append((err / spread if spread > 0 else float("inf"), k, err, spread))
    worst.sort(reverse=True)
    print("%s: %d gradients; worst err / spread: %s" % (tag, len(worst), ", ".join("%s %.2e / %.2e" % w[1:] for w in worst[:4])))
    assert grads["fc.weight"] is None and grads["fc.bias"] is None
    bad = [(k, err, spread) for ratio, k, err, spread in worst if not err <= SPREAD_FACTOR * spread]
    assert not bad, bad[:8]
    if zero is not None:
        assert grads[zero[0] + ".weight"][zero[1]].item() != 0.0        # the gamma = 0 channel still gets its dgamma
        assert not grads[zero[0].replace("bn", "conv") + ".weight"][zero[1]].any()      # and passes no gradient to its filter
