#!/usr/bin/env python3
"""Stage-0 fixture of the ActivityNet tree: one training step of the REAL reference model (ACT/models/gfv_net.py, ACT/models/resnet.py) as
ACT/main_dist.py:544-548 runs it for the focuser's ResNet (pretrain_glancer=False, no AMP), imported exactly like tools/gen_golden.py does
(its shims; no reference source is copied).  Writes tests/golden/g21_act_stage0.npz.  Runs on the CPU.

Configuration: gen_golden.act_args(num_segments=2, num_classes=10), B = 2, T = 2, 64 x 64 frames (synth.synth_frames, seed SEED_X), weights
by gen_golden.load_synth: neither is stored.  One BatchNorm gamma (layer2.0.bn2, channel 3) is set to exactly 0.  The model is in the
mode of the reference's train_mode for train_stage 0 (everything in train mode); the optimizer is main_dist.py:163-170's SGD over the
glancer's, the focuser's and the classifier's parameters (only the focuser's ResNet gets a gradient in this branch).

The weight seed.  The gradient of a ReLU network is piecewise constant in its ReLU branches, and on the 2 x 2 and 4 x 4 maps of layer4
and layer3 one unit on the other branch moves the gradients in front of it by a few per cent of their largest entry -- thousands of
times the fp32-vs-fp64 spread (tests/test_trunk_backward_gpu.py's docstring; measured for this step too).  Every set of weights has
units in those maps whose float64 ReLU input is below the largest fp32 forward error of their map (about 10^-6), so no seed is safe
against every fp32 implementation, and a fixture cannot follow the branches a device takes.  The seed is therefore CHOSEN: of SEEDS_W,
among the seeds whose float32 CPU run takes the float64 run's branch at every unit (so that the stored spreads hold no branch change),
the one whose thinnest unit -- |float64 ReLU input| over the fp32-vs-fp64 error of its map, over the maps of 16 pixels or fewer -- is
thickest.  That ratio is stored (`relu_margin`).

Stored (the float64 run's results as float32): the per-frame logits (B*T, C), the prediction (B, C), the loss, fc's gradients in full,
every BatchNorm weight / bias gradient in full, every conv weight gradient as G17's two projections  G v  (v of seed 174)  and  u^T G
(u of seed 184), the running statistics of every BatchNorm after the step, num_batches_tracked, and the per-frame logits of an
eval-mode forward after the SGD step (lr, momentum, weight_decay recorded).  Vectors of many parameters are concatenated in the order of
`names_bn` / `names_conv` / `names_stat` (the reference's state-dict names).  `spread_*`: the same step in float32, as a relative
difference per quantity (per parameter for the concatenated ones).

Usage:  python tools/gen_golden_stage0.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_golden_depths import save_stable  # noqa: E402

from adafocus_amd import synth  # noqa: E402

SEEDS_W, SEED_X = range(2151, 2167), 21
B, T, S, C = 2, 2, 64, 10
LR, MOMENTUM, WEIGHT_DECAY = 0.01, 0.9, 1e-4
TARGET = [3, 7]
ZERO_GAMMA = ("focuser.net.layer2.0.bn2.weight", 3)
PREFIX = "focuser.net."
SMALL = 16              # pixels


def import_reference():
    GG._enter_tree(GG.ACT)
    import models.gfv_net as G
    _rn, _mb = G.resnet50, G.mobilenet_v2
    G.resnet50 = lambda pretrained=False, **k: _rn(pretrained=False, **k)
    G.mobilenet_v2 = lambda pretrained=False, **k: _mb(pretrained=False, **k)
    return G


def build(G, args, seed, dtype):
    model = G.GFV(args)
    GG.load_synth(model, seed)
    with torch.no_grad():
        dict(model.named_parameters())[ZERO_GAMMA[0]][ZERO_GAMMA[1]] = 0.0
    return model.to(dtype)


def project(g, dtype):
    g = g.flatten(1)
    v = torch.from_numpy(GG.rnd((g.shape[1],), 174)).to(dtype)
    u = torch.from_numpy(GG.rnd((g.shape[0],), 184)).to(dtype)
    return g @ v, u @ g


def step(G, args, seed, dtype):
    """One stage-0 step of the reference in `dtype`: ({quantity: array}, {concatenated quantity: [array per parameter]}, the ReLU inputs
    of the focuser's ResNet in call order, names)."""
    torch.set_default_dtype(dtype)
    try:
        model = build(G, args, seed, dtype)
        args.train_stage = 0
        model.train_mode(args)
        opt = torch.optim.SGD([{"params": model.glancer.parameters()}, {"params": model.focuser.parameters()},
                               {"params": model.classifier.parameters()}], lr=LR, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
        images = torch.from_numpy(synth.synth_frames(B, T, S, seed=SEED_X)).to(dtype)
        target = torch.tensor(TARGET)
        pre = []
        hooks = [m.register_forward_pre_hook(lambda mod, inp: pre.append(inp[0].detach().clone()))
                 for m in model.focuser.net.modules() if isinstance(m, torch.nn.ReLU)]
        opt.zero_grad()
        frames = model(input=images, scan=None, glancer=False, backbone_pred=True, one_step=False)      # main_dist.py:544-548
        pred = frames.mean(1, keepdim=True).squeeze(1)
        loss = torch.nn.functional.cross_entropy(pred, target)
        loss.backward()
        for h in hooks:
            h.remove()
        params = dict(model.named_parameters())
        mods = dict(model.named_modules())
        names_bn = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.BatchNorm2d)]
        names_conv = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.Conv2d)]
        assert len(names_bn) + len(names_conv) + 2 == sum(1 for n in params if n.startswith(PREFIX))
        for n, p in params.items():          # nothing but the focuser's ResNet learns in this branch
            if not n.startswith(PREFIX):
                assert p.grad is None or not p.grad.any(), n
        out = {"logits": frames.detach().reshape(B * T, -1), "pred": pred.detach(), "loss": loss.detach().reshape(1),
               "fc_weight": params[PREFIX + "fc.weight"].grad, "fc_bias": params[PREFIX + "fc.bias"].grad}
        per = {"bn": [params[n].grad.reshape(-1) for n in names_bn], "conv_Gv": [], "conv_uG": []}
        for n in names_conv:
            gv, ug = project(params[n].grad, dtype)
            per["conv_Gv"].append(gv)
            per["conv_uG"].append(ug)
        opt.step()
        sd = model.state_dict()
        names_stat = [k for k in sd if k.startswith(PREFIX) and k.endswith(("running_mean", "running_var"))]
        per["stat"] = [sd[k].reshape(-1) for k in names_stat]
        tracked = {int(sd[k]) for k in sd if k.startswith(PREFIX) and k.endswith("num_batches_tracked")}
        assert tracked == {1}, tracked
        model.eval()
        with torch.no_grad():
            after = model(input=images, scan=None, glancer=False, backbone_pred=True, one_step=False)
        out["logits_after"] = after.reshape(B * T, -1)
        out = {k: v.detach().double().numpy() for k, v in out.items()}
        per = {k: [t.detach().double().numpy() for t in v] for k, v in per.items()}
        return out, per, pre, (names_bn, names_conv, names_stat)
    finally:
        torch.set_default_dtype(torch.float32)


def thinnest(pre32, pre64):
    """The smallest (|float64 ReLU input| / fp32-vs-fp64 error of its map) over the maps of SMALL pixels or fewer, and the number of units
    whose sign differs between the two runs over all maps."""
    worst, flips = float("inf"), 0
    for a, b in zip(pre32, pre64):
        flips += int(((a > 0) != (b > 0)).sum())
        if b.shape[2] * b.shape[3] <= SMALL:
            err = (a.double() - b).abs().max().item()
            worst = min(worst, b.abs().min().item() / err)
    return worst, flips


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG._install_shims()
    G = import_reference()
    args = GG.act_args(num_segments=T, num_classes=C)
    best = None
    for s in SEEDS_W:
        r32, p32, pre32, _ = step(G, args, s, torch.float32)
        r64, p64, pre64, names = step(G, args, s, torch.float64)
        margin, flips = thinnest(pre32, pre64)
        print("  weight seed %d: thinnest small-map ReLU input %.3f x its map's fp32 error, %d units differ between fp32 and fp64" % (s, margin, flips))
        if flips == 0 and (best is None or margin > best[0]):
            best = (margin, s, r32, p32, r64, p64, names)
    assert best is not None, "no weight seed whose fp32 run keeps the fp64 branches"
    margin, seed, r32, p32, r64, p64, names = best
    print("  chosen: weight seed %d (margin %.3f)" % (seed, margin))
    arrays = {"seeds": np.array([seed, SEED_X]), "dims": np.array([B, T, S, C]), "target": np.array(TARGET), "sgd": np.array([LR, MOMENTUM, WEIGHT_DECAY]),
              "zero_gamma_channel": np.array([ZERO_GAMMA[1]]), "zero_gamma_name": np.array([ZERO_GAMMA[0]]), "relu_margin": np.array([margin]),
              "names_bn": np.array(names[0]), "names_conv": np.array(names[1]), "names_stat": np.array(names[2])}
    for k in r64:
        arrays[k] = r64[k].astype(np.float32)
        arrays["spread_" + k] = np.array([rel(r32[k], r64[k])])
        print("  %-14s max %.3e  fp32-vs-fp64 %.2e" % (k, np.abs(r64[k]).max(), arrays["spread_" + k][0]))
    for k in p64:
        arrays[k] = np.concatenate(p64[k]).astype(np.float32)
        sp = np.array([rel(a, b) for a, b in zip(p32[k], p64[k])])
        arrays["spread_" + k] = sp
        print("  %-14s %d parameters, fp32-vs-fp64 min %.2e median %.2e max %.2e" % (k, len(sp), sp.min(), np.median(sp), sp.max()))
        assert np.isfinite(sp).all() and (sp > 0).all(), k
    save_stable("g21_act_stage0", **arrays)


if __name__ == "__main__":
    main()
