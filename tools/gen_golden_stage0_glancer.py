#!/usr/bin/env python3
"""Stage-0 fixture of the ActivityNet tree for the GLANCER: one training step of the REAL reference model (ACT/models/gfv_net.py,
ACT/models/mobilenet.py) as ACT/main_dist.py:544-548 runs it with pretrain_glancer=True (no AMP), imported exactly like
tools/gen_golden.py does (its shims; no reference source is copied).  Writes tests/golden/g23_act_stage0_glancer.npz.  Runs on the CPU.
Modelled on tools/gen_golden_stage0.py (G21).

Configuration: gen_golden.act_args(num_segments=2, num_classes=10), B = 2, T = 2, 64 x 64 frames (synth.synth_frames, seed SEED_X), weights
by gen_golden.load_synth: neither is stored.  One BatchNorm gamma (features.3's depthwise BatchNorm, channel 5) is set to exactly 0.  The
model is in the mode of the reference's train_mode for train_stage 0 (everything in train mode); the optimizer is main_dist.py:163-170's
SGD over the glancer's, the focuser's and the classifier's parameters (only the glancer's MobileNetV2 gets a gradient in this branch).

The dropout.  The glancer's classifier is Dropout(0.2) -> Linear.  The float64 run draws its mask as the reference does (torch's CPU
generator, seeded with SEED_DROP in front of the step); a forward hook on the Dropout records the multipliers (0 or 1.25) and the fp32 run
is given the same ones.  The mask is stored (`dropout_mask`, uint8: 1 = kept): the test injects it.

The weight seed is chosen by G21's rule, extended to both kinks of ReLU6: of SEEDS_W, among the seeds whose float32 CPU run takes the
float64 run's branch (below 0, between, above 6) at every unit, the one whose thinnest unit -- the distance of its float64 ReLU6 input
from the nearer kink over the fp32-vs-fp64 error of its map, over the maps of 16 pixels or fewer -- is thickest (`relu_margin`).

The bias of a project BatchNorm has a gradient of exactly zero: everything that reads a block's output is a 1x1 convolution followed by
a BatchNorm on batch statistics (through the identity chains too), which removes a per-channel constant.  What either run computes for it
is the rounding residue of a sum that cancels, so "relative to its largest entry" would compare noise with noise.  Such a gradient (its
largest float64 entry below ZERO_SHARE of the same BatchNorm's weight gradient's, a sum of the same upstream gradient) is measured on the
weight gradient's scale: `scale_bn` holds the scale of every BatchNorm gradient, its own largest entry for all the others.

Stored (the float64 run's results as float32): the per-frame logits (B*T, C), the prediction (B, C), the loss, the classifier's gradients
in full, every BatchNorm weight / bias gradient in full, every conv weight gradient as G17's two projections  G v  (v of seed 174)  and
u^T G  (u of seed 184), the running statistics of every BatchNorm after the step, and the per-frame logits of an eval-mode forward after
the SGD step (lr, momentum, weight_decay recorded).  Vectors of many parameters are concatenated in the order of `names_bn` /
`names_conv` / `names_stat` (the reference's state-dict names).  `spread_*`: the same step in float32, as a relative difference per
quantity (per parameter for the concatenated ones).

Usage:  python tools/gen_golden_stage0_glancer.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_golden_depths import save_stable  # noqa: E402
from gen_golden_stage0 import import_reference, project, rel  # noqa: E402

from adafocus_amd import synth  # noqa: E402

SEEDS_W, SEED_X, SEED_DROP = range(2351, 2367), 23, 2323
B, T, S, C = 2, 2, 64, 10
LR, MOMENTUM, WEIGHT_DECAY = 0.01, 0.9, 1e-4
TARGET = [3, 7]
ZERO_GAMMA = ("glancer.net.features.3.conv.1.1.weight", 5)
PREFIX = "glancer.net."
SMALL = 16              # pixels
KEEP = 0.8              # 1 - the dropout's p
ZERO_SHARE = 1e-6       # a BatchNorm bias gradient below this share of its weight gradient is a sum that cancels exactly


def build(G, args, seed, dtype):
    model = G.GFV(args)
    GG.load_synth(model, seed)
    with torch.no_grad():
        dict(model.named_parameters())[ZERO_GAMMA[0]][ZERO_GAMMA[1]] = 0.0
    return model.to(dtype)


def step(G, args, seed, dtype, mask=None):
    """One stage-0 step of the reference's glancer in `dtype` (mask: the dropout multipliers to use instead of a draw): ({quantity:
    array}, {concatenated quantity: [array per parameter]}, the ReLU6 inputs of the MobileNetV2 in call order, names, the mask)."""
    torch.set_default_dtype(dtype)
    try:
        model = build(G, args, seed, dtype)
        args.train_stage = 0
        model.train_mode(args)
        opt = torch.optim.SGD([{"params": model.glancer.parameters()}, {"params": model.focuser.parameters()},
                               {"params": model.classifier.parameters()}], lr=LR, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
        images = torch.from_numpy(synth.synth_frames(B, T, S, seed=SEED_X)).to(dtype)
        target = torch.tensor(TARGET)
        pre, drawn = [], []
        hooks = [m.register_forward_pre_hook(lambda mod, inp: pre.append(inp[0].detach().clone()))
                 for m in model.glancer.net.features.modules() if isinstance(m, torch.nn.ReLU6)]
        drop = model.glancer.net.classifier[0]
        assert isinstance(drop, torch.nn.Dropout) and abs(drop.p - (1 - KEEP)) < 1e-12

        def on_dropout(mod, inp, out):
            if mask is not None:
                return inp[0] * mask.to(inp[0].dtype)
            # a feature that is exactly 0 tells nothing about its multiplier, and its multiplier moves nothing
            drawn.append(torch.where(inp[0] != 0, (out != 0).to(out.dtype) / KEEP, torch.full_like(out, 1 / KEEP)).detach())
            return None
        hooks.append(drop.register_forward_hook(on_dropout))
        torch.manual_seed(SEED_DROP)
        opt.zero_grad()
        frames = model(input=images, scan=None, glancer=True, backbone_pred=True, one_step=False)      # main_dist.py:544-548
        pred = frames.mean(1, keepdim=True).squeeze(1)
        loss = torch.nn.functional.cross_entropy(pred, target)
        loss.backward()
        for h in hooks:
            h.remove()
        used = mask if mask is not None else drawn[0]
        params = dict(model.named_parameters())
        mods = dict(model.named_modules())
        names_bn = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.BatchNorm2d)]
        names_conv = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.Conv2d)]
        assert len(names_bn) + len(names_conv) + 2 == sum(1 for n in params if n.startswith(PREFIX))
        for n, p in params.items():          # nothing but the glancer's MobileNetV2 learns in this branch
            if not n.startswith(PREFIX):
                assert p.grad is None or not p.grad.any(), n
        out = {"logits": frames.detach().reshape(B * T, -1), "pred": pred.detach(), "loss": loss.detach().reshape(1),
               "cls_weight": params[PREFIX + "classifier.1.weight"].grad, "cls_bias": params[PREFIX + "classifier.1.bias"].grad}
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
            after = model(input=images, scan=None, glancer=True, backbone_pred=True, one_step=False)
        out["logits_after"] = after.reshape(B * T, -1)
        out = {k: v.detach().double().numpy() for k, v in out.items()}
        per = {k: [t.detach().double().numpy() for t in v] for k, v in per.items()}
        return out, per, pre, (names_bn, names_conv, names_stat), used.double()
    finally:
        torch.set_default_dtype(torch.float32)


def branch(z):
    return (z > 0).to(torch.int8) + (z >= 6).to(torch.int8)          # 0 below, 1 between, 2 above


def thinnest(pre32, pre64):
    """The smallest (distance of the float64 ReLU6 input from the nearer kink / fp32-vs-fp64 error of its map) over the maps of SMALL
    pixels or fewer, and the number of units whose branch differs between the two runs over all maps."""
    worst, flips = float("inf"), 0
    for a, b in zip(pre32, pre64):
        flips += int((branch(a) != branch(b)).sum())
        if b.shape[2] * b.shape[3] <= SMALL:
            err = (a.double() - b).abs().max().item()
            if err > 0:          # (the gamma = 0 channel aside, a map both runs get bit for bit has no thin unit)
                worst = min(worst, torch.minimum(b.abs(), (b - 6).abs()).min().item() / err)
    return worst, flips


def main():
    torch.set_num_threads(8)
    GG._install_shims()
    G = import_reference()
    args = GG.act_args(num_segments=T, num_classes=C)
    best = None
    for s in SEEDS_W:
        r64, p64, pre64, names, mask = step(G, args, s, torch.float64)
        r32, p32, pre32, _, _ = step(G, args, s, torch.float32, mask)
        margin, flips = thinnest(pre32, pre64)
        print("  weight seed %d: thinnest small-map ReLU6 input %.3f x its map's fp32 error from a kink, %d units differ between fp32 and fp64"
              % (s, margin, flips))
        if flips == 0 and (best is None or margin > best[0]):
            best = (margin, s, r32, p32, r64, p64, names, mask)
    assert best is not None, "no weight seed whose fp32 run keeps the fp64 branches"
    margin, seed, r32, p32, r64, p64, names, mask = best
    print("  chosen: weight seed %d (margin %.3f); dropout keeps %d of %d" % (seed, margin, int((mask > 0).sum()), mask.numel()))
    arrays = {"seeds": np.array([seed, SEED_X, SEED_DROP]), "dims": np.array([B, T, S, C]), "target": np.array(TARGET),
              "sgd": np.array([LR, MOMENTUM, WEIGHT_DECAY]), "zero_gamma_channel": np.array([ZERO_GAMMA[1]]),
              "zero_gamma_name": np.array([ZERO_GAMMA[0]]), "relu_margin": np.array([margin]), "dropout_keep": np.array([KEEP]),
              "dropout_mask": (mask > 0).numpy().astype(np.uint8),
              "names_bn": np.array(names[0]), "names_conv": np.array(names[1]), "names_stat": np.array(names[2])}
    for k in r64:
        arrays[k] = r64[k].astype(np.float32)
        arrays["spread_" + k] = np.array([rel(r32[k], r64[k])])
        print("  %-14s max %.3e  fp32-vs-fp64 %.2e" % (k, np.abs(r64[k]).max(), arrays["spread_" + k][0]))
    own = {n: float(np.abs(v).max()) for n, v in zip(names[0], p64["bn"])}
    scale_bn = []
    for n in names[0]:
        w = own[n[:-len("bias")] + "weight"] if n.endswith(".bias") else 0.0
        scale_bn.append(w if own[n] < ZERO_SHARE * w else own[n])
    arrays["scale_bn"] = np.array(scale_bn)
    print("  %d BatchNorm bias gradients cancel exactly (largest stored residue %.1e)" % (
        sum(1 for n, sc in zip(names[0], scale_bn) if sc != own[n]), max([own[n] for n, sc in zip(names[0], scale_bn) if sc != own[n]] + [0.0])))
    for k in p64:
        arrays[k] = np.concatenate(p64[k]).astype(np.float32)
        if k == "bn":
            sp = np.array([float(np.abs(a - b).max() / sc) for a, b, sc in zip(p32[k], p64[k], scale_bn)])
        else:
            sp = np.array([rel(a, b) for a, b in zip(p32[k], p64[k])])
        arrays["spread_" + k] = sp
        print("  %-14s %d parameters, fp32-vs-fp64 min %.2e median %.2e max %.2e" % (k, len(sp), sp.min(), np.median(sp), sp.max()))
        assert np.isfinite(sp).all() and (sp > 0).all(), k
    save_stable("g23_act_stage0_glancer", **arrays)


if __name__ == "__main__":
    main()
