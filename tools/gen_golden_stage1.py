#!/usr/bin/env python3
"""Stage-1 fixture of the ActivityNet tree: one training step of the REAL reference model (ACT/models/gfv_net.py:135-150 in the mode of its
train_mode for train_stage 1) as ACT/main_dist.py:473-493 runs it, imported exactly like tools/gen_golden.py does (its shims; no
reference source is copied).  Writes tests/golden/g22_act_stage1_p0.npz (dropout 0) and g22_act_stage1_mask.npz (dropout 0.5 with the mask
observed on the reference's own nn.Dropout call under torch.manual_seed(SEED_M), as G20 does it).  Runs on the CPU.

The call form.  The reference's non-AMP call (main_dist.py:486) omits `training=`, while gfv_net.py:146 reads kwargs["training"]: that
branch raises a KeyError as written.  What is run here is the AMP branch's call (:477, training=True) with the loss of :479, without
autocast and the scaler.

Configuration: gen_golden.act_args(random_patch=True, consensus='gru', hidden_dim=1024, num_segments=2, num_classes=10, input_size=96,
patch_size=64, glance_size=64), B = 2, T = 2, 96 x 96 frames (synth.synth_frames, seed SEED_X), the scan frames by
F.interpolate(images, (64, 64)) as main_dist.py:469 makes them, weights by gen_golden.load_synth: none of them stored.  Four 64 x 64
patches make layer4 2 x 2: 16 rows per BatchNorm column, G21's choice.  np.random is seeded (SEED_C) in front of the step; the origins it
then draws (y then x, frame by frame: utils.py:31-32) are stored as `origins` and checked against the patches the local CNN received.  The
optimizer is main_dist.py:172-177's SGD over the focuser's and the classifier's parameters.

The weight seed is chosen as G21's is, for the reason tools/gen_golden_stage0.py gives: of SEEDS_W, among the seeds whose float32 run
takes the float64 run's branch at every ReLU of the local CNN, the one whose thinnest small-map unit is thickest (`relu_margin`).  The
ReLU inputs do not depend on the dropout, so one choice serves both cases.

Asserted here: no glancer parameter has a gradient, no glancer buffer moves, focuser.net.fc has no gradient.

Stored (the float64 run's results as float32): logits (B*T, C), last (B, C), loss, the gradients of classifier.fc and of the GRU biases
in full, of the GRU weights and of every conv weight as G17's two projections, of every BatchNorm weight / bias in full, the running
statistics of the local CNN after the step, and the eval-mode stage-1-form logits after the SGD step on the same crops (`logits_after`;
lr, momentum, weight_decay in `sgd`).  `spread_*`: the same step in float32, as a relative difference per quantity (per parameter for the
concatenated ones).

Usage:  python tools/gen_golden_stage1.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_golden_depths import save_stable  # noqa: E402
from gen_golden_stage0 import import_reference, project, rel, thinnest  # noqa: E402
from gen_golden_stage3_sth import FixedMask, ObservedDropout  # noqa: E402

from adafocus_amd import synth  # noqa: E402

SEEDS_W, SEED_X, SEED_C, SEED_M = range(2251, 2267), 22, 221, 222
B, T, S, P, GLANCE, C, HIDDEN = 2, 2, 96, 64, 64, 10, 1024
LR, MOMENTUM, WEIGHT_DECAY = 0.01, 0.9, 1e-4
TARGET = [3, 7]
PREFIX = "focuser.net."


def drawn_origins():
    """The (y, x) origins np.random yields after seed SEED_C, frame by frame (utils.py:31-32)."""
    np.random.seed(SEED_C)
    return np.array([[np.random.randint(0, S - P), np.random.randint(0, S - P)] for _ in range(B * T)], dtype=np.int64)


def step(G, seed, dtype, p, mask=None):
    """One stage-1 step of the reference in `dtype` with dropout p (mask: fixed multipliers, else the module's own draw, observed):
    ({quantity: array}, {concatenated quantity: [array per parameter]}, the ReLU inputs of the focuser's ResNet in call order, names,
    the dropout multipliers)."""
    torch.set_default_dtype(dtype)
    try:
        args = GG.act_args(random_patch=True, consensus="gru", hidden_dim=HIDDEN, num_segments=T, num_classes=C, input_size=S, patch_size=P,
                           glance_size=GLANCE, dropout=p, batch_size=B)
        model = G.GFV(args)
        GG.load_synth(model, seed)
        model = model.to(dtype)
        if p > 0:
            model.classifier.dropout = ObservedDropout(p) if mask is None else FixedMask(mask)
        args.train_stage = 1
        model.train_mode(args)
        opt = torch.optim.SGD([{"params": model.focuser.parameters()}, {"params": model.classifier.parameters()}], lr=LR, momentum=MOMENTUM,
                              weight_decay=WEIGHT_DECAY)                                              # main_dist.py:172-177
        images = torch.from_numpy(synth.synth_frames(B, T, S, seed=SEED_X)).to(dtype)
        target = torch.tensor(TARGET)
        scan = torch.nn.functional.interpolate(images, (GLANCE, GLANCE))                               # main_dist.py:469
        pre, patches = [], []
        hooks = [m.register_forward_pre_hook(lambda mod, inp: pre.append(inp[0].detach().clone()))
                 for m in model.focuser.net.modules() if isinstance(m, torch.nn.ReLU)]
        hooks.append(model.focuser.net.conv1.register_forward_pre_hook(lambda mod, inp: patches.append(inp[0].detach().clone())))
        glancer_before = {k: v.clone() for k, v in model.glancer.state_dict().items()}
        origins = drawn_origins()
        np.random.seed(SEED_C)
        torch.manual_seed(SEED_M)
        opt.zero_grad()
        output, last = model(input=images, scan=scan, training=True, backbone_pred=False, one_step=False)   # main_dist.py:477
        loss = torch.nn.functional.cross_entropy(output, target.view(B, -1).expand(B, T).reshape(-1))        # main_dist.py:479
        loss.backward()
        for h in hooks:
            h.remove()
        frames = images.view(B * T, 3, S, S)
        for i, (y, x) in enumerate(origins):
            assert torch.equal(patches[0][i], frames[i, :, y:y + P, x:x + P]), i
        if p > 0 and mask is None:
            mask = model.classifier.dropout.seen.clone()
        params = dict(model.named_parameters())
        mods = dict(model.named_modules())
        for n, q in params.items():
            if n.startswith("glancer.") or n.startswith(PREFIX + "fc."):
                assert q.grad is None, n
        for k, v in model.glancer.state_dict().items():
            assert torch.equal(v, glancer_before[k]), k
        names_bn = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.BatchNorm2d)]
        names_conv = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.Conv2d)]
        assert len(names_bn) + len(names_conv) + 2 == sum(1 for n in params if n.startswith(PREFIX))
        out = {"logits": output.detach(), "last": last.detach(), "loss": loss.detach().reshape(1),
               "fc_weight": params["classifier.fc.weight"].grad, "fc_bias": params["classifier.fc.bias"].grad,
               "gru_bias_ih": params["classifier.gru.bias_ih_l0"].grad, "gru_bias_hh": params["classifier.gru.bias_hh_l0"].grad}
        for tag in ("ih", "hh"):
            out["gru_w_%s_Gv" % tag], out["gru_w_%s_uG" % tag] = project(params["classifier.gru.weight_%s_l0" % tag].grad, dtype)
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
        np.random.seed(SEED_C)                       # the same crops
        with torch.no_grad():
            after, _ = model(input=images, scan=scan, training=False, backbone_pred=False, one_step=False)
        out["logits_after"] = after
        out = {k: v.detach().double().numpy() for k, v in out.items()}
        per = {k: [t.detach().double().numpy() for t in v] for k, v in per.items()}
        return out, per, pre, (names_bn, names_conv, names_stat), mask
    finally:
        torch.set_default_dtype(torch.float32)


def write(name, seed, margin, p, mask, r32, p32, r64, p64, names):
    arrays = {"seeds": np.array([seed, SEED_X, SEED_C, SEED_M]), "dims": np.array([B, T, S, P, GLANCE, C, HIDDEN]), "target": np.array(TARGET),
              "sgd": np.array([LR, MOMENTUM, WEIGHT_DECAY]), "dropout": np.array([p]), "origins": drawn_origins(),
              "relu_margin": np.array([margin]), "names_bn": np.array(names[0]), "names_conv": np.array(names[1]),
              "names_stat": np.array(names[2])}
    if mask is not None:
        arrays["mask"] = mask.numpy().astype(np.float32)
    for k in r64:
        arrays[k] = r64[k].astype(np.float32)
        arrays["spread_" + k] = np.array([rel(r32[k], r64[k])])
        print("  %-14s max %.3e  fp32-vs-fp64 %.2e" % (k, np.abs(r64[k]).max(), arrays["spread_" + k][0]))
        assert np.isfinite(arrays["spread_" + k]).all() and arrays["spread_" + k][0] > 0, k
    for k in p64:
        arrays[k] = np.concatenate(p64[k]).astype(np.float32)
        sp = np.array([rel(a, b) for a, b in zip(p32[k], p64[k])])
        arrays["spread_" + k] = sp
        print("  %-14s %d parameters, fp32-vs-fp64 min %.2e median %.2e max %.2e" % (k, len(sp), sp.min(), np.median(sp), sp.max()))
        assert np.isfinite(sp).all() and (sp > 0).all(), k
    save_stable(name, **arrays)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG._install_shims()
    G = import_reference()
    best = None
    for s in SEEDS_W:
        r32, p32, pre32, _, _ = step(G, s, torch.float32, 0.0)
        r64, p64, pre64, names, _ = step(G, s, torch.float64, 0.0)
        margin, flips = thinnest(pre32, pre64)
        print("  weight seed %d: thinnest small-map ReLU input %.3f x its map's fp32 error, %d units differ between fp32 and fp64" % (s, margin, flips))
        if flips == 0 and (best is None or margin > best[0]):
            best = (margin, s, r32, p32, r64, p64, names)
    assert best is not None, "no weight seed whose fp32 run keeps the fp64 branches"
    margin, seed, r32, p32, r64, p64, names = best
    print("  chosen: weight seed %d (margin %.3f)" % (seed, margin))
    write("g22_act_stage1_p0", seed, margin, 0.0, None, r32, p32, r64, p64, names)
    r64, p64, pre64, names, mask = step(G, seed, torch.float64, 0.5)
    r32, p32, pre32, _, _ = step(G, seed, torch.float32, 0.5, mask)
    assert thinnest(pre32, pre64)[1] == 0
    assert set(np.unique(mask.numpy())) == {0.0, 2.0} and tuple(mask.shape) == (B, T, HIDDEN)
    write("g22_act_stage1_mask", seed, margin, 0.5, mask, r32, p32, r64, p64, names)


if __name__ == "__main__":
    main()
