#!/usr/bin/env python3
"""Stage-1 training on one MI355X: writes profiles/stage1_train_probe.json.

Configuration: one GPU's share of the shipped stage-1 configuration (ACT README: 64 clips on two GPUs) -- B = 32, T = 16, frames 224 x 224,
patch 128, glance 224, 200 classes, dropout 0.8, hidden 1024.

  step      train.train_stage1_batch (zero_grad, glance, crops, walk, classifier, loss, backward, SGD step) and the peak memory above the
            resident model.
  parts     the same step written out by hand (tests/test_stage1_gpu.py holds it to the step bit for bit) with HIP events around each
            part: glance, crop, walk forward, classifier forward, loss, classifier backward, trunk backward, SGD step.
  loss      the pair: hip_ops.ce_steps (loss and gradient, two launches) against F.cross_entropy + autograd on the same logits and the
            expanded target (main_dist.py:479's expression).  Asserted: the slowest round of ce_steps beats the fastest round of ATen.

One process; every member is warmed up first; the members of a pair alternate within a round; ROUNDS rounds; mean with the smallest and
largest round.

Usage:  python tools/stage1_train_probe.py [--rounds 5] [--frames 32x16] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stage0_train_probe import rounds_of, stat  # noqa: E402
from adafocus_amd import hip_ops, synth, trunk_train  # noqa: E402
from adafocus_amd.train import train_stage1_batch  # noqa: E402
from adafocus_amd.utils import get_patch_nhwc4  # noqa: E402

DEV = torch.device("cuda:0")
SIZE, PATCH, CLASSES, DROPOUT, HIDDEN = 224, 128, 200, 0.8, 1024
PARTS = ("glance", "crop", "walk_forward", "classifier_forward", "loss", "classifier_backward", "trunk_backward", "sgd_step")


def build(b, t):
    from adafocus_amd.gfv_net import GFV
    a = types.SimpleNamespace(num_segments=t, num_classes=CLASSES, reward="random", dataset="actnet", input_size=SIZE, batch_size=b,
                              patch_size=PATCH, with_glancer=True, feature_map_channels=1280, glance_size=SIZE, action_dim=49,
                              hidden_state_dim=1024, policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=True,
                              dropout=DROPOUT, consensus="gru", hidden_dim=HIDDEN, train_stage=1)
    m = GFV(a)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    m = m.to(DEV)
    m.focuser.net.set_math("f32")
    m.stage1_train_mode()
    opt = torch.optim.SGD([{"params": m.focuser.parameters()}, {"params": m.classifier.parameters()}], lr=1e-5, momentum=0.9, weight_decay=1e-4)
    return m, a, opt


def by_hand(m, opt, images, target, b, t):
    """The step part by part: {part: ms}."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PARTS) + 1)]
    frames = images.view(b * t, 3, SIZE, SIZE)
    opt.zero_grad()
    ev[0].record()
    with torch.no_grad():
        scan = m.glancer_input(images)
        fvec = m.glancer(scan.reshape(b * t, 3, scan.shape[2], scan.shape[3]))[1]
        ev[1].record()
        patches = get_patch_nhwc4(frames, m.focuser.patch_sampler.random_actions(frames), PATCH)
    ev[2].record()
    local = trunk_train.trunk_features(m.focuser.net, patches)
    ev[3].record()
    feature = torch.cat([fvec, local.detach()], 1).view(b, t, -1).requires_grad_(True)
    logits, _ = m.classifier(feature)
    ev[4].record()
    loss = hip_ops.CeStepsFn.apply(logits, target, t)
    ev[5].record()
    loss.backward()
    ev[6].record()
    local.backward(feature.grad.view(b * t, -1)[:, fvec.shape[1]:])
    ev[7].record()
    opt.step()
    ev[8].record()
    torch.cuda.synchronize()
    return {p: ev[i].elapsed_time(ev[i + 1]) for i, p in enumerate(PARTS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", default="32x16")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stage1_train_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the MI355X"
    torch.manual_seed(0)
    b, t = (int(v) for v in a.frames.split("x"))
    m, args, opt = build(b, t)
    images = torch.from_numpy(synth.synth_frames(b, t, SIZE, seed=5)).to(DEV)
    target = torch.arange(b, device=DEV) % CLASSES
    res = {"config": {"rounds": a.rounds, "batch": b, "segments": t, "size": SIZE, "patch": PATCH, "classes": CLASSES, "dropout": DROPOUT}}

    r = rounds_of({"train_stage1_batch": lambda: train_stage1_batch(m, images, target, args, opt)}, a.rounds)
    res["step"] = {"train_stage1_batch": stat(r["train_stage1_batch"])}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    train_stage1_batch(m, images, target, args, opt)
    torch.cuda.synchronize()
    res["step"]["peak_mb_above_resident"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    res["step"]["resident_mb"] = round(base / 2 ** 20, 1)
    print(json.dumps(res["step"]), flush=True)

    by_hand(m, opt, images, target, b, t)
    runs = [by_hand(m, opt, images, target, b, t) for _ in range(a.rounds)]
    res["parts"] = {p: stat([x[p] for x in runs]) for p in PARTS}
    res["parts"]["sum_of_means_ms"] = round(sum(res["parts"][p]["mean_ms"] for p in PARTS), 3)
    print(json.dumps(res["parts"]), flush=True)

    logits = torch.randn(b * t, CLASSES, device=DEV)

    def aten():
        leaf = logits.detach().requires_grad_(True)
        F.cross_entropy(leaf, target.view(b, -1).expand(b, t).reshape(-1)).backward()
        return leaf.grad

    def fn():
        leaf = logits.detach().requires_grad_(True)
        hip_ops.CeStepsFn.apply(leaf, target, t).backward()
        return leaf.grad

    pair = rounds_of({"ce_steps": lambda: hip_ops.ce_steps(logits, target, t), "aten_cross_entropy_autograd": aten,
                      "ce_steps_fn_autograd": fn}, a.rounds, reps=20)
    res["loss"] = {k: stat(v) for k, v in pair.items()}
    res["loss"]["rows"], res["loss"]["reps_per_round"] = b * t, 20
    res["loss"]["grad_vs_aten"] = ((hip_ops.ce_steps(logits, target, t)[1] - aten()).abs().max() / aten().abs().max()).item()
    print(json.dumps(res["loss"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    assert max(pair["ce_steps"]) < min(pair["aten_cross_entropy_autograd"]), (pair["ce_steps"], pair["aten_cross_entropy_autograd"])


if __name__ == "__main__":
    main()
