#!/usr/bin/env python3
"""Stage-0 training of the local CNN (BatchNorm on batch statistics) on one MI355X: writes profiles/stage0_train_probe.json.

  kernels   for every distinct trunk map shape of ResNet-50 at 384 patches of 144 x 144 (DESIGN 3.13's B = 32 configuration):
            hip_ops.bn_map_train_forward / _backward (csrc/bn_map.hip) against hip_ops.bn_train_forward / _backward (the PPO encoder's
            kernels of csrc/ppo_train.hip, the only batch-statistics BatchNorm before) on the same map, with the achieved bytes per second
            of the new ones against the 6.3 TB/s the project uses as achievable HBM.  Bytes are what the algorithm moves: forward
            2 reads of x + 1 write of y, backward 2 reads each of x, dy, y + 1 write of dx.  The new kernels must be faster on every
            shape (asserted).
  step      a whole training step of the trunk walk (forward + backward for a given d(features)) on the same patches, batch statistics
            against the frozen statistics of DESIGN 3.13, with its parts (HIP events around every hip_ops call of the walk) and the peak
            activation memory of both.
  stage0    train.train_stage0_batch (forward, cross-entropy, backward, SGD step) at B x T frames of 224 x 224.

Every pair alternates its members within a round; ROUNDS rounds after a warm-up; mean with the smallest and largest round.

Usage:  python tools/stage0_train_probe.py [--rounds 5] [--patches 384] [--frames 8x8] [--out FILE]
"""
import argparse
import collections
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import hip_ops, resnet, synth, trunk_train  # noqa: E402
from adafocus_amd.train import train_stage0_batch  # noqa: E402

DEV = torch.device("cuda:0")
HBM = 6.3e12
P = 144
# (name, rows per patch, columns): every distinct (rows, cols) of the ResNet-50 trunk's conv outputs at 144 x 144
MAPS = (("stem 72x72x64", 72 * 72, 64), ("layer1 36x36x64", 36 * 36, 64), ("layer1 36x36x256", 36 * 36, 256), ("layer2.0.conv1 36x36x128", 36 * 36, 128),
        ("layer2 18x18x128", 18 * 18, 128), ("layer2 18x18x512", 18 * 18, 512), ("layer3.0.conv1 18x18x256", 18 * 18, 256),
        ("layer3 9x9x256", 81, 256), ("layer3 9x9x1024", 81, 1024), ("layer4.0.conv1 9x9x512", 81, 512), ("layer4 5x5x512", 25, 512),
        ("layer4 5x5x2048", 25, 2048))
CATS = {"conv2d_bn_act": "conv_fwd", "stem7x7_bn_relu": "conv_fwd", "pack_conv_weight": "pack", "fold_bn": "pack", "bn_map_train_forward": "bn_fwd",
        "bn_map_train_backward": "bn_bwd", "conv_bn_param_grad": "bn_bwd", "conv2d_wgrad": "wgrad", "conv2d_dgrad": "dgrad",
        "pack_conv_dgrad_weight": "dgrad", "relu_backward": "adjoints", "global_avgpool_backward": "adjoints", "maxpool3x3s2_backward": "adjoints",
        "temporal_shift_backward": "adjoints", "temporal_shift": "adjoints", "maxpool3x3s2": "adjoints", "global_avgpool": "adjoints"}


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def rounds_of(fns, rounds, reps=1):
    """{name: [ms per call, one entry per round]}: one warm-up of every member, then the members alternate within each round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = collections.defaultdict(list)
    for _ in range(rounds):
        for name, fn in fns.items():
            out[name].append(once(lambda: [fn() for _ in range(reps)]) / reps)
    return out


def stat(v):
    return {"mean_ms": round(sum(v) / len(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def kernels(patches, rounds):
    rows_out = []
    for name, per, cols in MAPS:
        rows = patches * per
        x = torch.randn(rows, cols, device=DEV)
        dy = torch.randn(rows, cols, device=DEV)
        gamma, beta = torch.rand(cols, device=DEV) + 0.5, torch.randn(cols, device=DEV)
        y, mean, invstd = hip_ops.bn_map_train_forward(x, gamma, beta)
        y_old, mean_old, invstd_old = hip_ops.bn_train_forward(x, gamma, beta)
        agree = ((y - y_old).abs().max() / y_old.abs().max()).item()           # faster and different is not faster
        reps = 1 if rows * cols > 5e7 else 4
        r = rounds_of({"fwd_new": lambda: hip_ops.bn_map_train_forward(x, gamma, beta), "fwd_old": lambda: hip_ops.bn_train_forward(x, gamma, beta),
                       "bwd_new": lambda: hip_ops.bn_map_train_backward(x, y, dy, gamma, mean, invstd),
                       "bwd_old": lambda: hip_ops.bn_train_backward(x, y, dy, gamma, mean, invstd)}, rounds, reps)
        n4 = rows * cols * 4.0
        row = {"map": name, "rows": rows, "cols": cols, "mbytes": round(n4 / 2 ** 20, 1), "y_new_vs_old": agree}
        for d, moved in (("fwd", 3 * n4), ("bwd", 7 * n4)):
            new, old = r[d + "_new"], r[d + "_old"]
            row[d + "_new"], row[d + "_old"] = stat(new), stat(old)
            row[d + "_speedup"] = round((sum(old) / len(old)) / (sum(new) / len(new)), 2)
            row[d + "_new_tbps"] = round(moved / (sum(new) / len(new) * 1e-3) / 1e12, 3)
            row[d + "_new_frac_of_hbm"] = round(moved / (sum(new) / len(new) * 1e-3) / HBM, 3)
            assert max(new) < min(old), (name, d, new, old)
        assert agree < 1e-5, (name, agree)
        rows_out.append(row)
        print(json.dumps(row), flush=True)
        del x, dy, y, y_old
    return rows_out


class Split:
    """HIP events around the hip_ops calls of a walk: category -> [(start, end)].  cats: hip_ops name -> category (None: CATS)."""

    def __init__(self, cats=None):
        self.events, self.saved, self.cats = collections.defaultdict(list), {}, CATS if cats is None else cats

    def __enter__(self):
        for name, cat in self.cats.items():
            fn = self.saved[name] = getattr(hip_ops, name)

            def wrapped(*a, _fn=fn, _cat=cat, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*a, **k)
                e1.record()
                self.events[_cat].append((e0, e1))
                return out

            setattr(hip_ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(hip_ops, name, fn)
        return False

    def summary(self, steps):
        torch.cuda.synchronize()
        return {k + "_ms": round(sum(a.elapsed_time(b) for a, b in v) / steps, 3) for k, v in sorted(self.events.items())}


def step(patches_n, rounds):
    net = resnet.resnet50()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    net = net.to(DEV)
    net.set_math("f32")
    net.set_trainable(True)
    net.set_bn_batch_stats(True)
    x4 = torch.randn(patches_n, P, P, 4, device=DEV)
    x4[..., 3] = 0
    dfeat = torch.randn(patches_n, 2048, device=DEV)

    def run(train):
        net.train(train)
        net.zero_grad(set_to_none=True)
        trunk_train.trunk_features(net, x4).backward(dfeat)

    r = rounds_of({"batch_stats": lambda: run(True), "frozen_stats": lambda: run(False)}, rounds)
    out = {"patches": patches_n, "patch": P, "batch_stats": stat(r["batch_stats"]), "frozen_stats": stat(r["frozen_stats"])}
    for name, train in (("batch_stats", True), ("frozen_stats", False)):
        with Split() as sp:
            run(train)
            out[name]["parts"] = sp.summary(1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(train)
        torch.cuda.synchronize()
        out[name]["peak_activation_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        net.zero_grad(set_to_none=True)
    print(json.dumps(out), flush=True)
    return out


def stage0(b, t, rounds):
    from adafocus_amd.gfv_net import GFV
    a = types.SimpleNamespace(num_segments=t, num_classes=200, reward="random", dataset="actnet", input_size=224, batch_size=b, patch_size=96,
                              with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024, policy_conv=True,
                              gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.5, consensus="gru",
                              hidden_dim=1024, train_stage=0)
    m = GFV(a)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    m = m.to(DEV)
    m.focuser.net.set_math("f32")
    m.backbone_train_mode()
    opt = torch.optim.SGD(m.focuser.net.parameters(), lr=1e-5, momentum=0.9, weight_decay=1e-4)
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=5)).to(DEV)
    target = torch.arange(b, device=DEV) % a.num_classes
    r = rounds_of({"train_stage0_batch": lambda: train_stage0_batch(m, images, target, a, opt)}, rounds)
    out = {"batch": b, "segments": t, "frames": b * t, "size": 224, "train_stage0_batch": stat(r["train_stage0_batch"])}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    train_stage0_batch(m, images, target, a, opt)
    torch.cuda.synchronize()
    out["peak_activation_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--patches", type=int, default=384)
    ap.add_argument("--frames", default="8x8")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stage0_train_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the MI355X"
    torch.manual_seed(0)
    b, t = (int(v) for v in a.frames.split("x"))
    res = {"config": {"rounds": a.rounds, "patches": a.patches, "patch": P, "hbm_tbps": HBM / 1e12}}
    res["kernels"] = kernels(a.patches, a.rounds)
    res["step"] = step(a.patches, a.rounds)
    res["stage0"] = stage0(b, t, a.rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
