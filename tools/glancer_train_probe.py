#!/usr/bin/env python3
"""Stage-0 training of the glancer's MobileNetV2 on one MI355X: writes profiles/glancer_stage0_probe.json.

  dw        for every distinct depthwise map of MobileNetV2 at F frames of 224 x 224: hip_ops.dwconv3x3_dgrad / dwconv3x3_wgrad
            (csrc/dw_bwd.hip) against ATen on the same device and shape -- torch.autograd.grad of F.conv2d(groups=c) on NCHW tensors, what
            a user has today --, with the bytes the algorithm moves over the time against the 6.3 TB/s the project uses as achievable HBM.
            Bytes: dgrad reads g and writes dx; wgrad reads x and g.
  bn        hip_ops.bn_map_train_forward_act / _backward_act with ReLU6 on every distinct ReLU6 map against ATen (F.batch_norm in train
            mode + F.hardtanh and its autograd).  Bytes as tools/stage0_train_probe.py: forward 2 reads of x + 1 write of y, backward 2
            reads each of x, dy, y + 1 write of dx.
  rows      hip_ops.conv2d_wgrad_rows on the five pointwise convolutions with cout 16, 24 or 144.  Bytes: reads x and g.
  step      train.train_stage0_glancer_batch (forward, cross-entropy, backward, SGD step) at B clips x T frames, its split by kernel
            family (HIP events around every hip_ops call of the walk) and the peak memory of the step.

Nothing is asserted about speed: where a HIP kernel is slower than ATen the row says so (`*_vs_aten` below 1).
Every pair alternates its members within a round; ROUNDS rounds after a warm-up; mean with the smallest and largest round.

Usage:  python tools/glancer_train_probe.py [--rounds 5] [--clips 32x16] [--fallback 16x16] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from adafocus_amd import hip_ops, synth  # noqa: E402
from adafocus_amd.train import train_stage0_glancer_batch  # noqa: E402
from stage0_train_probe import Split, rounds_of, stat  # noqa: E402

DEV = torch.device("cuda:0")
HBM = 6.3e12
# (name, input side, channels, stride): every distinct depthwise convolution of MobileNetV2 at 224 x 224
DW = (("b1 112^2x32 s1", 112, 32, 1), ("b2 112^2x96 s2", 112, 96, 2), ("b3 56^2x144 s1", 56, 144, 1), ("b4 56^2x144 s2", 56, 144, 2),
      ("b5 28^2x192 s1", 28, 192, 1), ("b7 28^2x192 s2", 28, 192, 2), ("b8 14^2x384 s1", 14, 384, 1), ("b12 14^2x576 s1", 14, 576, 1),
      ("b14 14^2x576 s2", 14, 576, 2), ("b15 7^2x960 s1", 7, 960, 1))
# (name, side, columns): every distinct map behind a ReLU6
BN = (("stem / b1.dw 112^2x32", 112, 32), ("b2.expand 112^2x96", 112, 96), ("b2.dw 56^2x96", 56, 96), ("b3 56^2x144", 56, 144),
      ("b4.dw 28^2x144", 28, 144), ("b5 28^2x192", 28, 192), ("b7.dw 14^2x192", 14, 192), ("b8 14^2x384", 14, 384), ("b12 14^2x576", 14, 576),
      ("b14.dw 7^2x576", 7, 576), ("b15 7^2x960", 7, 960), ("head 7^2x1280", 7, 1280))
# (name, side, cin, cout): the pointwise convolutions whose cout is no multiple of 32
ROWS = (("b1.project 112^2 32->16", 112, 32, 16), ("b2.project 56^2 96->24", 56, 96, 24), ("b3.expand 56^2 24->144", 56, 24, 144),
        ("b3.project 56^2 144->24", 56, 144, 24), ("b4.expand 56^2 24->144", 56, 24, 144))
CATS = {"conv2d_bn_act": "conv_fwd", "dwconv3x3_bn_act": "dw_fwd", "pack_conv_weight": "pack", "pack_dw_weight": "pack",
        "pack_conv_dgrad_weight": "pack", "bn_map_train_forward_act": "bn_fwd", "bn_map_train_backward_act": "bn_bwd",
        "conv2d_wgrad_rows": "wgrad", "dwconv3x3_wgrad": "dw_wgrad", "conv2d_dgrad": "dgrad", "dwconv3x3_dgrad": "dw_dgrad", "add": "adjoints",
        "global_avgpool": "adjoints", "global_avgpool_backward": "adjoints", "fc_meanpool_forward": "classifier", "linear": "classifier"}


def mean(v):
    return sum(v) / len(v)


def rate(row, key, moved, times):
    row[key] = stat(times)
    row[key + "_tbps"] = round(moved / (mean(times) * 1e-3) / 1e12, 3)
    row[key + "_frac_of_hbm"] = round(moved / (mean(times) * 1e-3) / HBM, 3)


def reps_of(elems):
    return 1 if elems > 5e7 else 8


def dw(frames, rounds):
    out = []
    for name, side, c, s in DW:
        oside = (side - 1) // s + 1
        x = torch.randn(frames, side, side, c, device=DEV)
        g = torch.randn(frames, oside, oside, c, device=DEV)
        w = torch.randn(c, 1, 3, 3, device=DEV) / 3
        w33 = hip_ops.pack_dw_weight(w)
        xa, ga = x.permute(0, 3, 1, 2).contiguous(), g.permute(0, 3, 1, 2).contiguous()      # ATen's default layout, NCHW
        wa = w.clone().requires_grad_(True)
        xa.requires_grad_(True)
        ya = F.conv2d(xa, wa, None, s, 1, 1, c)
        dxa, dwa = torch.autograd.grad(ya, (xa, wa), ga, retain_graph=True)
        dx, dwh = hip_ops.dwconv3x3_dgrad(g, w33, tuple(x.shape), s), hip_ops.dwconv3x3_wgrad(x, g, s)
        agree = (((dx.permute(0, 3, 1, 2) - dxa).abs().max() / dxa.abs().max()).item(), ((dwh - dwa).abs().max() / dwa.abs().max()).item())
        del dxa, dx
        r = rounds_of({"dgrad": lambda: hip_ops.dwconv3x3_dgrad(g, w33, tuple(x.shape), s),
                       "dgrad_aten": lambda: torch.autograd.grad(ya, xa, ga, retain_graph=True),
                       "wgrad": lambda: hip_ops.dwconv3x3_wgrad(x, g, s),
                       "wgrad_aten": lambda: torch.autograd.grad(ya, wa, ga, retain_graph=True)}, rounds, reps_of(x.numel()))
        row = {"map": name, "frames": frames, "x_mbytes": round(x.numel() * 4 / 2 ** 20, 1), "dx_vs_aten": agree[0], "dw_vs_aten": agree[1]}
        rate(row, "dgrad", (g.numel() + x.numel()) * 4.0, r["dgrad"])
        rate(row, "wgrad", (g.numel() + x.numel()) * 4.0, r["wgrad"])
        for k in ("dgrad", "wgrad"):
            row[k + "_aten"] = stat(r[k + "_aten"])
            row[k + "_vs_aten"] = round(mean(r[k + "_aten"]) / mean(r[k]), 2)          # above 1: the HIP kernel is faster
        assert max(agree) < 1e-4, (name, agree)           # a number for a kernel that computes something else is no number
        out.append(row)
        print(json.dumps(row), flush=True)
        del x, g, xa, ga, ya
    return out


def bn(frames, rounds):
    out = []
    for name, side, cols in BN:
        rows = frames * side * side
        x = torch.randn(rows, cols, device=DEV)
        dy = torch.randn(rows, cols, device=DEV)
        gamma, beta = 3 * (torch.rand(cols, device=DEV) + 0.5), 3 + torch.randn(cols, device=DEV)
        y, m, i = hip_ops.bn_map_train_forward_act(x, gamma, beta, act=hip_ops.ACT_RELU6)

        def aten_fwd():
            return F.hardtanh(F.batch_norm(xa, None, None, ga, ba, True, 0.1, 1e-5), 0.0, 6.0)

        xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        ya = aten_fwd()
        agree = ((y - ya).abs().max() / ya.abs().max()).item()
        r = rounds_of({"fwd": lambda: hip_ops.bn_map_train_forward_act(x, gamma, beta, act=hip_ops.ACT_RELU6),
                       "fwd_aten": lambda: aten_fwd(),
                       "bwd": lambda: hip_ops.bn_map_train_backward_act(x, y, dy, gamma, m, i, act=hip_ops.ACT_RELU6),
                       "bwd_aten": lambda: torch.autograd.grad(ya, (xa, ga, ba), dy, retain_graph=True)}, rounds, reps_of(x.numel()))
        n4 = rows * cols * 4.0
        row = {"map": name, "rows": rows, "cols": cols, "mbytes": round(n4 / 2 ** 20, 1), "y_vs_aten": agree}
        rate(row, "fwd", 3 * n4, r["fwd"])
        rate(row, "bwd", 7 * n4, r["bwd"])
        for k in ("fwd", "bwd"):
            row[k + "_aten"] = stat(r[k + "_aten"])
            row[k + "_vs_aten"] = round(mean(r[k + "_aten"]) / mean(r[k]), 2)
        assert agree < 1e-4, (name, agree)
        out.append(row)
        print(json.dumps(row), flush=True)
        del x, dy, y, xa, ya
    return out


def rows_(frames, rounds):
    out = []
    for name, side, cin, cout in ROWS:
        x = torch.randn(frames, side, side, cin, device=DEV)
        g = torch.randn(frames, side, side, cout, device=DEV)
        r = rounds_of({"wgrad_rows": lambda: hip_ops.conv2d_wgrad_rows(x, g, (cout, 1, 1, cin))}, rounds, reps_of(x.numel()))
        row = {"conv": name, "frames": frames}
        rate(row, "wgrad_rows", (x.numel() + g.numel()) * 4.0, r["wgrad_rows"])
        out.append(row)
        print(json.dumps(row), flush=True)
        del x, g
    return out


def step(b, t, rounds):
    from adafocus_amd.gfv_net import GFV
    a = types.SimpleNamespace(num_segments=t, num_classes=200, reward="random", dataset="actnet", input_size=224, batch_size=b, patch_size=96,
                              with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024, policy_conv=True,
                              gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.5, consensus="gru",
                              hidden_dim=1024, train_stage=0)
    m = GFV(a)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    m = m.to(DEV)
    m.glancer_train_mode()
    opt = torch.optim.SGD(m.glancer.net.parameters(), lr=1e-5, momentum=0.9, weight_decay=1e-4)
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=5)).to(DEV)
    target = torch.arange(b, device=DEV) % a.num_classes

    def run():
        return train_stage0_glancer_batch(m, images, target, a, opt)

    r = rounds_of({"step": run}, rounds)
    out = {"clips": b, "frames_per_clip": t, "frames": b * t, "size": 224, "train_stage0_glancer_batch": stat(r["step"])}
    with Split(CATS) as sp:
        whole = rounds_of({"step": run}, 1)["step"][0]
        parts = sp.summary(2)                       # (rounds_of ran a warm-up and one round under the events)
    out["parts"] = parts
    out["parts_sum_ms"] = round(sum(parts.values()), 3)
    out["step_under_events_ms"] = round(whole, 3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    out["peak_step_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    out["resident_before_step_mb"] = round(base / 2 ** 20, 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", default="32x16")
    ap.add_argument("--fallback", default="16x16")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "glancer_stage0_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the MI355X"
    torch.manual_seed(0)
    res = {"config": {"rounds": a.rounds, "hbm_tbps": HBM / 1e12, "asked": a.clips}}
    for clips in (a.clips, a.fallback):
        b, t = (int(v) for v in clips.split("x"))
        try:
            res["step"] = step(b, t, a.rounds)
            res["config"]["ran"] = clips
            break
        except torch.cuda.OutOfMemoryError as e:
            print("%s does not fit: %s" % (clips, str(e).splitlines()[0]), flush=True)
            res["config"].setdefault("did_not_fit", []).append(clips)
            torch.cuda.empty_cache()
    frames = b * t
    res["dw"] = dw(frames, a.rounds)
    res["bn"] = bn(frames, a.rounds)
    res["rows"] = rows_(frames, a.rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
