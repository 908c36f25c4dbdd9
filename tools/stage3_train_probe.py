#!/usr/bin/env python3
"""Stage-3 step on one MI355X at B = 64, T = 16, P = 96 (F = 3328, H = 1024, C = 200): one JSON line with ms per step of
  frozen_fwd_ms      glancer + policy + crop + ResNet-50 from frames up to the (B, T, F) feature matrix (no_grad, HIP)
  cls_train_fwd_ms   the classifier's training forward (GRU scan + dropout + FC, activations kept)
  backward_ms        its backward (every parameter grad; dX is not wanted in stage 3, the features are frozen)
  torch_gru_fwd_bwd_ms   context only: PyTorch's own nn.GRU + dropout + nn.Linear forward + backward at the same shapes on the same GPU
With --trace DIR (the rocprofv3 --kernel-trace output of a `--backward-only` run of this probe; one persistent scan per backward) the
backward is split by kernel:
gh GEMM (the engine's conv-GEMM kernels), the scan, the strided weight GEMMs (dW_ih, dW_hh, dW_fc, dY) and the rest, with the weight
GEMMs' fraction of the 157.3 TFLOP/s fp32 matrix peak.

Usage:  python tools/stage3_train_probe.py [--steps 20] [--warmup 5] [--backward-only] [--trace DIR] [--out FILE]
"""
import argparse
import collections
import csv
import glob
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import hip_ops, synth  # noqa: E402
from adafocus_amd.gfv_net import GFV  # noqa: E402
from tests.helpers import manifest  # noqa: E402

B, T, P, F, H, C = 64, 16, 96, 3328, 1024, 200
PEAK_F32 = 157.3e12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def split_from_trace(d):
    per, calls = collections.defaultdict(float), 0
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"]
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            key = ("scan" if "gru_bptt" in n else "weight_gemms" if "bptt_gemm" in n else
                   "gh_gemm" if "conv" in n.lower() or "gemm" in n.lower() else "other")
            per[key] += us
            calls += n.startswith("gru_bptt_scan_kernel") or "::gru_bptt_scan_kernel" in n
    out = {k + "_ms": round(v / calls / 1e3, 4) for k, v in per.items()}
    flops = 2.0 * B * T * (3 * H * F + 3 * H * H + C * H + H * C)       # dW_ih, dW_hh, dW_fc, dY (no dX in stage 3)
    if per.get("weight_gemms"):
        out["weight_gemm_gflop"] = round(flops / 1e9, 2)
        out["weight_gemm_frac_of_f32_peak"] = round(flops / (per["weight_gemms"] / calls * 1e-6) / PEAK_F32, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--backward-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = np.random.Generator(np.random.PCG64(3))
    x = torch.from_numpy(g.standard_normal((B, T, F), dtype=np.float32) * np.float32(0.5)).to(dev)
    cls_sd = synth.synth_state_dict({k: v for k, v in manifest()["ACT"].items() if k.startswith("classifier.")}, 1007)
    w = [torch.from_numpy(cls_sd["classifier." + k]).to(dev) for k in
         ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "fc.weight", "fc.bias")]
    mask = torch.empty((B, T, H), device=dev).bernoulli_(0.5).mul_(2.0)
    logits, gi, hs = hip_ops.gru_cls_train_forward(x, *w, mask=mask)
    dlogits = torch.randn_like(logits) * 1e-3

    def bwd():
        hip_ops.gru_cls_backward(x, w[0], w[1], w[3], w[4], gi, hs, mask, dlogits, want_dx=False)

    if a.backward_only:
        timed(bwd, a.steps, a.warmup)
        print(json.dumps({"backward_only_calls": a.steps + a.warmup}))
        return
    res = {"probe": "stage3_train", "B": B, "T": T, "P": P, "F": F, "H": H, "C": C, "device": torch.cuda.get_device_name(0)}
    res["backward_ms"] = round(timed(bwd, a.steps, a.warmup), 4)
    res["cls_train_fwd_ms"] = round(timed(lambda: hip_ops.gru_cls_train_forward(x, *w, mask=mask), a.steps, a.warmup), 4)
    assert hip_ops.gru_scan_timeouts() == 0

    args = types.SimpleNamespace(num_segments=T, num_classes=C, reward="random", dataset="actnet", input_size=224, batch_size=B,
                                 patch_size=P, with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49,
                                 hidden_state_dim=1024, policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003,
                                 random_patch=False, dropout=0.5, consensus="gru", hidden_dim=H, train_stage=3)
    model = GFV(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(manifest()["ACT"], 1007).items()}, strict=True)
    model = model.to(dev)
    model.train()
    model.train_mode(args)
    images = torch.from_numpy(synth.synth_frames(B, T, 224, seed=5)).to(dev)

    def frozen():
        with torch.no_grad():
            frames, fvec, actions, _, b, t = model._frozen_inputs(images, images)
            model.hot_path_features(frames, fvec, actions, b, t)
    res["frozen_fwd_ms"] = round(timed(frozen, max(a.steps // 4, 3), 2), 4)

    def step():
        logits, _ = model(input=images, scan=images, training=False, backbone_pred=False, one_step=True)
        loss = torch.nn.functional.cross_entropy(logits, torch.zeros(B * T, dtype=torch.long, device=dev))
        loss.backward()
        model.focuser.memory.clear_memory()
    res["full_step_ms"] = round(timed(step, max(a.steps // 4, 3), 2), 4)
    del model, images
    torch.cuda.empty_cache()

    try:
        gru = torch.nn.GRU(F, H, batch_first=True).to(dev)
        fc = torch.nn.Linear(H, C).to(dev)
        drop = torch.nn.Dropout(0.5)

        def ref():
            out, _ = gru(x)
            fc(drop(out).reshape(B * T, -1)).backward(dlogits)
        res["torch_gru_fwd_bwd_ms"] = round(timed(ref, a.steps, a.warmup), 4)
    except Exception as e:            # context only
        res["torch_gru_fwd_bwd_ms"] = None
        res["torch_gru_error"] = str(e)[:200]
    if a.trace:
        res.update(split_from_trace(a.trace))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
