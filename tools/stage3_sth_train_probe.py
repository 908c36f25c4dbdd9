#!/usr/bin/env python3
"""Stage-3 step of the Something-Something model with the local CNN fine-tuned, on one MI355X, at the shipped configuration (Tg = 8,
Tf = 12, P = 144, TSM-ResNet-50) for B = 8 and B = 32: writes profiles/stage3_sth_train_probe.json, per batch size ms per step of

  frozen_ms          glance + policy + crop up to the (B*Tf, P, P, 4) patches (no_grad, HIP)
  engine_fwd_ms      the eval engine's fused forward on those patches (context: what inference pays)
  walk_fwd_ms        the training walk's forward on the same patches, one launch per layer, every output kept
  head_ms            dropout + FC + mean over frames + cross-entropy, forward and backward
  backward_ms        the trunk's backward, and its split (HIP events around every hip_ops call of the walk):
    wgrad_ms / wgrad_by_stage   the split-K weight gradients with their fraction of the 157.3 TFLOP/s fp32 matrix peak per stage
    dgrad_ms           filter packing + (zero insertion) + the engine launch
    dgrad_s2_3x3_ms    of which the three zero-inserted 3x3 stride-2 convs (4x the FLOPs of a strided form)
    small_ms           ReLU / pool / max-pool / shift adjoints
    bn_param_ms        column sums + dW scaling + dgamma / dbeta
  sgd_step_ms        torch.optim.SGD.step on the reference's groups
  repack_ms          the engine's re-pack of every weight at the first eval forward after the step (ResNet._sync)
  peak_activation_mb peak device memory of one forward + backward above the resident model
and, as context, the 1x1 weight-gradient shapes of the trunk through the strided GEMM the GRU backward uses (adaf_ppo_wenc_grad_f32 with
split_k = 0) against the split-K kernel.

Usage:  python tools/stage3_sth_train_probe.py [--steps 5] [--warmup 2] [--batches 8,32] [--out FILE]
"""
import argparse
import collections
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import hip_ops, synth, trunk_train  # noqa: E402
from adafocus_amd.gfv_net_sth import GFV  # noqa: E402
from tests.test_state_dict_compat import sth_args  # noqa: E402

TG, TF, P = 8, 12, 144
PEAK_F32 = 157.3e12
DEV = torch.device("cuda:0")


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


class Split:
    """HIP events around the hip_ops calls of the walk's backward: category -> [(start, end, flops)]."""
    CATS = {"conv2d_wgrad": "wgrad", "conv2d_dgrad": "dgrad", "pack_conv_dgrad_weight": "dgrad", "relu_backward": "small",
            "global_avgpool_backward": "small", "maxpool3x3s2_backward": "small", "temporal_shift_backward": "small",
            "temporal_shift": "small", "maxpool3x3s2": "small", "conv_bn_param_grad": "bn_param"}

    def __init__(self):
        self.events = collections.defaultdict(list)
        self.saved = {}

    def __enter__(self):
        for name, cat in self.CATS.items():
            fn = self.saved[name] = getattr(hip_ops, name)

            def wrapped(*a, _fn=fn, _name=name, _cat=cat, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*a, **k)
                e1.record()
                key, flops = _cat, 0.0
                stride = k.get("stride", a[3] if len(a) > 3 else 1)
                if _name == "conv2d_wgrad":
                    g, (cout, kh, kw, cin) = a[1], a[2]
                    flops = 2.0 * g.shape[0] * g.shape[1] * g.shape[2] * cout * kh * kw * (3 if kh == 7 else cin)
                    # the stage from the block's planes: a stride-2 1x1 is a downsample conv (2 planes -> 4 planes), else min(cin, cout)
                    planes = cout // 4 if (kh == 1 and stride == 2) else min(cout, cin)
                    key = "wgrad:%d" % (0 if kh == 7 else {64: 1, 128: 2, 256: 3, 512: 4}[planes])
                elif _name == "conv2d_dgrad" and a[1].shape[1] == 3 and stride == 2:
                    key = "dgrad_s2_3x3"
                self.events[key].append((e0, e1, flops))
                return out

            setattr(hip_ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(hip_ops, name, fn)
        return False

    def summary(self, steps):
        torch.cuda.synchronize()
        ms = {k: sum(a.elapsed_time(b) for a, b, _ in v) / steps for k, v in self.events.items()}
        fl = {k: sum(f for _, _, f in v) / steps for k, v in self.events.items()}
        names = ("stem", "layer1", "layer2", "layer3", "layer4")
        by_stage = {}
        for k in sorted(ms):
            if k.startswith("wgrad:"):
                by_stage[names[int(k[6:])]] = {"ms": round(ms[k], 3), "gflop": round(fl[k] / 1e9, 1),
                                               "frac_of_f32_peak": round(fl[k] / (ms[k] * 1e-3) / PEAK_F32, 4)}
        wg_ms = sum(v for k, v in ms.items() if k.startswith("wgrad:"))
        wg_fl = sum(v for k, v in fl.items() if k.startswith("wgrad:"))
        return {"wgrad_ms": round(wg_ms, 3), "wgrad_frac_of_f32_peak": round(wg_fl / (wg_ms * 1e-3) / PEAK_F32, 4), "wgrad_by_stage": by_stage,
                "dgrad_ms": round(ms.get("dgrad", 0.0) + ms.get("dgrad_s2_3x3", 0.0), 3), "dgrad_s2_3x3_ms": round(ms.get("dgrad_s2_3x3", 0.0), 3),
                "small_ms": round(ms.get("small", 0.0), 3), "bn_param_ms": round(ms.get("bn_param", 0.0), 3)}


def model_for(b):
    a = sth_args()
    a.gpu, a.batch_size, a.num_segments_glancer, a.num_segments_focuser, a.patch_size = 0, b, TG, TF, P
    m = GFV(a)
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    pol_shapes = {"policy." + k: tuple(v.shape) for k, v in m.focuser.policy.policy_old.state_dict().items()}
    pol = {k[len("policy."):]: torch.from_numpy(v) for k, v in synth.synth_state_dict(pol_shapes, 1007).items()}
    for p in (m.focuser.policy.policy_old, m.focuser.policy.policy):
        p.load_state_dict(pol)
    return m.to(DEV), a


def probe(b, steps, warmup):
    m, a = model_for(b)
    m.stage3_train_mode()
    net = m.focuser.net.base_model
    gl = torch.from_numpy(synth.synth_frames(b, TG, 224, seed=3)).to(DEV)
    fo = torch.from_numpy(synth.synth_frames(b, TF, 224, seed=4)).view(b, TF, 3, 224, 224).to(DEV)
    target = torch.arange(b, device=DEV) % a.num_classes
    groups = m.focuser.net.get_optim_policies() + [{"params": list(m.classifier.parameters())}]
    opt = torch.optim.SGD(groups, lr=0, momentum=0.9, weight_decay=5e-4)
    for g in opt.param_groups:
        g["lr"] = 1e-5 * g.get("lr_mult", 1)
    out = {"batch": b, "patches": b * TF}

    def frozen():
        with torch.no_grad():
            fm, glog = m.glance(gl)
            return m._stage_features(fo, fm, 0, a, None, False, None, None, patches_only=True)[0], glog

    out["frozen_ms"] = round(timed(frozen, steps, warmup), 3)
    patches, glog = frozen()

    def engine():
        with torch.no_grad():
            return net.features_nhwc4(patches)

    out["engine_fwd_ms"] = round(timed(engine, steps, warmup), 3)
    out["walk_fwd_ms"] = round(timed(lambda: trunk_train.trunk_features(net, patches), steps, warmup), 3)
    feat = trunk_train.trunk_features(net, patches).detach()

    from adafocus_amd.gfv_net_sth import _FcMeanPool

    def head_step():
        f = feat.clone().requires_grad_(True)
        logit = _FcMeanPool.apply(m.dropout(f), m.classifier.weight, m.classifier.bias, glog, b)
        F.cross_entropy(logit, target).backward()
        return f.grad

    out["head_ms"] = round(timed(head_step, steps, warmup), 3)
    dfeat = head_step().detach()
    m.zero_grad(set_to_none=True)

    def fwd_bwd():
        trunk_train.trunk_features(net, patches).backward(dfeat)

    both = timed(fwd_bwd, steps, warmup)
    out["backward_ms"] = round(both - out["walk_fwd_ms"], 3)
    with Split() as sp:
        for _ in range(steps):
            fwd_bwd()
        out.update(sp.summary(steps))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_bwd()
    torch.cuda.synchronize()
    out["peak_activation_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    out["sgd_step_ms"] = round(timed(opt.step, steps, warmup), 3)

    def repack():
        opt.step()                       # bumps every parameter version: the next eval forward re-packs the engine's weights
        engine()

    out["repack_ms"] = round(timed(repack, steps, warmup) - out["sgd_step_ms"] - out["engine_fwd_ms"], 3)
    out["step_ms"] = round(out["frozen_ms"] + both + out["head_ms"] + out["sgd_step_ms"], 3)
    return out


def pointwise_context(b, steps, warmup):
    """The trunk's 1x1 weight-gradient shapes at b * Tf patches: the split-K kernel against the strided GEMM (one chain per output)."""
    n = b * TF
    rows = []
    for name, hw, cin, cout in (("layer1 64->256", 36, 64, 256), ("layer1 256->64", 36, 256, 64), ("layer2 512->128", 18, 512, 128),
                                ("layer3 1024->256", 9, 1024, 256), ("layer3 256->1024", 9, 256, 1024), ("layer4 2048->512", 5, 2048, 512),
                                ("layer4 512->2048", 5, 512, 2048)):
        x = torch.randn(n, hw, hw, cin, device=DEV)
        g = torch.randn(n, hw, hw, cout, device=DEV)
        flops = 2.0 * n * hw * hw * cin * cout
        sk = timed(lambda: hip_ops.conv2d_wgrad(x, g, (cout, 1, 1, cin)), steps, warmup)
        st = timed(lambda: hip_ops.ppo_wenc_grad(x.view(-1, cin), g.view(-1, cout), None, split_k=False), steps, warmup)
        rows.append({"shape": name, "pixels": n * hw * hw, "split_k_ms": round(sk, 3), "split_k_frac_of_f32_peak": round(flops / (sk * 1e-3) / PEAK_F32, 4),
                     "strided_gemm_ms": round(st, 3), "strided_gemm_frac_of_f32_peak": round(flops / (st * 1e-3) / PEAK_F32, 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="8,32")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stage3_sth_train_probe.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    res = {"config": {"Tg": TG, "Tf": TF, "P": P, "base_model": "resnet50", "steps": a.steps, "warmup": a.warmup}, "runs": [], "pointwise_wgrad": {}}
    for b in (int(v) for v in a.batches.split(",")):
        res["runs"].append(probe(b, a.steps, a.warmup))
        print(json.dumps(res["runs"][-1]), flush=True)
        res["pointwise_wgrad"]["B%d" % b] = pointwise_context(b, a.steps, a.warmup)
        print(json.dumps(res["pointwise_wgrad"]["B%d" % b]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
