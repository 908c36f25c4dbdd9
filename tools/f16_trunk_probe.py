#!/usr/bin/env python3
"""fp16 ResNet-50 trunk (ADAF_MATH_F16) against the fp32 trunk, in one process on one device: ONE JSON line with
  trunk_ms_per_1024   ms per 1024 patches at 96^2, 128^2, 144^2 (median of timed forwards, events around the whole call)
  act_clips_s         hot-path clips/s, ActivityNet: the headline shape (B = 64, T = 16, P = 96) and config 4's shape (T = 8, P = 128)
  sth_clips_s         Something-Something action_stage3 (gather + TSM trunk + FC / mean): config 4 (Tf = 8, P = 128, temporal shift) and the
                      shipped configuration (Tg = 8, Tf = 12, P = 144)
  launches_f16_96     forward_profiled of the fp16 trunk at 1024 x 96^2: per launch ms, the FLOP share of the f16 MFMA peak (2.5 PF dense)
                      and the byte share of HBM (6.3 TB/s achievable) over the launch's time
Usage: python tools/f16_trunk_probe.py [--quick]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import act_args, synth_model_state  # noqa: E402
from adafocus_amd import synth  # noqa: E402
from adafocus_amd.resnet import resnet50  # noqa: E402
from adafocus_amd.utils import nchw_to_nhwc4  # noqa: E402
from tests.helpers import synth_sd  # noqa: E402

dev = torch.device("cuda:0")
QUICK = "--quick" in sys.argv
F16_PEAK, HBM = 2.5e15, 6.3e12


def timed(fn, steps=10 if not QUICK else 3, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def trunk(math):
    net = resnet50(num_classes=200).eval()
    net.load_state_dict(synth_sd("ACT", 1007, "focuser.net.", keep_prefix=False), strict=True)
    net.set_math(math)
    return net.to(dev)


def act_model(t, p, b, math):
    from adafocus_amd.gfv_net import GFV
    a = act_args(t, p, b)
    a.local_math = math
    m = GFV(a).eval()
    m.load_state_dict(synth_model_state(m, 1007))
    return m.to(dev)


def sth_model(tf, p, b, math):
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.gpu, a.batch_size, a.num_segments_focuser, a.patch_size, a.local_math = 0, b, tf, p, math
    m = GFV(a).eval()
    m.load_state_dict(synth_model_state(m, 1007))
    return m.to(dev), a


def main():
    out = {"trunk_ms_per_1024": {}, "act_clips_s": {}, "sth_clips_s": {}}
    nets = {m: trunk(m) for m in ("f32", "f16")}
    with torch.no_grad():
        for p in (96, 128, 144):
            x = nchw_to_nhwc4(torch.randn((1024, 3, p, p), device=dev))
            row = {m: round(timed(lambda: nets[m].features_nhwc4(x)), 3) for m in nets}
            row["speedup"] = round(row["f32"] / row["f16"], 2)
            out["trunk_ms_per_1024"][str(p)] = row
        x = nchw_to_nhwc4(torch.randn((1024, 3, 96, 96), device=dev))
        prof = nets["f16"]._sync().profile(x)
        out["launches_f16_96"] = [dict(ms=round(r["ms"], 4), tile=r["tile"], flop_frac=round(r["flops"] / (r["ms"] * 1e-3) / F16_PEAK, 3) if r["ms"] > 0 else 0,
                                       hbm_frac=round(r["bytes"] / (r["ms"] * 1e-3) / HBM, 3) if r["ms"] > 0 else 0) for r in prof]
        out["launches_f16_96_total_ms"] = round(sum(r["ms"] for r in prof), 3)
        del nets
        for t, p in ((16, 96), (8, 128)):
            b = 64
            frames = torch.from_numpy(synth.synth_frames(b, t, 224, seed=1)).to(dev).view(b * t, 3, 224, 224)
            actions = torch.from_numpy(synth.synth_actions(b * t, 7, seed=2)[1]).to(dev)
            gvec = torch.randn((b, t, 1280), device=dev)
            row = {}
            for m in ("f32", "f16"):
                model = act_model(t, p, b, m)
                row[m] = round(b / (timed(lambda: model.hot_path(frames, gvec, actions, b, t)) * 1e-3), 1)
                del model
            row["speedup"] = round(row["f16"] / row["f32"], 2)
            out["act_clips_s"]["T%d_P%d_B%d" % (t, p, b)] = row
            del frames
        for tf, p in ((8, 128), (12, 144)):
            b = 64
            fo = torch.from_numpy(synth.synth_frames(b, tf, 224, seed=4)).view(b, tf, 3, 224, 224).to(dev)
            fm = torch.randn((b, 8, 7, 7, 1280), device=dev).permute(0, 1, 4, 2, 3)
            glog = torch.randn((b, 8, 174), device=dev)
            forced = torch.rand((b, 2), device=dev)
            row = {}
            for m in ("f32", "f16"):
                model, a = sth_model(tf, p, b, m)
                row[m] = round(b / (timed(lambda: model.action_stage3(fo, fm, glog, 0, a, prev_local_patch=None, forced_action=forced)) * 1e-3), 1)
                del model
            row["speedup"] = round(row["f16"] / row["f32"], 2)
            out["sth_clips_s"]["Tg8_Tf%d_P%d_B%d" % (tf, p, b)] = row
            del fo
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
