#!/usr/bin/env python3
"""ResNet-50 / -101 / -152 local CNN on the HIP trunk, all three depths in one process on one device: ONE JSON line with
  trunk_ms_per_1024   ms per 1024 patches at 96^2 and 128^2, fp32 and fp16 (median of timed forwards, events around the whole call)
  conv_frac_f32_96    forward_profiled of the fp32 trunk at 1024 x 96^2: the conv launches' algorithmic FLOPs over their summed time, as a
                      fraction of the dense fp32 MFMA peak (bench.MFMA_F32_PEAK_TFLOPS); also that ratio against ResNet-50's, and the
                      five conv launches furthest below the depth's own fraction
  sth_clips_s         Something-Something action_stage3 with base_model = <depth> (gather + TSM trunk + FC / mean): Tf = 8, P = 128, B = 64
Usage: python tools/resnet_depth_probe.py [--quick]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import MFMA_F32_PEAK_TFLOPS, synth_model_state  # noqa: E402
from adafocus_amd import resnet, synth  # noqa: E402
from adafocus_amd.utils import nchw_to_nhwc4  # noqa: E402

dev = torch.device("cuda:0")
QUICK = "--quick" in sys.argv
DEPTHS = ("resnet50", "resnet101", "resnet152")


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


def trunk(arch):
    net = getattr(resnet, arch)()
    net.load_state_dict(synth_model_state(net, 1007), strict=True)
    return net.eval().to(dev)


def sth_model(arch, tf, p, b):
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.gpu, a.batch_size, a.num_segments_focuser, a.patch_size, a.base_model = 0, b, tf, p, arch
    m = GFV(a).eval()
    m.load_state_dict(synth_model_state(m, 1007))
    return m.to(dev), a


def main():
    out = {"trunk_ms_per_1024": {}, "conv_frac_f32_96": {}, "sth_clips_s": {}}
    with torch.no_grad():
        xs = {p: nchw_to_nhwc4(torch.randn((1024, 3, p, p), device=dev)) for p in (96, 128)}
        for arch in DEPTHS:
            net = trunk(arch)
            row = {}
            for math in ("f32", "f16"):
                net.set_math(math)
                for p, x in xs.items():
                    row["%s_%d" % (math, p)] = round(timed(lambda: net.features_nhwc4(x)), 3)
            out["trunk_ms_per_1024"][arch] = row
            net.set_math("f32")
            prof = net._sync().profile(xs[96])
            convs = [r for r in prof if r["flops"] > 0 and r["ms"] > 0]
            fl, ms = sum(r["flops"] for r in convs), sum(r["ms"] for r in convs)
            frac = fl / (ms * 1e-3) / (MFMA_F32_PEAK_TFLOPS * 1e12)
            low = sorted(((r["flops"] / (r["ms"] * 1e-3) / (MFMA_F32_PEAK_TFLOPS * 1e12), i, r) for i, r in enumerate(prof) if r in convs))[:5]
            out["conv_frac_f32_96"][arch] = dict(tflop=round(fl / 1e12, 3), conv_ms=round(ms, 3), launches=len(prof), frac=round(frac, 3),
                                                 lowest=[dict(launch=i, tile=r["tile"], ms=round(r["ms"], 4), frac=round(f, 3)) for f, i, r in low])
            del net
        base = out["conv_frac_f32_96"]["resnet50"]["frac"]
        for arch in DEPTHS:
            out["conv_frac_f32_96"][arch]["vs_resnet50"] = round(out["conv_frac_f32_96"][arch]["frac"] / base, 3)
        del xs
        tf, p, b = 8, 128, 64
        fo = torch.from_numpy(synth.synth_frames(b, tf, 224, seed=4)).view(b, tf, 3, 224, 224).to(dev)
        fm = torch.randn((b, 8, 7, 7, 1280), device=dev).permute(0, 1, 4, 2, 3)
        glog = torch.randn((b, 8, 174), device=dev)
        forced = torch.rand((b, 2), device=dev)
        for arch in DEPTHS:
            model, a = sth_model(arch, tf, p, b)
            ms = timed(lambda: model.action_stage3(fo, fm, glog, 0, a, prev_local_patch=None, forced_action=forced))
            out["sth_clips_s"]["%s_Tf%d_P%d_B%d" % (arch, tf, p, b)] = round(b / (ms * 1e-3), 1)
            del model
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
