#!/usr/bin/env python3
"""Bit-level fingerprint of the ResNet trunk's host walk: for every case one JSON line with the sha256 of the feature bytes (and of the map for
forward_map) and, from profile(), the (flops, bytes, tile) of every launch -- no times, so two builds of the library that take the same
launch decisions and compute the same bits print the same file.  Cases: the three arithmetics x depths x patch sizes / batch sizes on
both sides of the fused forms' thresholds x shift placements x fusion settings x tile overrides x entry points.  Weights and inputs are
seeded (adafocus_amd.synth); only the public surface of resnet.py / hip_ops.ResNet50Trunk is used.
Usage: python tools/trunk_digest.py > digest.json        (compare two trees with diff)"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import _lib, resnet, synth  # noqa: E402
from adafocus_amd.utils import nchw_to_nhwc4  # noqa: E402

dev = torch.device("cuda:0")
MATHS = ("f32", "split_bf16", "f16")
_inputs = {}


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def patches(n, p):
    if (n, p) not in _inputs:
        _inputs[(n, p)] = nchw_to_nhwc4(torch.from_numpy(synth.synth_frames(n, 1, p, seed=100 + p)).to(dev))
    return _inputs[(n, p)]


def build(arch):
    net = getattr(resnet, arch)()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    return net.eval().to(dev)


def cases(arch, math):
    """(name, entry, n, patch, settings); settings: T / div / place (shift), fusion, lat_rows, tiles {conv launch: id}."""
    f16 = math == "f16"
    plain = dict(T=0)
    s8 = dict(T=8, place="blockres")
    if arch != "resnet50":          # the deeper stacks: one plain and one shifted case (every other conv1 shifted)
        return [("plain", "forward", 64, 96, plain), ("blockres8", "forward", 128, 96, s8)]
    out = []
    for n, p in ((16, 96), (64, 96), (1024, 96), (1032, 96), (64, 128), (64, 144), (64, 100)):
        out.append(("plain", "forward", n, p, plain))
    for n, p in ((128, 96), (64, 128)):
        out.append(("blockres8", "forward", n, p, s8))
    for n, p in ((240, 96), (96, 144)):       # 12 segments: the next conv1 stays out of the fused tail
        out.append(("blockres12", "forward", n, p, dict(T=12, place="blockres")))
    out.append(("block8", "forward", 128, 96, dict(T=8, place="block")))
    out.append(("blockres8_div4", "forward", 128, 96, dict(T=8, place="blockres", div=4)))
    out.append(("blockres8_div16", "forward", 128, 96, dict(T=8, place="blockres", div=16)))     # fold 64 / 16 = 4: refused by the fp16 trunk
    for fusion in (0, 2):
        for n in (16, 128):
            out.append(("fusion%d" % fusion, "forward", n, 96, dict(T=0, fusion=fusion)))
        out.append(("fusion%d_blockres8" % fusion, "forward", 128, 96, dict(T=8, place="blockres", fusion=fusion)))
        out.append(("fusion%d_block8" % fusion, "forward", 128, 96, dict(T=8, place="block", fusion=fusion)))
    out.append(("lat0", "forward", 16, 96, dict(T=0, lat_rows=0)))
    out.append(("tile_stage1", "forward", 128, 96, dict(T=0, tiles={2: 82 if f16 else 2})))
    out.append(("tile_stage1_blockres8", "forward", 128, 96, dict(T=8, place="blockres", tiles={5: 82 if f16 else 2})))
    if math == "f32":
        out.append(("tile_stem", "forward", 64, 96, dict(T=0, tiles={0: 2})))
    for n, p in ((16, 96), (64, 96), (64, 100)):
        out.append(("plain", "forward_map", n, p, plain))
    out.append(("blockres8", "forward_map", 128, 96, s8))
    # two action sets over 160 frames of 168^2: 320 patches (the strip stem gathers its own windows at 96 and 144, not at 100, not for 16 patches)
    for layout in ("planar", "pixel_major"):
        for nf, p in ((160, 96), (160, 144), (160, 100), (8, 96)):
            out.append((layout, "forward_frames", nf, p, plain))
        out.append((layout + "_blockres8", "forward_frames", 160, 96, s8))
        out.append((layout + "_fusion0", "forward_frames", 160, 96, dict(T=0, fusion=0)))
    return out


def run(net, arch, math, name, entry, n, p, cfg):
    trunk = net._sync()
    nconv = 1 + 3 * sum(net.layers) + 4
    T, div = cfg.get("T", 0), cfg.get("div", 8)
    trunk.set_fusion(cfg.get("fusion", 1))
    trunk.set_shift_place(cfg.get("place", "blockres"))
    trunk.set_latency_rows(cfg.get("lat_rows", -1))
    tiles = [0] * nconv
    for i, t in cfg.get("tiles", {}).items():
        tiles[i] = t
    trunk.set_tiles(tiles)
    rec = dict(arch=arch, math=math, case=name, entry=entry, n=n, patch=p, **{k: v for k, v in cfg.items() if k != "tiles"})
    if "tiles" in cfg:
        rec["tiles"] = sorted(cfg["tiles"].items())
    try:
        if entry == "forward_frames":
            frames = torch.from_numpy(synth.synth_frames(n, 1, 168, seed=7)).to(dev)
            if name.startswith("pixel_major"):
                frames = nchw_to_nhwc4(frames)
            acts = torch.from_numpy(synth.synth_actions(2 * n, 7, seed=3)[1]).to(dev)
            rec["feat"] = sha(trunk.forward_frames(frames, acts, p, 1, T, div))
        else:
            x = patches(n, p)
            if entry == "forward_map":
                fmap, feat = trunk.forward_map(x, T, div)
                rec["map"], rec["feat"] = sha(fmap), sha(feat)
            else:
                rec["feat"] = sha(trunk.forward(x, T, div))
            rec["launches"] = [(r["flops"], r["bytes"], r["tile"]) for r in trunk.profile(x, T, div)]
    except _lib.AdafError as e:      # a refused configuration is part of the fingerprint: code and message
        rec["error"] = str(e)
    print(json.dumps(rec, sort_keys=True), flush=True)


def main():
    with torch.no_grad():
        for arch in ("resnet50", "resnet101", "resnet152"):
            net = build(arch)
            for math in MATHS:
                net.set_math(math)
                for name, entry, n, p, cfg in cases(arch, math):
                    run(net, arch, math, name, entry, n, p, cfg)
            del net


if __name__ == "__main__":
    main()
