#!/usr/bin/env python3
"""Bit-level fingerprint of the two MBConv networks' host walks (tools/trunk_digest.py is the same for the ResNet trunk): one JSON line
per case with the sha256 of the output bytes, so two builds of the library that take the same launch decisions and compute the same
bits print the same file.  EfficientNet-B3 in both storage types, fusion on and off: a native size with the stride-2 whole block
(144), dynamic padding (75 under 300), the smallest input in a batch of two half chunks (32 x 513), and every size at effnet_chunk = 4
with 9 frames (a pair of chunks and a tail) -- each as map + pooled vector and as the pooled vector alone (the head conv with the pool
in its epilogue).  MobileNetV2 at 224^2 and 64^2 with the strip forms on and off.  Weights and inputs are seeded (adafocus_amd.synth).
Usage: python tools/effnet_digest.py > digest.jsonl        (ADAF_LIB=<other build> in a fresh process for the other side; compare with cmp)"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import _lib, synth  # noqa: E402
from adafocus_amd.efficientnet import EfficientNet  # noqa: E402
from adafocus_amd.mobilenet import mobilenet_v2  # noqa: E402
from adafocus_amd.utils import nchw_to_nhwc4  # noqa: E402

dev = torch.device("cuda:0")
EFFNET_CASES = [(1024, size, pad, 513 if size == 32 else 3) for size, pad in ((144, 0), (75, 300), (32, 0))] + \
    [(4, size, pad, 9) for size, pad in ((144, 0), (75, 300), (32, 0))]       # (effnet_chunk, size, pad_size, n)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def frames(n, size):
    return nchw_to_nhwc4(torch.from_numpy(synth.synth_frames(n, 1, size, seed=100 + size)).to(dev))


def seeded(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()})
    return module.eval().to(dev)


def emit(**rec):
    print(json.dumps(rec, sort_keys=True), flush=True)


def main():
    with torch.no_grad():
        for dtype in ("f32", "f16"):
            m = seeded(EfficientNet.from_name("efficientnet-b3", num_classes=10, dtype=dtype), 1007)
            for fuse in (True, False):
                m.fusion = fuse
                eng = m.engine()
                for chunk, size, pad, n in EFFNET_CASES:
                    x = frames(n, size)
                    with _lib.option("effnet_chunk", chunk):
                        fmap, fvec = eng.forward(x, pad, want_map=True, want_vec=True)
                        _, pooled = eng.forward(x, pad, want_map=False, want_vec=True)
                        emit(net="effnet-b3", dtype=dtype, fuse=fuse, effnet_chunk=chunk, size=size, pad_size=pad, n=n,
                             whole_blocks=eng.whole_blocks(size, pad), fused_expand_blocks=eng.fused_expand_blocks(size, pad),
                             map=sha(fmap), vec=sha(fvec), pooled=sha(pooled))
            del m
        g = seeded(mobilenet_v2(), 3)
        for strip in (1, 0):
            with _lib.option("mb_strip", strip):
                for size in (224, 64):
                    fmap, fvec = g.features_from_nhwc4(frames(4, size))
                    emit(net="mobilenetv2", mb_strip=strip, size=size, n=4, map=sha(fmap), vec=sha(fvec))


if __name__ == "__main__":
    main()
