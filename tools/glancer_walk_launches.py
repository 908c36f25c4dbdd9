#!/usr/bin/env python3
"""The launches of the glancer's training walk (adafocus_amd/glancer_train.py), recorded on the host: what tools/trunk_walk_launches.py does
for the trunk, with that tool's Recorder, `patched` and `summary` -- ``hip_ops._call`` replaced by the recorder, ``hip_ops._workspace`` by a stub
and ``_lib.need_gpu_f32`` by a no-op, so that ``net.features_train_nhwc4(x).backward(dfeat)`` of a MobileNetV2 in train mode completes on CPU
tensors.  Per case: every C-ABI call with its symbol, its scalars, the ConvParams fields and its tensor operands named by what produced them;
a case's digest is the sha256 of its sorted launch lines.

The cases are patterns of requires_grad over ``features.*`` (the classifier is no part of the walk and never requires grad): everything; the
last block and the head; the BatchNorm affines; one depthwise filter in mid-network, where the data-gradient chain must stop; the project
of one block with use_res_connect; the stem's filter alone (the whole chain, every `add`, no data gradient at the stem); nothing.

Only MobileNetV2's public surface and the three replacements are used, so the file runs unchanged against another version of the walk.  The
recording of the walk before its layer treatment moved into the core it shares with the trunk is tests/golden/glancer_walk_launches.json; it
is not regenerated from later code.

Usage:  python tools/glancer_walk_launches.py > launches.json        {"cases": {case: {"digest", "counts": {symbol: launches}}}}
        python tools/glancer_walk_launches.py --dump CASE            the sorted launch lines of one case (diff two versions' dumps)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402

from adafocus_amd import mobilenet  # noqa: E402
from trunk_walk_launches import Recorder, patched, summary  # noqa: E402,F401

N, SIZE = 2, 64
CASES = {
    "all": lambda k, p: True,
    "tail": lambda k, p: k.startswith(("features.17.", "features.18.")),
    "bn_affine": lambda k, p: p.dim() == 1,
    "mid_dw": lambda k, p: k == "features.7.conv.1.0.weight",
    "res_project": lambda k, p: k == "features.3.conv.2.weight",
    "stem": lambda k, p: k == "features.0.0.weight",
    "none": lambda k, p: False,
}

_NET = []


def prepare(case):
    """-> (net in train mode with both opt-ins, frames, dfeat, the names that require grad, a Recorder that knows the named tensors)."""
    if not _NET:
        _NET.append(mobilenet.MobileNetV2())
    net = _NET[0]
    net.train()
    net.set_trainable(True)
    net.set_bn_batch_stats(True)
    net.zero_grad(set_to_none=True)
    want = set()
    for k, p in net.named_parameters():
        p.requires_grad_(k.startswith("features.") and CASES[case](k, p))
        if p.requires_grad:
            want.add(k)
    g = torch.Generator().manual_seed(7)
    x4 = torch.randn((N, SIZE, SIZE, 4), generator=g)
    dfeat = torch.randn((N, 1280), generator=g)
    named = dict(net.state_dict(keep_vars=True), frames=x4, dfeat=dfeat)
    return net, x4, dfeat, want, Recorder(named)


def run(net, x4, dfeat):
    """One step of the walk; -> the names of the parameters that received a .grad."""
    feat = net.features_train_nhwc4(x4)
    if feat.requires_grad:
        feat.backward(dfeat)
    return {k for k, p in net.named_parameters() if p.grad is not None}


def record(case):
    net, x4, dfeat, want, rec = prepare(case)
    with patched(rec):
        got = run(net, x4, dfeat)
    assert got == want, (case, sorted(got ^ want))
    return rec


def digests():
    return {case: summary(record(case)) for case in CASES}


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print("\n".join(sorted(record(sys.argv[2]).lines)))
    else:
        print(json.dumps({"cases": digests()}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
