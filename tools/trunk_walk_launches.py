#!/usr/bin/env python3
"""The launches of the trunk's training walk (adafocus_amd/trunk_train.py), recorded on the host: the walk is orchestration over hip_ops,
so with ``hip_ops._call`` replaced by a recorder, ``hip_ops._workspace`` by a stub and ``_lib.need_gpu_f32`` by a no-op the real wrappers run
their shape logic on CPU tensors and ``net.features_train_nhwc4(x).backward(dfeat)`` completes without a GPU.  Per case: every C-ABI call
with its symbol, its scalars, the ConvParams fields and its tensor operands.  Two versions of the walk that skip the same launches and hand
every launch the same operands print the same digests, whatever the order of independent launches.

A tensor operand is named by what produced it, not by when it was first seen: parameters and buffers by their state-dict name, the patches
and d(features) by role, a workspace as "ws"; a tensor a call sees for the first time is an output of that call, named by a hash of (symbol,
scalars, the names of the call's inputs, its argument position).  Tensors are keyed by storage pointer and kept alive while a case records.
A case's canonical form is the sorted list of its launch lines, its digest the sha256 of that list.

Only ResNet's public surface and the three replacements are used, so the file runs unchanged against another version of the walk.  The
recording of the walk before its two copies were merged is tests/golden/trunk_walk_launches.json; it is not regenerated from later code.

Usage:  python tools/trunk_walk_launches.py > launches.json          {case: {"digest", "counts": {symbol: launches}}}
        python tools/trunk_walk_launches.py --dump CASE              the sorted launch lines of one case (diff two versions' dumps)"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from adafocus_amd import _lib, hip_ops, resnet  # noqa: E402

N, P = 2, 32
FORMS = ("frozen", "batch")
SHIFTS = {"noshift": (0, "blockres"), "blockres": (2, "blockres"), "block": (2, "block")}
# which trunk parameters require grad (fc is no part of the walk and never does)
PATTERNS = {
    "all": lambda k, p: True,
    "layer4": lambda k, p: k.startswith("layer4."),
    "bn_affine": lambda k, p: p.dim() == 1,
    "mid_conv": lambda k, p: k == "layer2.1.conv1.weight",
    "downsample": lambda k, p: k == "layer1.0.downsample.0.weight",
    "none": lambda k, p: False,
}
# case -> (arch, form, shift, pattern); ResNet-101 has n_round == 2: every other block of a stage is unshifted
CASES = {"%s/%s/%s" % (f, s, r): ("resnet50", f, s, r) for f in FORMS for s in SHIFTS for r in PATTERNS}
CASES.update({"%s/r101_blockres/all" % f: ("resnet101", f, "blockres", "all") for f in FORMS})


def _hash(*parts):
    return hashlib.sha256("\x1f".join(parts).encode()).hexdigest()[:16]


class Recorder:
    """Stands in for hip_ops._call: one line per C-ABI call."""

    def __init__(self, named):
        self.lines, self.symbols, self.keep = [], [], []
        self.label = {}
        for name, t in named.items():
            self.name(t, name)

    def name(self, t, label):
        self.keep.append(t)
        self.label[t.untyped_storage().data_ptr()] = label

    def workspace(self, query, device, *extents):
        ws = torch.empty(4, dtype=torch.float32)
        self.name(ws, "ws")
        return ws, 0

    def call(self, sym, where, *args, stream=True):
        shown, new = [], []
        for i, a in enumerate(args):
            if isinstance(a, torch.Tensor):
                label = self.label.get(a.untyped_storage().data_ptr())
                if label is None:
                    new.append(i)
                shown.append(label)
            elif a is None:
                shown.append("null")
            elif hasattr(a, "_obj"):            # ctypes.byref(ConvParams)
                shown.append("{%s}" % ",".join("%s=%d" % (f, getattr(a._obj, f)) for f, _ in a._obj._fields_))
            elif isinstance(a, C._SimpleCData):
                shown.append(repr(a.value))
            else:
                shown.append(repr(a))
        given = [s if s is not None else "out" for s in shown]
        for i in new:
            shown[i] = "out:" + _hash(sym, str(i), *given)
            self.name(args[i], shown[i])
        self.lines.append("%s(%s)" % (sym, ", ".join(shown)))
        self.symbols.append(sym)

    def patches(self):
        """(object, attribute, replacement): what a recording replaces, for monkeypatch.setattr or `patched`."""
        return [(hip_ops, "_call", self.call), (hip_ops, "_workspace", self.workspace), (_lib, "need_gpu_f32", lambda *t: None)]


@contextlib.contextmanager
def patched(rec):
    saved = [(o, k, getattr(o, k)) for o, k, _ in rec.patches()]
    try:
        for o, k, v in rec.patches():
            setattr(o, k, v)
        yield rec
    finally:
        for o, k, v in saved:
            setattr(o, k, v)


_NETS = {}


def prepare(case):
    """-> (net in the case's mode, patches, dfeat, the names that require grad, a Recorder that knows the case's named tensors)."""
    arch, form, shift, pattern = CASES[case]
    if arch not in _NETS:
        _NETS[arch] = getattr(resnet, arch)()
    net = _NETS[arch]
    net.train(form == "batch")
    net.set_math("f32")
    net.set_trainable(True)
    net.set_bn_batch_stats(form == "batch")
    net.tsm_segments, net.tsm_div, net.tsm_place = SHIFTS[shift][0], 8, SHIFTS[shift][1]
    net.zero_grad(set_to_none=True)
    want = set()
    for k, p in net.named_parameters():
        p.requires_grad_(not k.startswith("fc.") and PATTERNS[pattern](k, p))
        if p.requires_grad:
            want.add(k)
    g = torch.Generator().manual_seed(7)
    x4 = torch.randn((N, P, P, 4), generator=g)
    dfeat = torch.randn((N, 2048), generator=g)
    named = dict(net.state_dict(keep_vars=True), patches=x4, dfeat=dfeat)
    return net, x4, dfeat, want, Recorder(named)


def run(net, x4, dfeat):
    """One step of the walk; -> the names of the parameters that received a .grad."""
    feat = net.features_train_nhwc4(x4)
    if feat.requires_grad:
        feat.backward(dfeat)
    return {k for k, p in net.named_parameters() if p.grad is not None}


def summary(rec):
    counts = {}
    for s in rec.symbols:
        counts[s] = counts.get(s, 0) + 1
    return {"digest": hashlib.sha256("\n".join(sorted(rec.lines)).encode()).hexdigest(), "counts": counts}


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
        print(json.dumps(digests(), indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
