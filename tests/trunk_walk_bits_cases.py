"""One step of the trunk's training walk per case, as bits: the cases behind tests/test_trunk_walk_bits_gpu.py and
tools/trunk_walk_bits.py.  The nets, inputs and seeds are those of tests/test_trunk_backward_gpu.py (frozen BatchNorm statistics, 8 patches)
and tests/test_stage0_gpu.py (batch statistics, 4 patches); on the smallest case of each form also the two patterns of requires_grad where
the two forms differ most in what they skip."""
import hashlib

import torch

from adafocus_amd import _lib as L
from adafocus_amd.utils import nchw_to_nhwc4
from tests import test_stage0_gpu as BS
from tests import test_trunk_backward_gpu as FZ

PATTERNS = {"all": lambda k, p: True, "layer4": lambda k, p: k.startswith("layer4."), "bn_affine": lambda k, p: p.dim() == 1}
# case -> (the test module that owns the net and the inputs, its tag, the pattern of requires_grad)
CASES = {"frozen/%s/all" % t: (FZ, t, "all") for t in FZ.CASES}
CASES.update({"batch/%s/all" % t: (BS, t, "all") for t in BS.CASES})
CASES.update({"frozen/r50_64/%s" % p: (FZ, "r50_64", p) for p in ("layer4", "bn_affine")})
CASES.update({"batch/r50/%s" % p: (BS, "r50", p) for p in ("layer4", "bn_affine")})


def device_cus(dev):
    return int(L.load_library().adaf_device_cus(L.handle(dev)))


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digest(name, dev):
    """{"features" | "grad/<parameter>" | "stat/<running statistic>" (batch statistics: after the step): sha256 of the tensor's bytes}."""
    mod, tag, pattern = CASES[name]
    sd, x, dfeat = mod._inputs(tag)
    net = mod._net(tag, dev)
    net.set_trainable(True)
    for k, p in net.named_parameters():
        p.requires_grad_(not k.startswith("fc.") and PATTERNS[pattern](k, p))
    feat = net.features_train_nhwc4(nchw_to_nhwc4(x.to(dev)))
    feat.backward(dfeat.to(dev))
    torch.cuda.synchronize()
    out = {"features": _sha(feat)}
    for k, p in net.named_parameters():
        assert (p.grad is not None) == p.requires_grad, k
        if p.grad is not None:
            out["grad/" + k] = _sha(p.grad)
    if mod is BS:
        out.update({"stat/" + k: _sha(v) for k, v in net.state_dict().items() if "running" in k})
    return out


def digests(dev):
    return {name: digest(name, dev) for name in CASES}
