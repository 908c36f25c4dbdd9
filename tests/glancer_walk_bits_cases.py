"""One step of the glancer's training walk per case, as bits: the cases behind tests/test_glancer_walk_bits_gpu.py and
tools/glancer_walk_bits.py.  The net, its state and the inputs are those of tests/test_glancer_train_gpu.py (4 frames of 64 x 64, both
kinks of the ReLU6 met, one BatchNorm gamma at 0); the patterns of requires_grad are everything, the last block with the head (the
data-gradient chain stops there), and the BatchNorm affines alone (no weight gradient anywhere)."""
import torch

from adafocus_amd.utils import nchw_to_nhwc4
from tests import test_glancer_train_gpu as G
from tests.trunk_walk_bits_cases import _sha, device_cus  # noqa: F401

CASES = {
    "all": lambda k, p: True,
    "tail": lambda k, p: k.startswith(("features.17.", "features.18.")),
    "bn_affine": lambda k, p: p.dim() == 1,
}


def digest(name, dev):
    """{"features" | "grad/<parameter>" | "stat/<running statistic>" (after the step): sha256 of the tensor's bytes}."""
    x, dfeat = G._inputs()
    net = G._train(G._net(dev))
    for k, p in net.named_parameters():
        p.requires_grad_(k.startswith("features.") and CASES[name](k, p))
    feat = net.features_train_nhwc4(nchw_to_nhwc4(x.to(dev)))
    feat.backward(dfeat.to(dev))
    torch.cuda.synchronize()
    out = {"features": _sha(feat)}
    for k, p in net.named_parameters():
        assert (p.grad is not None) == p.requires_grad, k
        if p.grad is not None:
            out["grad/" + k] = _sha(p.grad)
    out.update({"stat/" + k: _sha(v) for k, v in net.state_dict().items() if "running" in k})
    return out


def digests(dev):
    return {name: digest(name, dev) for name in CASES}
