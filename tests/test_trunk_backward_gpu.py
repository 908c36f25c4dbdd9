"""The differentiable walk of the ResNet trunk on the MI355X (adafocus_amd/trunk_train.py): its features equal the eval
engine's bit for bit, and the gradient of EVERY trunk parameter for a random upstream d(features) is held to a torch-CPU restatement of
the trunk with eval BatchNorm in fp64.

Tolerance: error against the fp64 result, relative to that quantity's largest entry, at most 50x the distance between the same CPU
autograd in fp32 and in fp64 (G17's rule, tests/test_stage3_gpu.py).

The branch at a ReLU whose input is zero to within fp32 rounding.  The gradient of the trunk is piecewise constant in its ReLU masks,
and every case has ten to twenty units in its small maps (5 x 5 and below) whose fp64 pre-activation is smaller than the fp32 forward
error of that map: there an fp32 forward may land on either side of zero (the CPU's own fp32 run takes another branch than its fp64 run at
one to three units in three of the four cases), and one such unit on a 2 x 2 or 4 x 4 map moves the gradients in front of it by 1e-3 to
1e-2 of their largest entry.  Both branches are correct fp32 behaviour, so the yardstick is the fp64 gradient ON THE BRANCHES THE DEVICE
TOOK: the test reads the walk's stored layer outputs, asserts that every unit whose sign differs from the fp64 forward's has an fp64
pre-activation of at most 50x the measured fp32-vs-fp64 forward error of its map (anything else is a wrong forward), and evaluates the
fp64 reference with those masks.  Where no unit differs it is the plain fp64 autograd result.  The spread is always that of the plain
fp32 and fp64 runs."""
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import resnet, synth
from adafocus_amd.utils import nchw_to_nhwc4
from tests.helpers import rnd
from tests.test_f16_trunk import _shift
from tests.trunk_walk_harness import SPREAD_FACTOR, _device_branches, _run, check_features_and_gradients  # noqa: F401 (SPREAD_FACTOR: tests/test_stage1_gpu.py)

pytestmark = pytest.mark.gpu

BN_EPS = 1e-5
# tag -> (arch, patch size, temporal shift segments (0 = none), placement, a (BatchNorm, channel) whose gamma is set to exactly 0)
CASES = {
    "r50_72_shift": ("resnet50", 72, 4, "blockres", ("layer2.0.bn2", 3)),
    "r50_64": ("resnet50", 64, 0, "blockres", None),
    "r101_64_shift": ("resnet101", 64, 4, "blockres", None),
    "r50_64_block": ("resnet50", 64, 4, "block", None),
}
N = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _cbn(p, conv, bn, x, stride=1, pad=0):
    y = F.conv2d(x, p[conv + ".weight"], stride=stride, padding=pad)
    scale = p[bn + ".weight"] / torch.sqrt(p[bn + ".running_var"] + BN_EPS)
    return y * scale.view(1, -1, 1, 1) + (p[bn + ".bias"] - p[bn + ".running_mean"] * scale).view(1, -1, 1, 1)


def _cpu_trunk(p, x, layers, tsm, div, place, pre=None, masks=None):
    """The trunk on the CPU with eval BatchNorm (tests/test_resnet_depths_gpu._contract_trunk without the fp16 roundings; 'block' puts
    the shift in front of every whole block).  pre: a dict that receives every ReLU's input by name ("stem", "<block>.z1", ".z2",
    ".y"); masks: name -> bool map that replaces the ReLU's own branch (z * mask in place of relu(z))."""
    def act(name, z):
        if pre is not None:
            pre[name] = z.detach()
        return F.relu(z) if masks is None else z * masks[name].to(z.dtype)

    n_round = 2 if layers[2] >= 23 else 1
    y = F.max_pool2d(act("stem", _cbn(p, "conv1", "bn1", x, 2, 3)), 3, 2, 1)
    for li, (nblk, stride) in enumerate(zip(layers, (1, 2, 2, 2)), start=1):
        for b in range(nblk):
            q = "layer%d.%d" % (li, b)
            s = stride if b == 0 else 1
            if tsm and place == "block":
                y = _shift(y, tsm, div)
            z = _shift(y, tsm, div) if tsm and place != "block" and b % n_round == 0 else y
            z = act(q + ".z1", _cbn(p, q + ".conv1", q + ".bn1", z))
            z = act(q + ".z2", _cbn(p, q + ".conv2", q + ".bn2", z, s, 1))
            z = _cbn(p, q + ".conv3", q + ".bn3", z)
            idn = _cbn(p, q + ".downsample.0", q + ".downsample.1", y, s) if b == 0 else y
            y = act(q + ".y", z + idn)
    return y.mean((2, 3))


def _is_param(k):
    return k.endswith((".weight", ".bias")) and not k.startswith("fc.")


_CACHE = {}


def _reference(tag, dt, masks=None):
    """CPU autograd of the case in `dt`: (features, {param name: grad}, {ReLU name: its input})."""
    arch, size, tsm, place, _ = CASES[tag]
    sd, x, dfeat = _inputs(tag)
    p = {k: (v.to(dt).requires_grad_(True) if _is_param(k) else v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    pre = {}
    feat = _cpu_trunk(p, x.to(dt), resnet.DEPTHS[arch], tsm, 8, place, pre=pre, masks=masks)
    names = [k for k in p if _is_param(k)]
    grads = torch.autograd.grad(feat, [p[k] for k in names], dfeat.to(dt))
    return feat.detach(), dict(zip(names, grads)), pre


def _inputs(tag):
    if ("in", tag) not in _CACHE:
        arch, size, tsm, place, zero = CASES[tag]
        net = getattr(resnet, arch)()
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1300 + len(tag)).items()}
        if zero is not None:
            sd[zero[0] + ".weight"][zero[1]] = 0.0
        _CACHE["in", tag] = (sd, rnd((N, 3, size, size), 1310 + len(tag)), rnd((N, 2048), 1320 + len(tag)))
    return _CACHE["in", tag]


def _case(tag):
    """-> (state dict, patches (N,3,P,P), dfeat, {dtype: (features, {param name: grad}, {ReLU name: input})}) -- the CPU reference,
    computed once."""
    if tag not in _CACHE:
        _CACHE[tag] = _inputs(tag) + ({dt: _reference(tag, dt) for dt in (torch.float64, torch.float32)},)
    return _CACHE[tag]


def _net(tag, dev):
    arch, size, tsm, place, _ = CASES[tag]
    sd = _inputs(tag)[0]
    net = getattr(resnet, arch)()
    net.load_state_dict(sd, strict=True)
    net = net.eval().to(dev)
    net.set_math("f32")          # pinned: training is fp32 only, whatever default the session's other modules run the trunk with
    net.tsm_segments, net.tsm_div, net.tsm_place = tsm, 8, place
    return net


@pytest.mark.parametrize("tag", list(CASES))
def test_features_and_every_gradient_against_fp64(dev, tag):
    sd, x, dfeat, ref = _case(tag)
    net = _net(tag, dev)
    with torch.no_grad():
        engine = net.features_nhwc4(nchw_to_nhwc4(x.to(dev))).clone()
    stats = {k: v.clone() for k, v in net.state_dict().items() if "running" in k}
    feat, grads = _run(net, x, dfeat, dev)
    assert torch.equal(feat, engine), "the training walk's features differ from the eval engine's in %d values" % int((feat != engine).sum())
    f64, g64, pre64 = ref[torch.float64]
    f32, g32, pre32 = ref[torch.float32]
    masks, differ = _device_branches(tag, net, x, dev, pre64, pre32)
    if differ:                       # the fp64 gradient on the branches the device took (module docstring)
        f64, g64, _ = _reference(tag, torch.float64, masks)
    check_features_and_gradients(tag, feat, grads, (f32, g32), (f64, g64), CASES[tag][4])
    for k, v in net.state_dict().items():
        if "running" in k:
            assert torch.equal(v, stats[k]), k                          # the BatchNorm statistics are never touched


def test_only_layer4_trainable_stops_the_chain(dev):
    """With only layer4 requiring grad, every earlier parameter keeps .grad None (no weight-gradient launch, and the data-gradient chain
    stops at layer4.0's input), and layer4's gradients are the all-trainable run's, bit for bit."""
    tag = "r50_72_shift"
    _, x, dfeat, _ = _case(tag)
    net = _net(tag, dev)
    _, full = _run(net, x, dfeat, dev)
    full = {k: v.clone() for k, v in full.items() if v is not None}
    for k, p in net.named_parameters():
        p.requires_grad_(k.startswith("layer4."))
    _, part = _run(net, x, dfeat, dev)
    for k, g in part.items():
        if k.startswith("layer4."):
            assert torch.equal(g, full[k]), k
        else:
            assert g is None, k


def test_training_walk_is_off_by_default_and_fp32_only(dev):
    tag = "r50_64"
    _, x, _, _ = _case(tag)
    net = _net(tag, dev)
    x4 = nchw_to_nhwc4(x.to(dev))
    with pytest.raises(RuntimeError, match="set_trainable"):
        net.features_train_nhwc4(x4)
    net.set_trainable(True)
    for mode in ("f16", "split_bf16"):
        net.set_math(mode)
        with pytest.raises(NotImplementedError, match=mode):
            net.features_train_nhwc4(x4)
    net.set_math("f32")
    net.train()
    with pytest.raises(RuntimeError, match="batch-statistics"):
        net.features_train_nhwc4(x4)
