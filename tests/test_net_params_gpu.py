"""GPU tests of the weight side the three network objects share (csrc/adaf_net.h: parameter table, weight arena, conv + BN packer):
what finalize refuses (a missing parameter, a wrong size) and that the object recovers, reloading other weights into one object under
every arithmetic, the trunk changing depth in place, that the registered tensors are not needed once load() has returned, the
lifetime rule of a registration at the C ABI (it ends when the next finalize returns), and the one depthwise weight permutation.

The code under test is the host's packing, not a kernel's tiling: every network runs 2 images at the smallest size its entry point
takes (EfficientNet-B0 at 96^2, the smallest tests/test_effnet.py runs it at).  A reference is always a FRESH object loaded once;
identity is torch.equal."""
import functools

import pytest
import torch

from adafocus_amd import _lib, hip_ops, synth
from adafocus_amd.utils import nchw_to_nhwc4
from tests.helpers import rnd

pytestmark = pytest.mark.gpu
E_BADARG, E_STATE = "(-1)", "(-5)"
A, B = 4101, 4102            # two weight seeds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _synth(module):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")}
    return lambda seed: {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()}


@functools.lru_cache(maxsize=None)
def _cpu_params(net, seed):
    """The engine's parameter dict (CPU tensors, never modified) of network `net` ("trunk", "trunk101", "mbv2", "effnet")."""
    if net.startswith("trunk"):
        from adafocus_amd import resnet
        return _synth(getattr(resnet, "resnet101" if net == "trunk101" else "resnet50")())(seed)
    if net == "mbv2":
        from adafocus_amd.glancer_hip import neutral_params
        from adafocus_amd.mobilenet import mobilenet_v2
        return neutral_params(_synth(mobilenet_v2())(seed), "act")
    from adafocus_amd.efficientnet import EfficientNet
    m = EfficientNet.from_name("efficientnet-b0", num_classes=10)
    return m._neutral({k: v for k, v in _synth(m)(seed).items() if not k.startswith("_fc.")})


def _params(dev, net, seed):
    """Fresh device copies (a test may overwrite them)."""
    return {k: v.to(dev).clone() for k, v in _cpu_params(net, seed).items()}


NETS = {     # name: (late key to drop, first conv's weight)
    "trunk": ("layer4.2.bn3.running_var", "conv1.weight"),
    "mbv2": ("b17.project.bn.bias", "stem.weight"),
    "effnet": ("b15.se_expand.bias", "stem.weight"),
}
ARITH = [("trunk", "f32"), ("trunk", "split_bf16"), ("trunk", "f16"), ("mbv2", "f32"), ("effnet", "f32"), ("effnet", "f16")]


def _make(dev, net, arith="f32"):
    if net.startswith("trunk"):
        e = hip_ops.ResNet50Trunk(dev)
        e.set_math(arith)
    elif net == "mbv2":
        e = hip_ops.MobileNetV2Net(dev)
    else:
        e = hip_ops.EffNetNet(dev, 1.0, 1.0)
        e.set_dtype(arith)
    return e


@functools.lru_cache(maxsize=None)
def _input(net):
    return nchw_to_nhwc4(rnd((2, 3, 96 if net == "effnet" else 32, 96 if net == "effnet" else 32), 4200).cuda())


def _run(e, net):
    """Every output of one forward, as a tuple of clones."""
    x = _input("trunk" if net.startswith("trunk") else net)
    if net.startswith("trunk"):
        out = (e.forward(x),)
    elif net == "mbv2":
        out = e.forward(x)
    else:
        out = (e.forward(x, 0, want_map=False, want_vec=True)[1],)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)
    return tuple(t.clone() for t in out)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


_REF = {}


def _fresh(dev, net, seed, arith="f32"):
    """Outputs of a fresh object loaded once with (net, seed) under `arith`; computed once, shared, never modified."""
    key = (net, seed, arith)
    if key not in _REF:
        e = _make(dev, net, arith)
        e.load(_params(dev, net, seed))
        _REF[key] = _run(e, net)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1-3. what finalize / forward refuse
@pytest.mark.parametrize("net", list(NETS))
def test_missing_parameter_is_named_and_the_object_recovers(dev, net):
    late = NETS[net][0]
    p = _params(dev, net, A)
    assert late in p
    del p[late]
    e = _make(dev, net)
    with pytest.raises(_lib.AdafError) as ei:
        e.load(p)
    assert E_STATE in str(ei.value) and late in str(ei.value) and "missing parameter" in str(ei.value)
    e.load(_params(dev, net, A))
    assert _same(_run(e, net), _fresh(dev, net, A))


@pytest.mark.parametrize("net", list(NETS))
def test_wrong_size_names_the_key_and_both_counts(dev, net):
    first = NETS[net][1]
    p = _params(dev, net, A)
    want = p[first].numel()
    p[first] = p[first].flatten()[:-1].clone()
    e = _make(dev, net)
    with pytest.raises(_lib.AdafError) as ei:
        e.load(p)
    msg = str(ei.value)
    assert E_BADARG in msg and "'%s' has %d elements, expected %d" % (first, want - 1, want) in msg


@pytest.mark.parametrize("net", list(NETS))
def test_forward_before_any_load(dev, net):
    e = _make(dev, net)
    with pytest.raises(_lib.AdafError, match=r"\(-5\)"):
        _run(e, net)


# ------------------------------------------------------------------------------------------------ 4. packed buffers are reused
@pytest.mark.parametrize("net,arith", ARITH)
def test_reload_a_b_a_on_one_object(dev, net, arith):
    assert not _same(_fresh(dev, net, A, arith), _fresh(dev, net, B, arith))       # the two sets really differ
    e = _make(dev, net, arith)
    for seed in (A, B, A):
        e.load(_params(dev, net, seed))
        assert _same(_run(e, net), _fresh(dev, net, seed, arith)), seed


# ------------------------------------------------------------------------------------------------ 5. the trunk changes depth in place
def test_trunk_depth_50_101_50_on_one_object(dev):
    """The depth comes from the names of the CURRENT registration: after ResNet-101, a ResNet-50 load builds the 50 plan again.
    (Before the table was cleared by finalize, the stale layer3.6. .. layer3.22. names kept the 101 plan, over freed pointers.)"""
    e = _make(dev, "trunk")
    for net, convs in (("trunk", 53), ("trunk101", 104), ("trunk", 53)):
        e.load(_params(dev, net, A))
        assert _same(_run(e, net), _fresh(dev, net, A)), net
        assert e.n_launches == convs + 2
        e.set_tiles([0] * convs)
        with pytest.raises(_lib.AdafError):
            e.set_tiles([0] * (convs + 1))


# ------------------------------------------------------------------------------------------------ 6. sources are not needed afterwards
@pytest.mark.parametrize("net", list(NETS))
def test_registered_tensors_are_not_read_after_load(dev, net):
    p = _params(dev, net, A)
    e = _make(dev, net)
    e.load(p)
    before = _run(e, net)
    for t in p.values():
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    assert _same(_run(e, net), before) and _same(before, _fresh(dev, net, A))
    if net == "trunk":       # the other arithmetics derive their filters from the packed copy, not from the sources
        for arith in ("f16", "split_bf16"):
            e.set_math(arith)
            assert _same(_run(e, net), _fresh(dev, net, A, arith)), arith


# ------------------------------------------------------------------------------------------------ 7. the lifetime rule at the C ABI
def test_a_registration_ends_when_finalize_returns(dev):
    lib = _lib.load_library()
    ef = _make(dev, "effnet")
    ef.load(_params(dev, "effnet", A))
    _lib.check(lib.adaf_effnet_set_dtype(ef._net, _lib.DTYPE_F16), ef._h)
    with pytest.raises(_lib.AdafError) as ei:
        _lib.check(lib.adaf_effnet_finalize(ef._net, _lib.stream_ptr()), ef._h)
    assert E_STATE in str(ei.value) and "missing parameter" in str(ei.value)
    ef.set_dtype("f16")      # the Python path registers the full set again
    ef.load(_params(dev, "effnet", A))
    assert _same(_run(ef, "effnet"), _fresh(dev, "effnet", A, "f16"))

    tr = _make(dev, "trunk")
    tr.load(_params(dev, "trunk", A))
    w = _params(dev, "trunk", B)["conv1.weight"]
    _lib.check(lib.adaf_resnet50_set_param(tr._net, b"conv1.weight", _lib.ptr(w), w.numel()), tr._h)
    with pytest.raises(_lib.AdafError) as ei:
        _lib.check(lib.adaf_resnet50_finalize(tr._net, _lib.stream_ptr()), tr._h)
    assert E_STATE in str(ei.value) and "missing parameter" in str(ei.value)
    tr.load(_params(dev, "trunk", A))
    assert _same(_run(tr, "trunk"), _fresh(dev, "trunk", A))


# ------------------------------------------------------------------------------------------------ 8. one depthwise permutation
@pytest.mark.parametrize("c", [20, 288])
def test_depthwise_pack_3x3_is_the_kxk_pack(dev, c):
    w = rnd((c, 1, 3, 3), 4300 + c).to(dev)
    a, b = hip_ops.pack_dw_weight(w), hip_ops.pack_dw_weight_kxk(w)
    assert torch.equal(a.reshape(9, c), b.reshape(9, c))
    assert torch.equal(b, w.reshape(c, 9).t())
