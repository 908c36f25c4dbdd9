"""GPU tests of the ResNet-101 / ResNet-152 local CNN on the HIP trunk (the adaf_resnet50_* object at the depths {3,4,23,3} / {3,8,36,3}):
the real reference's features and logits (tests/golden/g16_resnet_depths.npz, tools/gen_golden_depths.py), make_temporal_shift's n_round
rule in every launch form (fused stage-1 tail with an unshifted / shifted next conv1, the lean shifted conv1, position-major tiles), the
bit identity of every alternative plan, the split-bf16 and fp16 arithmetics, and the refusal of a depth the library does not know."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib, synth
from tests.helpers import golden, rnd, synth_sd
from tests.test_f16_trunk import CONTRACT_TOL, SPREAD_FACTOR, _conv_bn, _h, _rel_rms, _shift

pytestmark = pytest.mark.gpu

TOL = 1e-3           # against the reference, relative to max(1, |reference|max): these features reach a few hundred
G = "g16_resnet_depths"
ARCH = {"r101": "resnet101", "r152": "resnet152"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g16():
    return golden(G)


def _close(got, ref, tol=TOL):
    ref = np.asarray(ref)
    err = np.abs(np.asarray(got) - ref).max()
    return err < tol * max(1.0, float(np.abs(ref).max())), err


def _tsn(dev, arch, place="blockres", div=8, seed=1616, segments=4, math="f32"):
    """TSN with the reference's own spelling of its keys and the generator's weights (synth over those keys)."""
    from adafocus_amd.tsn import TSN
    net = TSN(segments, "RGB", base_model=arch, is_shift=True, shift_div=div, shift_place=place)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()}, strict=True)
    net.base_model.set_math(math)
    return net.eval().to(dev)


def _feat(net, x, dev):
    from adafocus_amd.utils import nchw_to_nhwc4
    with torch.no_grad():
        return net.features_nhwc4(nchw_to_nhwc4(x.to(dev))).clone()


# ---------------------------------------------------------------------------------------------------- 1. the reference's features
@pytest.mark.parametrize("d", ["r101", "r152"])
def test_trunk_features_golden(dev, g16, d):
    """TSN.forward(no_reshape=True) for 'blockres' (shift_div 8 and 4: n_round = 2) and 'block', then the unshifted get_featmap."""
    from adafocus_amd import resnet
    x = rnd((8, 3, 96, 96), int(g16["seed_in"][0])).to(dev)
    for tag, place, div in (("blockres8", "blockres", 8), ("blockres4", "blockres", 4), ("block", "block", 8)):
        net = _tsn(dev, ARCH[d], place, div)
        with torch.no_grad():
            got = net(x, no_reshape=True).cpu().numpy()
        ok, err = _close(got, g16["%s_%s" % (d, tag)])
        print("%s %s: max |diff| %.2e" % (d, tag, err))
        assert ok, (d, tag, err)
    plain = getattr(resnet, ARCH[d])()
    shapes = {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    plain.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1616).items()}, strict=True)
    plain = plain.eval().to(dev)
    with torch.no_grad():
        pooled = plain.get_featmap(x, pooled=True).cpu().numpy().reshape(8, -1)
        fmap = plain.get_featmap(x[:1], pooled=False).cpu().numpy()
    assert fmap.shape == g16[d + "_map"].shape
    for tag, got in (("pooled", pooled), ("map", fmap)):
        ok, err = _close(got, g16["%s_%s" % (d, tag)])
        assert ok, (d, tag, err)


def _sth_model(dev, arch):
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.gpu, a.base_model = 0, arch
    m = GFV(a).eval()
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])  # evaluate.py:83
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    pol = {k[len("policy."):]: v for k, v in synth_sd("STH_POLICY", 1007).items()}
    for p in (m.focuser.policy.policy_old, m.focuser.policy.policy):
        p.load_state_dict(pol)
        p.eval()
    return m.to(dev), a


def test_sth_gfv_resnet101_golden(dev, g16):
    """GFV(args) with args.base_model = 'resnet101' (config 4: Tg = Tf = 8, P = 128, B = 2): action_stage2 logits with the policy's own
    action and with a forced one against the reference; the crop actions sit >= 0.02 px from a pixel boundary and match it, and they are
    the ResNet-50 model's actions bit for bit (the policy reads the glancer only)."""
    m, a = _sth_model(dev, "resnet101")
    m50, _ = _sth_model(dev, "resnet50")
    gl = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=3)).to(dev)
    fo = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=4)).view(2, 8, 3, 224, 224).to(dev)
    forced = torch.from_numpy(g16["sth_forced_action"]).to(dev)
    acts = []
    with torch.no_grad():
        for mm in (m, m50):
            fm, glog = mm.glance(gl)
            acts.append(mm.focuser.policy.policy_old.act_nhwc(fm.permute(0, 1, 3, 4, 2).reshape(16, 7, 7, 1280), 2, 8).clone())
        fm, glog = m.glance(gl)
        pred, _, _ = m.action_stage2(fo, fm, glog, 0, a, prev_local_patch=None, training=False, with_baseline=False)
        pred_f, _, _ = m.action_stage2(fo, fm, glog, 0, a, prev_local_patch=None, training=False, forced_action=forced)
    assert g16["sth_policy_action_px_margin"].min() >= 0.02
    assert np.abs(acts[0].cpu().numpy() - g16["sth_policy_action"]).max() < 1e-4
    assert torch.equal(acts[0], acts[1])
    for got, key in ((pred, "sth_logits"), (pred_f, "sth_logits_forced")):
        ok, err = _close(got.cpu().numpy(), g16[key])
        print("%s: max |diff| %.2e" % (key, err))
        assert ok, (key, err)


def test_validate_sth_resnet101_uint8_clips(dev):
    """evaluate.validate_sth with base_model = 'resnet101' on stacked uint8 clips: torch.equal to the same clips normalised on the host."""
    from adafocus_amd import evaluate as E
    from oracle import ref_model as O
    m, a = _sth_model(dev, "resnet101")
    a.batch_size, a.glance_size = 2, 224
    labels = torch.tensor([5, 100, 7])

    class DS:
        def __init__(self, g_, f_):
            self.g, self.f = g_, f_

        def __len__(self):
            return len(self.g)

        def __getitem__(self, i):
            return self.g[i], self.f[i], labels[i]

    gen = np.random.Generator(np.random.PCG64([23, 101]))
    gu = gen.integers(0, 256, size=(3, 224, 224, 24), dtype=np.uint8)
    fu = gen.integers(0, 256, size=(3, 224, 224, 24), dtype=np.uint8)
    gf = torch.stack([O.ingest_uint8(v) for v in gu])
    ff = torch.stack([O.ingest_uint8(v) for v in fu])
    torch.manual_seed(11)
    r8 = E.validate_sth(DS(torch.from_numpy(gu), torch.from_numpy(fu)), m, torch.nn.CrossEntropyLoss(), a, quiet=True, return_logits=True)
    torch.manual_seed(11)
    r32 = E.validate_sth(DS(gf, ff), m, torch.nn.CrossEntropyLoss(), a, quiet=True, return_logits=True)
    assert r8[4].shape == (3, 174) and torch.isfinite(r8[4]).all()
    assert torch.equal(r8[4], r32[4]) and r8[:2] == r32[:2]


# ---------------------------------------------------------------------------------------------------- 2. bit identity of the plans
def test_resnet101_plans_bit_identical(dev):
    """1024 patches of 96^2 in clips of 8 ('blockres', n_round = 2): the fused stage-1 tail carries an unshifted next conv1 (layer1.0)
    and a shifted one (layer1.1) on position-major tiles.  Run to run, fusion off, and batch position (a clip alone, where the small
    plan runs) all give the same bits."""
    net = _tsn(dev, "resnet101", segments=8, seed=1017)
    x = rnd((1024, 3, 96, 96), 1018)
    big = _feat(net.base_model, x, dev)
    assert torch.isfinite(big).all() and big.abs().max().item() > 0.1
    assert torch.equal(big, _feat(net.base_model, x, dev))
    assert torch.equal(big[8:24], _feat(net.base_model, x[8:24], dev))
    net.base_model.set_fusion(False)
    off = _feat(net.base_model, x, dev)
    net.base_model.set_fusion(True)
    assert torch.equal(big, off)
    # the same weights without the shift are another network (the shift is live in the kept blocks)
    net.base_model.tsm_segments = 0
    assert (_feat(net.base_model, x[:8], dev) - big[:8]).abs().max().item() > 1e-2


def test_resnet152_latency_form_and_frames(dev):
    """16 patches without a shift: the small-batch form equals the batched plan.  forward_frames (the stem gathers the windows) equals
    the gather launch followed by the trunk."""
    from adafocus_amd.resnet import resnet152
    from adafocus_amd.utils import get_patch_nhwc4, nchw_to_nhwc4
    net = resnet152()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1520).items()}, strict=True)
    net = net.eval().to(dev)
    x = nchw_to_nhwc4(rnd((16, 3, 96, 96), 1521).to(dev))
    with torch.no_grad():
        lat = net.features_nhwc4(x).clone()
        net._sync().set_latency_rows(0)
        batched = net.features_nhwc4(x).clone()
        net._sync().set_latency_rows(-1)
    assert torch.isfinite(lat).all() and torch.equal(lat, batched)
    frames = rnd((300, 3, 224, 224), 1522).to(dev)
    act = torch.from_numpy(np.random.Generator(np.random.PCG64(1523)).random((300, 2), dtype=np.float32)).to(dev)
    with torch.no_grad():
        got = net.features_from_frames(frames, act, 96).clone()
        ref = net.features_nhwc4(get_patch_nhwc4(frames, act, 96, 1))
    assert torch.equal(got, ref)


def test_resnet101_frames_with_shift(dev):
    """forward_frames with one action per clip of 8 and the n_round shift: torch.equal to gather-then-trunk."""
    from adafocus_amd.utils import get_patch_nhwc4
    net = _tsn(dev, "resnet101", segments=8, seed=1019).base_model
    frames = rnd((264, 3, 224, 224), 1020).to(dev)
    act = torch.from_numpy(np.random.Generator(np.random.PCG64(1021)).random((33, 2), dtype=np.float32)).to(dev)
    with torch.no_grad():
        got = net.features_from_frames(frames, act, 128, frames_per_action=8).clone()
        ref = net.features_nhwc4(get_patch_nhwc4(frames, act, 128, 8))
    assert torch.isfinite(got).all() and torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------- 3. the other arithmetics
def test_split_bf16_resnet101_golden(dev, g16):
    x = rnd((8, 3, 96, 96), int(g16["seed_in"][0])).to(dev)
    net = _tsn(dev, "resnet101", math="split_bf16")
    with torch.no_grad():
        got = net(x, no_reshape=True).cpu().numpy()
    ok, err = _close(got, g16["r101_blockres8"])
    assert ok, err


def _contract_trunk(sd, x, layers, tsm=0, div=8):
    """tests/test_f16_trunk.contract_trunk at any Bottleneck depth, 'blockres' with make_temporal_shift's n_round."""
    n_round = 2 if layers[2] >= 23 else 1
    y = F.relu(_conv_bn(sd, "conv1", "bn1", x, 2, 3))
    y = _h(F.max_pool2d(y, 3, 2, 1))
    for li, (nblk, stride) in enumerate(zip(layers, (1, 2, 2, 2)), start=1):
        for b in range(nblk):
            p = "layer%d.%d" % (li, b)
            s = stride if b == 0 else 1
            z = _shift(y, tsm, div) if tsm and b % n_round == 0 else y
            z = _h(F.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", z)))
            z = _h(F.relu(_conv_bn(sd, p + ".conv2", p + ".bn2", z, s, 1)))
            z = _conv_bn(sd, p + ".conv3", p + ".bn3", z)
            idn = _h(_conv_bn(sd, p + ".downsample.0", p + ".downsample.1", y, s)) if b == 0 else y
            y = _h(F.relu(z + idn))
    return y.mean((2, 3))


@pytest.mark.parametrize("d", ["r101", "r152"])
def test_f16_against_contract_and_f32(dev, d):
    """ADAF_MATH_F16 with the n_round shift (T = 4, shift_div 8): within the DESIGN 3.9 self-distance bound of the contract model AT THIS
    DEPTH -- max(2e-4, 1.5 x the distance between the contract model accumulated in fp32 and in fp64) -- and close to the fp32 trunk."""
    from adafocus_amd import resnet
    layers = resnet.DEPTHS[ARCH[d]]
    net = getattr(resnet, ARCH[d])()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1616).items()}
    net.load_state_dict(sd, strict=True)
    net = net.eval().to(dev)
    net.tsm_segments, net.tsm_div = 4, 8
    x = rnd((8, 3, 64, 64), 1617)
    f32 = _feat(net, x, dev).cpu()
    net.set_math("f16")
    f16 = _feat(net, x, dev).cpu()
    with torch.no_grad():
        ref = _contract_trunk(sd, x, layers, tsm=4)
        ref64 = _contract_trunk({k: v.double() for k, v in sd.items()}, x.double(), layers, tsm=4)
    bound = max(CONTRACT_TOL, SPREAD_FACTOR * _rel_rms(ref, ref64))
    err, err32 = _rel_rms(f16, ref), _rel_rms(f16, f32)
    print("%s fp16: contract rel rms %.2e (bound %.2e), vs fp32 %.2e" % (d, err, bound, err32))
    assert torch.isfinite(f16).all() and err <= bound, (err, bound)
    assert err32 <= 1e-2, err32


# ---------------------------------------------------------------------------------------------------- 4. depths the library refuses
def test_unknown_depth_is_refused(dev):
    """layer3.0 - layer3.9 only ({3, 4, 10, 3}): finalize refuses it, naming the counts it found."""
    from adafocus_amd import hip_ops
    from adafocus_amd.resnet import resnet101
    sd = {k: v for k, v in resnet101().state_dict().items()
          if not (k.startswith("layer3.") and int(k.split(".")[1]) >= 10)}
    trunk = hip_ops.ResNet50Trunk(dev)
    with pytest.raises(_lib.AdafError, match=r"3, 4, 10, 3"):
        trunk.load({k: v.to(dev) for k, v in sd.items()})
