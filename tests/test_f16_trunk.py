"""GPU tests of the opt-in fp16 ResNet-50 trunk (ADAF_MATH_F16, include/adafocus.h: numerics contract).

1. Contract parity: a CPU fp32 ResNet-50 built here from F.conv2d and the folded BN affine that rounds to fp16 (.half().float()) exactly
   where the contract rounds -- the stem's pooled output, every conv's activated output, the filters -- and averages the rounded final
   map.  Only fp32 accumulation order separates it from the kernels -- but every fp16 rounding turns that order noise into whole-ulp flips
   (the conv sums cancel: their terms are 10-30x the result), so two implementations of the contract that differ ONLY in accumulation
   (this model in fp32 and in fp64) are ~5.6e-4 apart in relative rms at the pooled features, not the 2e-4 once estimated.  The bound is
   therefore calibrated per case: the kernels may be at most 1.5x as far from the fp32 model as the fp64 model is (and 2e-4 always passes).
2. Against fp32: the fp16 trunk's features and the end-to-end logits stay within 1e-2 relative rms of the fp32 model; the crop actions
   (glancer + policy, fp32 in either mode) are bit-identical.
3. Temporal shift: both placements against the contract model; a clip's features do not depend on the other clips in its batch.
4. Bit identity of every alternative plan of the fp16 trunk (torch.equal)."""
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib, synth
from tests.helpers import golden, rnd, synth_sd

pytestmark = pytest.mark.gpu

CONTRACT_TOL = 2e-4     # fp16 trunk vs the contract model: always accepted ...
SPREAD_FACTOR = 1.5     # ... and up to 1.5x the distance between the contract model accumulated in fp32 and in fp64
F32_TOL = 1e-2          # fp16 trunk vs the fp32 trunk
BN_EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _h(x):
    return x.half().to(x.dtype)


def _rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


# ---------------------------------------------------------------------------------------------------- the contract model (CPU, fp32)
def _affine(sd, bn):
    scale = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
    return scale, sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale


def _conv_bn(sd, conv, bn, x, stride=1, pad=0):
    y = F.conv2d(x, _h(sd[conv + ".weight"]), stride=stride, padding=pad)
    s, b = _affine(sd, bn)
    return y * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def _shift(x, t, div):
    nt, c, hh, ww = x.shape
    v = x.view(nt // t, t, c, hh, ww)
    fold = c // div
    out = torch.zeros_like(v)
    out[:, :-1, :fold] = v[:, 1:, :fold]
    out[:, 1:, fold:2 * fold] = v[:, :-1, fold:2 * fold]
    out[:, :, 2 * fold:] = v[:, :, 2 * fold:]
    return out.view(nt, c, hh, ww)


def contract_trunk(sd, x, tsm=0, div=8, place="blockres", pooled=True):
    """The fp16 trunk's arithmetic on the CPU: fp32 stem + pool rounded once; per conv fp16 operands, fp32 products / BN / residual /
    ReLU, one rounding; the pool averages the rounded map."""
    y = F.relu(_conv_bn(sd, "conv1", "bn1", x, 2, 3))
    y = _h(F.max_pool2d(y, 3, 2, 1))
    for li, nblk, stride in ((1, 3, 1), (2, 4, 2), (3, 6, 2), (4, 3, 2)):
        for b in range(nblk):
            p = "layer%d.%d" % (li, b)
            s = stride if b == 0 else 1
            xin, t = y, tsm
            if t and place == "block":
                xin, t = _shift(xin, t, div), 0
            z = _shift(xin, t, div) if t else xin
            z = _h(F.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", z)))
            z = _h(F.relu(_conv_bn(sd, p + ".conv2", p + ".bn2", z, s, 1)))
            z = _conv_bn(sd, p + ".conv3", p + ".bn3", z)
            idn = _h(_conv_bn(sd, p + ".downsample.0", p + ".downsample.1", xin, s)) if b == 0 else xin
            y = _h(F.relu(z + idn))
    return y.mean((2, 3)) if pooled else y


def _contract_bound(sd, x, ref, **kw):
    """max(2e-4, 1.5 x the accumulation-order spread of the contract itself: the same model with fp64 convs, rounded at the same points)."""
    with torch.no_grad():
        ref64 = contract_trunk({k: v.double() for k, v in sd.items()}, x.double(), **kw)
    return max(CONTRACT_TOL, SPREAD_FACTOR * _rel_rms(ref, ref64))


def _trunk(dev, seed, math="f16"):
    from adafocus_amd.resnet import resnet50
    net = resnet50(num_classes=200).eval()
    sd = synth_sd("ACT", seed, "focuser.net.", keep_prefix=False)
    net.load_state_dict(sd, strict=True)
    net.set_math(math)
    return net.to(dev), sd


def _feat(net, x, dev):
    from adafocus_amd.utils import nchw_to_nhwc4
    with torch.no_grad():
        return net.features_nhwc4(nchw_to_nhwc4(x.to(dev))).clone()


# ---------------------------------------------------------------------------------------------------- 1. contract parity
@pytest.mark.parametrize("seed,p,n", [(404, 64, 2), (1103, 96, 4), (1135, 128, 3), (1151, 144, 2), (1107, 100, 3)])
def test_contract_parity(dev, seed, p, n):
    """G4's weights and input (seed 404, (2,3,64,64) of seed 45), then random patches at 96^2, 128^2, 144^2 and an odd 100^2."""
    net, sd = _trunk(dev, seed)
    x = rnd((2, 3, 64, 64), 45) if seed == 404 else rnd((n, 3, p, p), 500 + p)
    got = _feat(net, x, dev)
    with torch.no_grad():
        ref = contract_trunk(sd, x)
    assert torch.isfinite(got).all()
    err, bound = _rel_rms(got, ref), _contract_bound(sd, x, ref)
    print("contract parity p=%d: rel rms %.2e (bound %.2e)" % (p, err, bound))
    assert err <= bound, (err, bound)


def test_contract_parity_featmap_and_rows_stem(dev):
    """pooled=False (forward_map: the fp32 widening of the fp16 map) and the strip-walking stem's fp16 form (stem_rows = 2 takes it at any
    batch size) -- the map itself against the contract model."""
    net, sd = _trunk(dev, 1196)
    x = rnd((3, 3, 96, 96), 596)
    old = _lib.set_option("stem_rows", 2)
    try:
        with torch.no_grad():
            fmap = net.get_featmap(x.to(dev), pooled=False).cpu()
            rows = _feat(net, x, dev)
    finally:
        _lib.set_option("stem_rows", old)
    with torch.no_grad():
        ref = contract_trunk(sd, x, pooled=False)
    assert fmap.shape == ref.shape
    assert torch.equal(fmap, _h(fmap))                     # an exact widening of fp16 values
    err, bound = _rel_rms(fmap, ref), _contract_bound(sd, x, ref, pooled=False)
    print("contract parity, 3x3 map at 96^2: rel rms %.2e (bound %.2e)" % (err, bound))
    assert err <= bound, (err, bound)
    assert torch.equal(rows, _feat(net, x, dev))          # strip-walking stem == tile-form stem (fp16 store)


# ---------------------------------------------------------------------------------------------------- 2. against fp32
def test_g4_features_against_f32(dev):
    x = rnd((2, 3, 64, 64), 45)
    n16, _ = _trunk(dev, 404, "f16")
    n32, _ = _trunk(dev, 404, "f32")
    f16, f32 = _feat(n16, x, dev), _feat(n32, x, dev)
    g = torch.from_numpy(golden("g4_resnet_blocks")["trunk"])
    err = _rel_rms(f16, f32)
    print("G4 trunk features fp16 vs fp32: rel rms %.2e (vs golden %.2e)" % (err, _rel_rms(f16, g)))
    assert torch.isfinite(f16).all() and err <= F32_TOL, err


def _act_model(dev, local_math):
    from adafocus_amd.gfv_net import GFV
    from tests.test_state_dict_compat import act_args
    a = act_args()
    a.__dict__.update(num_segments=8, gpu=0, local_math=local_math)
    m = GFV(a).eval()
    m.load_state_dict(synth_sd("ACT", 1007), strict=True)
    return m.to(dev)


def test_act_end_to_end_against_f32(dev):
    """G7 (ActivityNet, B = 2, T = 8, P = 96): logits of the fp16 trunk within 1e-2 of the fp32 model's; the policy's crop actions --
    computed before the local CNN, fp32 in either mode -- bit-identical; a captured hot path equals the eager one."""
    g = golden("g7_act_e2e")
    m32, m16 = _act_model(dev, "f32"), _act_model(dev, "f16")
    assert m16.focuser.net.math == "f16" and m32.focuser.net.math == "f32"
    frames = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=0)).to(dev)
    with torch.no_grad():
        l32, last32, _, idx32 = m32.offline_forward(frames, frames)
        l16, last16, _, idx16 = m16.offline_forward(frames, frames)
        lf16, _, _, _ = m16.offline_forward(frames, frames, torch.from_numpy(g["forced_idx"]))
    assert torch.equal(idx16, idx32)
    assert torch.isfinite(l16).all() and torch.isfinite(last16).all()
    err, errf = _rel_rms(l16, l32), _rel_rms(lf16, torch.from_numpy(g["logits_forced"]))
    print("G7 ACT logits fp16 vs fp32: rel rms %.2e; forced actions vs the reference's logits: %.2e" % (err, errf))
    assert err <= F32_TOL and errf <= F32_TOL, (err, errf)
    # the captured hot path (exclusive: the persistent GRU scan stays in the graph, as in the eager call)
    table = torch.from_numpy(synth.grid_table(7))
    actions = table[torch.from_numpy(g["forced_idx"]).reshape(-1)].to(dev)
    gvec = torch.from_numpy(g["glancer_vec"]).to(dev)
    fr = frames.view(16, 3, 224, 224)
    with torch.no_grad():
        le, laste, _ = m16.hot_path(fr, gvec, actions, 2, 8)
        le, laste = le.clone(), laste.clone()
        graph = m16.capture_hot_path(2, 8, exclusive=True, check_every=0)
        lg, lastg = graph(fr, gvec, actions)
        torch.cuda.synchronize()
    assert torch.equal(lg, le) and torch.equal(lastg, laste)


def _sth_model(dev, local_math):
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.gpu = 0
    a.local_math = local_math
    m = GFV(a).eval()
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])  # evaluate.py:83
    m.load_state_dict(synth_sd("STH", 1007), strict=True)
    pol = {k[len("policy."):]: v for k, v in synth_sd("STH_POLICY", 1007).items()}
    for p in (m.focuser.policy.policy_old, m.focuser.policy.policy):
        p.load_state_dict(pol)
        p.eval()
    return m.to(dev), a


def test_sth_end_to_end_against_f32(dev):
    """G7 STH (TSM-ResNet-50 with the shift fused into conv1, Tg = Tf = 8, P = 128): stage-2 logits within 1e-2 of fp32."""
    g = golden("g7_sth_e2e")
    (m32, a), (m16, _) = _sth_model(dev, "f32"), _sth_model(dev, "f16")
    gl = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=3)).to(dev)
    fo = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=4)).view(2, 8, 3, 224, 224).to(dev)
    forced = torch.from_numpy(g["forced_action"]).to(dev)
    out = {}
    with torch.no_grad():
        for k, m in (("f32", m32), ("f16", m16)):
            fm, glog = m.glance(gl)
            out[k] = m.action_stage2(fo, fm, glog, 0, a, prev_local_patch=None, training=False, forced_action=forced)[0].clone()
    err = _rel_rms(out["f16"], out["f32"])
    print("G7 STH logits fp16 vs fp32: rel rms %.2e" % err)
    assert torch.isfinite(out["f16"]).all() and err <= F32_TOL, err


# ---------------------------------------------------------------------------------------------------- 3. temporal shift
@pytest.mark.parametrize("t,place", [(8, "blockres"), (12, "blockres"), (16, "blockres"), (8, "block")])
def test_temporal_shift_against_contract(dev, t, place):
    net, sd = _trunk(dev, 1300 + t)
    net.tsm_segments, net.tsm_div, net.tsm_place = t, 8, place
    x = rnd((2 * t, 3, 64, 64), 600 + t)
    got = _feat(net, x, dev)
    with torch.no_grad():
        ref = contract_trunk(sd, x, tsm=t, div=8, place=place)
    err, bound = _rel_rms(got, ref), _contract_bound(sd, x, ref, tsm=t, div=8, place=place)
    print("contract parity, shift T=%d %s: rel rms %.2e (bound %.2e)" % (t, place, err, bound))
    assert err <= bound, (t, place, err, bound)
    # a clip's features do not depend on the other clips of its batch
    assert torch.equal(_feat(net, x[t:], dev), got[t:])


def test_temporal_shift_fold_must_be_whole_chunks(dev):
    """fold = cin / tsm_div: a multiple of 8 halfs (16-byte chunks) or ADAF_E_LAYOUT -- tsm_div 16 gives fold 4 at layer1.0's conv1."""
    net, _ = _trunk(dev, 1300)
    net.tsm_segments, net.tsm_div = 4, 16
    with pytest.raises(_lib.AdafError):
        _feat(net, rnd((4, 3, 64, 64), 601), dev)


# ---------------------------------------------------------------------------------------------------- 4. bit identity
def test_bit_identity_batch_position_pool_fusion_and_map(dev):
    net, _ = _trunk(dev, 1400)
    x = rnd((1032, 3, 96, 96), 700)
    big = _feat(net, x, dev)
    assert torch.equal(big, _feat(net, x, dev))                                   # run to run
    one = _feat(net, x[1017:1018], dev)
    assert torch.equal(one[0], big[1017])                                         # batch of 1 vs index 1017 of 1032 (rows stem, full tiles)
    assert torch.equal(_feat(net, x[:20], dev), big[:20])                         # 20 patches: a part-filled last pool tile
    old = _lib.set_option("conv_pool", 0)                                         # separate fp16 pool launch
    try:
        sep = _feat(net, x[:20], dev)
    finally:
        _lib.set_option("conv_pool", old)
    assert torch.equal(sep, big[:20])
    net.set_fusion(0)                                                              # unfused stem + fp16 max-pool, separate layer1.0 launches
    try:
        assert torch.equal(_feat(net, x[:20], dev), big[:20])
    finally:
        net.set_fusion(1)
    from adafocus_amd.utils import nchw_to_nhwc4
    with torch.no_grad():
        fmap, feat = net._sync().forward_map(nchw_to_nhwc4(x[:20].to(dev)))
    assert torch.equal(feat, big[:20])
    s = torch.zeros_like(feat)
    for i in range(3):                                                             # the pool rule: rounded values, pixel order, / hw
        for j in range(3):
            s += fmap[:, i, j]
    assert torch.equal(s / torch.full_like(s, 9.0), feat)                         # (a tensor divisor: a scalar one is a reciprocal multiply)


def test_bit_identity_forward_frames(dev):
    """forward_frames (the stem gathers its windows; below 256 patches the gather runs first) against gather + forward, NCHW and NHWC4
    frames, two action sets."""
    from adafocus_amd.utils import get_patch, nchw_to_nhwc4
    net, _ = _trunk(dev, 1500)
    for nf in (128, 8):
        frames = rnd((nf, 3, 160, 160), 800 + nf).to(dev)
        acts = torch.rand((2 * nf, 2), generator=torch.Generator().manual_seed(nf)).to(dev)
        with torch.no_grad():
            patches = torch.cat([get_patch(frames, acts[:nf], 96), get_patch(frames, acts[nf:], 96)])
            ref = net.features_nhwc4(nchw_to_nhwc4(patches)).clone()
            a = net.features_from_frames(frames, acts, 96).clone()
            b = net.features_from_frames(nchw_to_nhwc4(frames), acts, 96).clone()
        assert torch.equal(a, ref) and torch.equal(b, ref), nf


def test_bit_identity_streams_and_math_switch(dev):
    net, _ = _trunk(dev, 1600)
    xs = [rnd((40, 3, 96, 96), 900 + i).to(dev) for i in range(6)]
    from adafocus_amd.utils import nchw_to_nhwc4
    with torch.no_grad():
        serial = [net.features_nhwc4(nchw_to_nhwc4(x)).clone() for x in xs]
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [None] * 6
        for i, x in enumerate(xs):
            s = streams[i % 3]
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs[i] = net.features_nhwc4(nchw_to_nhwc4(x))
        torch.cuda.synchronize()
    for a, b in zip(outs, serial):
        assert torch.equal(a, b)
    # f16 -> f32 gives the bits of a fresh fp32 trunk
    net.set_math("f32")
    fresh, _ = _trunk(dev, 1600, "f32")
    assert torch.equal(_feat(net, xs[0].cpu(), dev), _feat(fresh, xs[0].cpu(), dev))
    assert not torch.equal(_feat(net, xs[0].cpu(), dev), serial[0])
