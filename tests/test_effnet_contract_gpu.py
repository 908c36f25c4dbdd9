"""GPU tests of EfficientNet-B3 in fp16 storage against its numerics contract (include/adafocus.h; the CPU model:
tests/effnet_contract.py), block by block on each block's OWN input, in both launch plans.

Teacher-forced: block k's input is what the kernels stored after k blocks (forward_blocks(x4, k)), its output what they stored after
k + 1; the fp64 contract model applied to that input differs from a correct kernel by the order of fp32 sums only, which a rounding
turns into isolated one-ulp flips.  Metric, element by element: e = |got - ref| / (2^-10 max(|ref|, rms of ref over the image)).
Bound per block: max(1, 1.5 x spread), spread = the max e between the contract model run in fp32 and in fp64 ON THE SAME INPUT -- the
distance between two implementations of the contract that differ in accumulation only; 1.5 is tests/test_f16_trunk.py's
SPREAD_FACTOR; the floor of one ulp is a single rounding flip.  Never taken from the kernels' output.

Case matrix (n = 3: a ragged last pair where a workgroup of the whole-block kernel owns two images):
  144^2 native padding   config 5's own: 9 x 9 and 5 x 5 maps under the one-launch kernels (16 blocks)
  100^2 dynamic padding  odd maps 25 / 13, 7 x 7 and 4 x 4 (15 blocks)
  75^2  native padding   9 x 9 for blocks 6-7, 4 x 4 behind them (11 blocks)
each with fusion on (whole-block kernels + expand inside the depthwise launch) and off (four launches per block, the expand launch
included).  What the bound can and cannot see: tests/test_effnet_contract_host.py.

Measured on an MI355X (`pytest -s` prints every block; the table: LABNOTES.md 3.15): max e per block 0.02 - 1.39 ulps in either plan.  Nearly
every difference is a one-ulp flip of a stored output (e <= 1); the two above 1 (1.39: block 0 at 75^2; 1.29: block 2 at 144^2) are two-ulp
differences -- one flip of an intermediate stored value, amplified by the project conv -- on blocks where the model's own fp32-vs-fp64 spread
is as large (1.39, 2.09).  Closest to its bound: block 5 at 75^2, 0.97 of 1.00.  Head map 3.0e-7 - 3.6e-7 of bounds 8.8e-7 - 1.0e-6, pooled
1.3e-7 - 2.0e-7 of 2.6e-7 - 4.1e-7 (144^2: 2.03e-7 of 2.71e-7); depthwise squeeze mean 0.8e-7 - 1.6e-7 of 1.6e-7 - 2.7e-7 (the mean of the
rounded map: 1.3e-4 - 2.6e-4); free-running pooled features 2.02e-4 of 3.00e-4.  No disagreement between the plans or with the contract.
"""
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import synth
from tests import effnet_contract as C
from tests.helpers import rnd
from tests.test_f16_trunk import CONTRACT_TOL, SPREAD_FACTOR

pytestmark = pytest.mark.gpu

CASES = [(144, "native", 16, 7), (100, None, 15, 7), (75, "native", 11, 5)]     # size, padding, whole blocks, fused-expand blocks
# fp32 results that nothing rounds to fp16 (the head map, the pooled vector, the squeeze mean) are compared relative to max(1, max |ref|) of
# the sample and bounded by SPREAD_FACTOR x the model's own fp32-vs-fp64 distance; the floor is the fp32 analogue of "one flip is legitimate":
# one fp32 ulp of the scale.
F32_ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


def _smooth(shape, seed):
    """tests/test_effnet.py's inputs: structure at every scale."""
    n, c, h, w = shape
    coarse = rnd((n, c, 6, 6), seed, 0.8)
    return F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False) + rnd(shape, seed + 1, 0.5)


def _swish(x):
    return x * torch.sigmoid(x)


_NETS, _REFS = {}, {}


def _net(dev, image_size):
    if image_size not in _NETS:
        from adafocus_amd.efficientnet import EfficientNet
        m = EfficientNet.from_name(C.NAME, num_classes=200, image_size=image_size, dtype="f16").eval()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}
        m.load_state_dict(sd, strict=True)
        _NETS[image_size] = (m.to(dev), sd)
    return _NETS[image_size]


def _refs(key, xin, make):
    """(fp64, fp32) contract outputs for `xin`, computed once per distinct input: the two plans share every block whose input they
    agree on to the bit."""
    for x0, r in _REFS.setdefault(key, []):
        if x0.shape == xin.shape and torch.equal(x0, xin):
            return r
    with torch.no_grad():
        r = (make(torch.float64), make(torch.float32))
    _REFS[key].append((xin, r))
    return r


def _rel_max(a, b):
    """max |a - b| / max(1, max |b|), per sample (first axis), the worst sample."""
    n = b.shape[0]
    scale = b.double().reshape(n, -1).abs().amax(1).clamp(min=1.0)
    return float(((a.double() - b.double()).reshape(n, -1).abs().amax(1) / scale).max())


def _stored(eng, x4, k):
    t = eng.forward_blocks(x4, k)
    assert t.dtype == torch.float16
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def _run_plan(dev, size, image_size, whole, fused, fusion):
    """The stored tensors after 0 .. 26 blocks in one plan."""
    from adafocus_amd import _lib as L
    from adafocus_amd.utils import nchw_to_nhwc4
    m, sd = _net(dev, image_size)
    x = _smooth((3, 3, size, size), 2000 + size)
    x4 = nchw_to_nhwc4(x.to(dev))
    plan = int(L.get_option("effnet_plan"))
    assert plan & L.EF_PLAN_FUSED_EXPAND
    with torch.no_grad():
        m.fusion = fusion
        try:
            if fusion:
                eng = m.engine()
                assert eng.whole_blocks(size) == whole and eng.fused_expand_blocks(size) == fused
                outs = [_stored(eng, x4, k) for k in range(27)]
            else:
                with L.option("effnet_plan", plan & ~L.EF_PLAN_FUSED_EXPAND):
                    eng = m.engine()
                    assert eng.whole_blocks(size) == 0 and eng.fused_expand_blocks(size) == 0
                    outs = [_stored(eng, x4, k) for k in range(27)]
        finally:
            m.fusion = True
    return m, sd, x, x4, outs


@pytest.mark.parametrize("fusion", [True, False], ids=["fused", "four_launch"])
@pytest.mark.parametrize("size,image_size,whole,fused", CASES)
def test_every_block_on_its_own_input(dev, size, image_size, whole, fused, fusion):
    """The stem from the frames and all 26 MBConv blocks, each on the input the kernels themselves stored."""
    assert SPREAD_FACTOR == C.SPREAD_FACTOR
    _, sd, x, _, outs = _run_plan(dev, size, image_size, whole, fused, fusion)
    tag = "%d^2 %s %s" % (size, image_size, "fused" if fusion else "four-launch")
    bad = []
    for bi in range(-1, 26):
        got = outs[bi + 1]
        if bi < 0:
            r64, r32 = _refs((size, image_size, bi), x, lambda dt: C.contract_stem(sd, x, image_size, dt))
        else:
            xin = outs[bi]
            r64, r32 = _refs((size, image_size, bi), xin, lambda dt: C.contract_block(sd, xin, bi, image_size, dt))
        assert got.shape == r64.shape and torch.isfinite(got).all(), (tag, bi)
        bound, spread = C.ulp_bound(r32, r64)
        err = float(C.ulp_error(got, r64).max())
        print("%s %s: max e %.2f ulps, bound %.2f (spread %.2f), differs from the fp32 model in %.1e of %d elements"
              % (tag, "stem    " if bi < 0 else "block %2d" % bi, err, bound, spread, C.flip_share(got, r32), got.numel()))
        if not err <= bound:
            bad.append((bi, err, bound))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("size,image_size,whole,fused", CASES)
def test_head_and_pool_on_the_stored_block_output(dev, size, image_size, whole, fused):
    """The pooled features of the head-pool epilogue (features_nhwc4) and the map of the separate launches (extract_features) against
    the contract's head on the kernels' own block-26 output, in fp32: max |got - ref| / max(1, max |ref|) per sample, bound
    max(one fp32 ulp, 1.5 x the same distance between the fp32 and the fp64 model)."""
    m, sd, x, x4, outs = _run_plan(dev, size, image_size, whole, fused, True)
    with torch.no_grad():
        fvec = m.features_nhwc4(x4).cpu()
        fmap = m.extract_features(x.to(dev)).cpu().contiguous()
        (map64, vec64), (map32, vec32) = _refs((size, image_size, "head"), outs[26], lambda dt: C.contract_head_pooled(sd, outs[26], dt))
    dist = _rel_max
    assert fmap.shape == map64.shape and fvec.shape == vec64.shape == (3, 1536)
    for what, got, r32, r64 in (("map", fmap, map32, map64), ("pooled", fvec, vec32, vec64)):
        spread = dist(r32, r64)
        bound, err = max(F32_ULP, SPREAD_FACTOR * spread), dist(got, r64)
        print("%d^2 %s head %s: %.2e, bound %.2e (spread %.2e)" % (size, image_size, what, err, bound, spread))
        assert err <= bound, (size, image_size, what, err, bound)


def test_free_running_pooled_features(dev):
    """One free-running case (144^2, n = 2): pooled features against contract_features, relative rms, bound as
    test_f16_trunk._contract_bound: max(CONTRACT_TOL, SPREAD_FACTOR x the fp32-vs-fp64 spread of the model)."""
    from adafocus_amd.utils import nchw_to_nhwc4
    m, sd = _net(dev, "native")
    x = _smooth((2, 3, 144, 144), 2300)
    with torch.no_grad():
        got = m.features_nhwc4(nchw_to_nhwc4(x.to(dev))).cpu()
        ref = C.contract_features(sd, x, "native", torch.float32)
        ref64 = C.contract_features(sd, x, "native", torch.float64)

    def rel_rms(a, b):
        a, b = a.double(), b.double()
        return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    err, bound = rel_rms(got, ref), max(CONTRACT_TOL, SPREAD_FACTOR * rel_rms(ref, ref64))
    print("free-running 144^2 pooled features: rel rms %.2e (bound %.2e)" % (err, bound))
    assert torch.isfinite(got).all() and err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------------- the fp16 building blocks
def _held(tag, got, r32, r64):
    bound, spread = C.ulp_bound(r32, r64)
    err = float(C.ulp_error(got, r64).max())
    print("%s: max e %.2f ulps, bound %.2f (spread %.2f), differs from the fp32 model in %.1e of %d elements"
          % (tag, err, bound, spread, C.flip_share(got, r32), got.numel()))
    assert got.shape == r64.shape and err <= bound, (tag, err, bound)


@pytest.mark.parametrize("k,stride,size,c", [(5, 2, 9, 816), (3, 1, 3, 2304), (5, 2, 11, 48)])
def test_dwconv_f16_elementwise(dev, ops, k, stride, size, c):
    """fp16 inputs: an fp64 depthwise conv of those inputs + BN affine + swish, rounded once.  The squeeze mean the launch returns is
    the mean of the UNROUNDED fp32 values: held to the fp64 mean of those at max(one fp32 ulp, 1.5 x the model's fp32-vs-fp64 distance),
    a bar the mean of the rounded map misses by more than ten times (asserted), so this tells the two apart for the stand-alone
    depthwise kernels (the staged one and, at 3 x 3, the tiny-map one)."""
    from oracle import ref_effnet as R
    n = 11 if size <= 9 else 3
    x16 = rnd((n, c, size, size), 700 + size + c).half()
    w = rnd((c, 1, k, k), 701 + c, 0.3)
    scale, bias = rnd((c,), 702, 0.2) + 1.0, rnd((c,), 703, 0.1)
    pb, pa = R.same_pad(size, k, stride)

    def unrounded(dt):
        y = F.conv2d(F.pad(x16.to(dt), (pb, pa, pb, pa)), w.to(dt), None, stride, 0, 1, c)
        return _swish(y * scale.to(dt).view(1, -1, 1, 1) + bias.to(dt).view(1, -1, 1, 1))

    def model(dt):
        return unrounded(dt).half().to(dt)
    wk = ops.pack_dw_weight_kxk(w.to(dev))
    got, pool = ops.dwconv_same_bn_act(x16.permute(0, 2, 3, 1).contiguous().to(dev), wk, scale.to(dev), bias.to(dev), k, stride, ops.ACT_SWISH,
                                       want_pool=True)
    assert got.dtype == torch.float16 and pool.dtype == torch.float32
    tag = "dwconv k%d s%d %d^2 c%d" % (k, stride, size, c)
    _held(tag, got.float().cpu().permute(0, 3, 1, 2), model(torch.float32), model(torch.float64))
    mean64, mean32 = unrounded(torch.float64).mean((2, 3)), unrounded(torch.float32).mean((2, 3))
    spread = _rel_max(mean32, mean64)
    bound, err = max(F32_ULP, SPREAD_FACTOR * spread), _rel_max(pool.cpu(), mean64)
    wrong = _rel_max(model(torch.float64).mean((2, 3)), mean64)             # what a squeeze over the ROUNDED map would give
    print("%s squeeze mean: %.2e, bound %.2e (spread %.2e); the mean of the rounded map: %.2e" % (tag, err, bound, spread, wrong))
    assert pool.shape == mean64.shape and err <= bound, (tag, err, bound)
    assert wrong > 10 * bound, (tag, wrong, bound)


@pytest.mark.parametrize("hw,cin,cout,res", [(25, 2304, 384, True), (10, 24, 24, True), (49, 40, 24, False)])
def test_conv1x1_gated_f16_elementwise(dev, ops, hw, cin, cout, res):
    """The operand fp16(x16 * gate) and fp16 filters, in fp64, + BN affine (+ the fp16 identity), rounded once."""
    n = 3
    side = int(round(hw ** 0.5))
    hh, ww = (side, side) if side * side == hw else (1, hw)
    x16 = rnd((n, hh, ww, cin), 720 + cin).half()
    gate = torch.sigmoid(rnd((n, cin), 721))
    w16 = rnd((cout, cin), 722, (1.0 / cin) ** 0.5).half()
    scale, bias = rnd((cout,), 723, 0.2) + 1.0, rnd((cout,), 724, 0.1)
    r16 = rnd((n, hh, ww, cout), 725).half() if res else None
    xg = (x16.float() * gate.view(n, 1, 1, cin)).half()

    def model(dt):
        y = (xg.to(dt).reshape(-1, cin) @ w16.to(dt).t()).view(n, hh, ww, cout) * scale.to(dt) + bias.to(dt)
        return (y + r16.to(dt) if res else y).half().to(dt)
    got = ops.conv1x1_gated_bn(x16.to(dev), gate.to(dev), w16.to(dev), scale.to(dev), bias.to(dev), r16.to(dev) if res else None)
    assert got.dtype == torch.float16
    _held("gated project hw%d %d -> %d%s" % (hw, cin, cout, " + identity" if res else ""), got.float().cpu(), model(torch.float32),
          model(torch.float64))


def test_conv_engine_swish_f16_elementwise(dev, ops):
    """conv2d_bn_act_f16 with ADAF_ACT_SWISH (the expand launch of the four-launch plan) at test_conv_engine_swish_epilogue's shape."""
    x16 = rnd((2, 9, 9, 96), 730).half()
    w = rnd((576, 96, 1, 1), 731, 0.1)
    scale, bias = rnd((576,), 732, 0.2) + 1.0, rnd((576,), 733, 0.1)

    def model(dt):
        y = x16.to(dt).reshape(-1, 96) @ w.half().to(dt).view(576, 96).t()
        return _swish(y * scale.to(dt) + bias.to(dt)).view(2, 9, 9, 576).half().to(dt)
    got = ops.conv2d_bn_act_f16(x16.to(dev), ops.pack_conv_weight_f16(w.to(dev)), scale.to(dev), bias.to(dev), act=ops.ACT_SWISH)
    assert got.dtype == torch.float16
    _held("conv engine swish 96 -> 576", got.float().cpu(), model(torch.float32), model(torch.float64))
