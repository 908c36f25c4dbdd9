"""Backward primitives of the trunk's convolutions on the MI355X (csrc/conv_bwd.hip): the split-K weight gradient and the
engine-run data gradient per geometry of the ResNet trunk against F.conv2d autograd in fp64, the BatchNorm affine gradients with a
gamma = 0 channel, run-to-run bit identity, the exact one-pass kernels (max-pool routing, the shift adjoint) and the workspace contract.

Tolerance of every comparison: the error against the fp64 result, relative to that quantity's largest entry, is at most 50x the
distance between the same CPU autograd in fp32 and in fp64 (G17's rule, tests/test_stage3_gpu.py); no other number appears."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib as L
from tests.helpers import rnd

pytestmark = pytest.mark.gpu

SPREAD_FACTOR = 50


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _pad4(x_nhwc):
    """(N,H,W,3) -> (N,H,W,4) with a zero lane: the stem's input layout."""
    return F.pad(x_nhwc, (0, 4 - x_nhwc.shape[-1])) if x_nhwc.shape[-1] % 4 else x_nhwc


def _autograd(x, w, g, stride, pad, scale, dtype):
    """(dW of the plain convolution, dx with `scale` per output channel folded into the upstream gradient) by CPU autograd in `dtype`."""
    x, w, g = (t.to(dtype) for t in (x, w, g))
    x.requires_grad_(True)
    w.requires_grad_(True)
    y = F.conv2d(x, w, None, stride, pad)
    dw, = torch.autograd.grad(y, w, g, retain_graph=True)
    dx, = torch.autograd.grad(y, x, g * scale.to(dtype).view(1, -1, 1, 1))
    return dw, dx


def _rel(got, ref64):
    return ((got.double() - ref64).abs().max() / ref64.abs().max()).item()


# (tag, N, Cin, Cout, k, stride, pad, H, W, dgrad too)
CASES = [
    ("1x1_s1", 5, 64, 256, 1, 1, 0, 9, 9, True),
    ("1x1_s2", 3, 256, 512, 1, 2, 0, 9, 9, True),
    ("3x3_s1_9", 3, 64, 64, 3, 1, 1, 9, 9, True),
    ("3x3_s1_2", 3, 64, 64, 3, 1, 1, 2, 2, True),
    ("3x3_s2_even", 3, 128, 128, 3, 2, 1, 10, 10, True),
    ("3x3_s2_odd", 3, 128, 128, 3, 2, 1, 9, 9, True),
    ("stem_40", 2, 3, 64, 7, 2, 3, 40, 40, False),
    ("stem_37", 2, 3, 64, 7, 2, 3, 37, 37, False),
    ("long", 33, 64, 64, 3, 1, 1, 18, 18, True),
]


def _case(tag):
    i = [c[0] for c in CASES].index(tag)
    _, n, cin, cout, k, s, p, hh, ww, _ = CASES[i]
    x = rnd((n, cin, hh, ww), 2000 + i)
    w = rnd((cout, cin, k, k), 2100 + i, (cin * k * k) ** -0.5)
    oh, ow = (hh + 2 * p - k) // s + 1, (ww + 2 * p - k) // s + 1
    g = rnd((n, cout, oh, ow), 2200 + i)
    scale = rnd((cout,), 2300 + i)
    scale[1] = 0.0
    return x, w, g, scale, s, p


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_wgrad_and_dgrad_against_fp64_autograd(dev, ops, tag):
    want_dgrad = CASES[[c[0] for c in CASES].index(tag)][9]
    x, w, g, scale, s, p = _case(tag)
    dw64, dx64 = _autograd(x, w, g, s, p, scale, torch.float64)
    dw32, dx32 = _autograd(x, w, g, s, p, scale, torch.float32)
    xd, gd = _pad4(_nhwc(x)).to(dev), _nhwc(g).to(dev)
    w_ohwi = ops.pack_conv_weight(w.to(dev))
    assert w_ohwi.shape[-1] == xd.shape[-1]
    dw = ops.conv2d_wgrad(xd, gd, tuple(w_ohwi.shape), s, p)
    assert tuple(dw.shape) == tuple(w_ohwi.shape) and torch.isfinite(dw).all()
    if w.shape[1] == 3:
        assert not dw[..., 3].any()                       # the zero lane of the stem's input
    got = dw[..., :w.shape[1]].permute(0, 3, 1, 2).cpu()
    spread = _rel(dw32, dw64)
    err = _rel(got, dw64)
    print("%s wgrad: rel err %.2e, fp32-fp64 spread %.2e" % (tag, err, spread))
    assert spread > 0 and err <= SPREAD_FACTOR * spread, (tag, err, spread)
    assert torch.equal(dw, ops.conv2d_wgrad(xd, gd, tuple(w_ohwi.shape), s, p))          # twice on the same inputs: the same bits
    if want_dgrad:
        wd = ops.pack_conv_dgrad_weight(w_ohwi, scale.to(dev))
        dx = ops.conv2d_dgrad(gd, wd, tuple(xd.shape), s, p)
        assert torch.isfinite(dx).all()
        got = dx.permute(0, 3, 1, 2).cpu()
        spread = _rel(dx32, dx64)
        err = _rel(got, dx64)
        print("%s dgrad: rel err %.2e, fp32-fp64 spread %.2e" % (tag, err, spread))
        assert spread > 0 and err <= SPREAD_FACTOR * spread, (tag, err, spread)
        if s == 2 and w.shape[-1] == 1:
            assert not got[:, :, 1::2].any() and not got[:, :, :, 1::2].any()      # a 1x1 stride-2 conv never read the odd positions


def test_bn_affine_gradients_with_a_zero_gamma(dev, ops):
    """conv 3x3 + BatchNorm(eval) with gamma[1] = 0: dW, dgamma, dbeta from the unscaled weight gradient, finite and within the rule."""
    x, w, g, _, s, p = _case("3x3_s1_9")
    cout = w.shape[0]
    gamma, beta, mean = rnd((cout,), 31), rnd((cout,), 32), rnd((cout,), 33, 0.3)
    var = rnd((cout,), 34).abs() + 0.5
    gamma[1] = 0.0

    def ref(dt):
        ps = [t.to(dt).requires_grad_(True) for t in (w, gamma, beta)]
        y = F.batch_norm(F.conv2d(x.to(dt), ps[0], None, s, p), mean.to(dt), var.to(dt), ps[1], ps[2], False, 0.0, 1e-5)
        return torch.autograd.grad(y, ps, g.to(dt))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    xd, gd = _nhwc(x).to(dev), _nhwc(g).to(dev)
    w_ohwi = ops.pack_conv_weight(w.to(dev))
    scale, _ = ops.fold_bn(gamma.to(dev), beta.to(dev), mean.to(dev), var.to(dev), 1e-5)
    dw_raw = ops.conv2d_wgrad(xd, gd, tuple(w_ohwi.shape), s, p)
    got = ops.conv_bn_param_grad(gd, dw_raw, w_ohwi, scale, mean.to(dev), var.to(dev), 1e-5, w.shape[1])
    for name, a, b64, b32 in zip(("dW", "dgamma", "dbeta"), got, r64, r32):
        assert torch.isfinite(a).all(), name
        spread, err = _rel(b32, b64), _rel(a.cpu(), b64)
        print("%s: rel err %.2e, spread %.2e" % (name, err, spread))
        assert err <= SPREAD_FACTOR * spread, (name, err, spread)
    assert not got[0][1].any() and got[1][1].item() != 0.0          # the gamma = 0 channel: no weight gradient, a live dgamma


@pytest.mark.parametrize("hw", [(8, 8), (9, 9), (7, 10)])
def test_maxpool_backward_routes_like_autograd(dev, ops, hw):
    x = rnd((2, 64) + hw, 51 + hw[0]).requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    g = rnd(tuple(y.shape), 52)
    ref, = torch.autograd.grad(y, x, g)
    got = ops.maxpool3x3s2_backward(_nhwc(x.detach()).to(dev), _nhwc(g).to(dev))
    assert torch.equal(got.permute(0, 3, 1, 2).cpu(), ref)


def test_maxpool_backward_ties_go_to_the_first_maximum(dev, ops):
    """A constant map: every window's arg-max is its first element in row-major order, as in ATen."""
    x = torch.ones(1, 4, 6, 6, requires_grad=True)
    y = F.max_pool2d(x, 3, 2, 1)
    g = rnd(tuple(y.shape), 53)
    ref, = torch.autograd.grad(y, x, g)
    got = ops.maxpool3x3s2_backward(_nhwc(x.detach()).to(dev), _nhwc(g).to(dev))
    assert torch.equal(got.permute(0, 3, 1, 2).cpu(), ref)


@pytest.mark.parametrize("div", [8, 4])
def test_shift_adjoint_equals_autograd_of_the_oracle_shift(dev, ops, div):
    from oracle import ref_model as O
    x = rnd((8, 64, 3, 3), 61).requires_grad_(True)
    y = O.temporal_shift(x, 4, div)
    g = rnd(tuple(y.shape), 62)
    ref, = torch.autograd.grad(y, x, g)
    assert torch.equal(ops.temporal_shift_backward(g.to(dev), 4, div, L.LAYOUT_NCHW).cpu(), ref)
    got = ops.temporal_shift_backward(_nhwc(g).to(dev), 4, div, L.LAYOUT_NHWC)
    assert torch.equal(got.permute(0, 3, 1, 2).cpu(), ref)


def test_relu_and_avgpool_backward(dev, ops):
    y = rnd((3, 5, 5, 64), 71).to(dev)
    dy, dy2 = rnd((3, 5, 5, 64), 72).to(dev), rnd((3, 5, 5, 64), 73).to(dev)
    assert torch.equal(ops.relu_backward(dy, y), torch.where(y > 0, dy, torch.zeros_like(dy)))
    assert torch.equal(ops.relu_backward(dy, y, dy2), torch.where(y > 0, dy + dy2, torch.zeros_like(dy)))
    df = rnd((3, 64), 74)
    full = (df / 25.0).view(3, 1, 1, 64).expand(3, 5, 5, 64).contiguous()       # an IEEE division, on the CPU (the device divides by a scalar as a product with its reciprocal)
    assert torch.equal(ops.global_avgpool_backward(df.to(dev), (3, 5, 5, 64)).cpu(), full)
    assert torch.equal(ops.global_avgpool_backward(df.to(dev), (3, 5, 5, 64), y).cpu(), torch.where(y.cpu() > 0, full, torch.zeros_like(full)))


# ---- the workspace contract, through ctypes with exactly the queried bytes under guard bands -----------------------------
def _params(x_shape, w_shape, s, p):
    n, hh, ww, cin = x_shape
    cout, kh, kw, _ = w_shape
    return L.ConvParams(n=n, h=hh, w=ww, cin=cin, cout=cout, kh=kh, kw=kw, stride=s, pad=p, act=0, tsm_segments=0, tsm_div=0, ldx=0, ldo=0,
                        ldr=0, tile=0)


@pytest.mark.parametrize("tag", ["1x1_s1", "long"])
def test_wgrad_workspace_contract(dev, ops, tag):
    from tests.test_workspace_contract_gpu import contract
    lib = L.load_library()
    x, w, g, _, s, p = _case(tag)
    xs = [_nhwc(x).to(dev), _nhwc(x.flip(0) * 0.5).to(dev)]
    gd = _nhwc(g).to(dev)
    w_shape = (w.shape[0], w.shape[2], w.shape[3], w.shape[1])
    prm = _params(tuple(xs[0].shape), w_shape, s, p)
    need = lib.adaf_conv2d_wgrad_workspace_bytes(C.byref(prm))
    h = L.handle(dev)

    def call(ws, nbytes, outs, alt):
        xin = xs[1 if alt else 0]
        return lib.adaf_conv2d_wgrad_f32(h, C.byref(prm), L.ptr(xin), L.ptr(gd), L.ptr(outs["dw"]), L.ptr(ws), nbytes, L.stream_ptr())

    contract("conv_wgrad", tag, dev, need, call, {"dw": w_shape}, align=True,
             wrapper=lambda: {"dw": ops.conv2d_wgrad(xs[0], gd, w_shape, s, p)})
    prm.cout = 48                                                   # a description the call refuses: the query says 0
    assert lib.adaf_conv2d_wgrad_workspace_bytes(C.byref(prm)) == 0


@pytest.mark.parametrize("tag", ["1x1_s2", "3x3_s2_even"])
def test_dgrad_workspace_contract(dev, ops, tag):
    from tests.test_workspace_contract_gpu import contract
    lib = L.load_library()
    x, w, g, scale, s, p = _case(tag)
    gs = [_nhwc(g).to(dev), _nhwc(g.flip(0) * 0.5).to(dev)]
    wd = ops.pack_conv_dgrad_weight(ops.pack_conv_weight(w.to(dev)), scale.to(dev))
    x_shape = (x.shape[0], x.shape[2], x.shape[3], x.shape[1])
    prm = _params(x_shape, (w.shape[0], w.shape[2], w.shape[3], w.shape[1]), s, p)
    need = lib.adaf_conv2d_dgrad_workspace_bytes(C.byref(prm))
    h = L.handle(dev)

    def call(ws, nbytes, outs, alt):
        gin = gs[1 if alt else 0]
        return lib.adaf_conv2d_dgrad_f32(h, C.byref(prm), L.ptr(gin), L.ptr(wd), L.ptr(outs["dx"]), L.ptr(ws), nbytes, L.stream_ptr())

    contract("conv_dgrad", tag, dev, need, call, {"dx": x_shape}, align=True,
             wrapper=lambda: {"dx": ops.conv2d_dgrad(gs[0], wd, x_shape, s, p)})
    prm.stride = 1
    assert lib.adaf_conv2d_dgrad_workspace_bytes(C.byref(prm)) == 0          # stride 1 needs none
