"""The weight gradient for output channels that do not fill a block of 32 filter rows (adaf_conv2d_wgrad_rows_f32): the
split-K core of csrc/splitk_wgrad.h with its row bound.  MobileNetV2's cout 16, 24 and 144 against F.conv2d autograd in float64; for
cout 64 and 96 the bits of conv2d_wgrad; the workspace contract.

Tolerance: the error against the float64 result, relative to the largest entry, is at most 50x the distance between the same CPU autograd
in fp32 and in fp64 (G17's rule, tests/test_stage3_gpu.py); no other number appears."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib as L
from tests.helpers import rnd
from tests.trunk_walk_harness import SPREAD_FACTOR

pytestmark = pytest.mark.gpu

# (tag, N, Cin, Cout, k, stride, pad, H, W)
CASES = [
    ("1x1_c16", 3, 32, 16, 1, 1, 0, 7, 7),
    ("1x1_c24", 3, 96, 24, 1, 1, 0, 7, 7),
    ("1x1_c144", 3, 24, 144, 1, 1, 0, 7, 7),
    ("3x3_s2_c24", 2, 8, 24, 3, 2, 1, 9, 8),
    ("1x1_c64", 3, 32, 64, 1, 1, 0, 7, 7),
    ("1x1_c96", 3, 32, 96, 1, 1, 0, 7, 7),
    ("3x3_c96", 2, 16, 96, 3, 1, 1, 6, 5),
]


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


def _case(tag):
    i = [c[0] for c in CASES].index(tag)
    _, n, cin, cout, k, s, p, hh, ww = CASES[i]
    x = rnd((n, cin, hh, ww), 5000 + i)
    g = rnd((n, cout, (hh + 2 * p - k) // s + 1, (ww + 2 * p - k) // s + 1), 5100 + i)
    return x, g, (cout, k, k, cin), s, p


def _autograd(x, g, w_shape, s, p, dtype):
    cout, k, _, cin = w_shape
    w = torch.zeros((cout, cin, k, k), dtype=dtype, requires_grad=True)
    dw, = torch.autograd.grad(F.conv2d(x.to(dtype), w, None, s, p), w, g.to(dtype))
    return dw


def _rel(got, ref64):
    return ((got.double() - ref64).abs().max() / ref64.abs().max()).item()


@pytest.mark.parametrize("tag", ["1x1_c16", "1x1_c24", "1x1_c144", "3x3_s2_c24"])
def test_narrow_cout_against_fp64_autograd(dev, ops, tag):
    x, g, w_shape, s, p = _case(tag)
    dw64, dw32 = _autograd(x, g, w_shape, s, p, torch.float64), _autograd(x, g, w_shape, s, p, torch.float32)
    xd, gd = _nhwc(x).to(dev), _nhwc(g).to(dev)
    dw = ops.conv2d_wgrad_rows(xd, gd, w_shape, s, p)
    assert tuple(dw.shape) == w_shape and torch.isfinite(dw).all()
    spread, err = _rel(dw32, dw64), _rel(dw.permute(0, 3, 1, 2).cpu(), dw64)
    print("%s wgrad_rows: rel err %.2e, fp32-fp64 spread %.2e, ratio %.3f" % (tag, err, spread, err / spread))
    assert spread > 0 and err <= SPREAD_FACTOR * spread, (tag, err, spread)
    assert torch.equal(dw, ops.conv2d_wgrad_rows(xd, gd, w_shape, s, p))          # twice on the same inputs: the same bits
    with pytest.raises(L.AdafError):
        ops.conv2d_wgrad(xd, gd, w_shape, s, p)                                    # the whole-block export still refuses it


@pytest.mark.parametrize("tag", ["1x1_c64", "1x1_c96", "3x3_c96"])
def test_whole_blocks_give_the_bits_of_conv2d_wgrad(dev, ops, tag):
    x, g, w_shape, s, p = _case(tag)
    xd, gd = _nhwc(x).to(dev), _nhwc(g).to(dev)
    lib, prm = L.load_library(), ops._bwd_params(tuple(xd.shape), w_shape, s, p)[0]
    assert lib.adaf_conv2d_wgrad_rows_workspace_bytes(C.byref(prm)) == lib.adaf_conv2d_wgrad_workspace_bytes(C.byref(prm)) > 0
    assert torch.equal(ops.conv2d_wgrad_rows(xd, gd, w_shape, s, p), ops.conv2d_wgrad(xd, gd, w_shape, s, p))


@pytest.mark.parametrize("tag", ["1x1_c24", "3x3_s2_c24", "1x1_c144"])
def test_workspace_contract(dev, ops, tag):
    from tests.test_workspace_contract_gpu import contract
    lib, h = L.load_library(), L.handle(dev)
    x, g, w_shape, s, p = _case(tag)
    xs = [_nhwc(x).to(dev), _nhwc(x.flip(0) * 0.5).to(dev)]
    gd = _nhwc(g).to(dev)
    prm = ops._bwd_params(tuple(xs[0].shape), w_shape, s, p)[0]
    need = lib.adaf_conv2d_wgrad_rows_workspace_bytes(C.byref(prm))
    assert lib.adaf_conv2d_wgrad_workspace_bytes(C.byref(prm)) == 0          # the whole-block query refuses the same description

    def call(ws, nbytes, outs, alt):
        return lib.adaf_conv2d_wgrad_rows_f32(h, C.byref(prm), L.ptr(xs[1 if alt else 0]), L.ptr(gd), L.ptr(outs["dw"]), L.ptr(ws), nbytes,
                                              L.stream_ptr())

    contract("conv_wgrad_rows", tag, dev, need, call, {"dw": w_shape}, align=True,
             wrapper=lambda: {"dw": ops.conv2d_wgrad_rows(xs[0], gd, w_shape, s, p)})
    prm.cout = 18                                                              # not a multiple of 4: refused, the query says 0
    assert lib.adaf_conv2d_wgrad_rows_workspace_bytes(C.byref(prm)) == 0
