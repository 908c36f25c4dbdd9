"""Backward of the depthwise 3x3 convolution on the MI355X (csrc/dw_bwd.hip): the gather data gradient and the strip-walk
weight gradient against F.conv2d(groups=c) autograd in float64, run-to-run bit identity, the weight gradient's workspace contract, and
padding taps that are skipped rather than multiplied.

Shapes (n, hh, ww, c, stride): a map smaller than the filter, odd and even extents under stride 2, non-square maps, fewer channels than
one column chunk (16 quads) and more than one, and more pixels than one round of the pixel lanes (several slices).

Tolerance of every comparison: the error against the float64 result, relative to that quantity's largest entry, is at most 50x the
distance between the same CPU autograd in fp32 and in fp64 (G17's rule, tests/test_stage3_gpu.py); no other number appears.  The CPU
references are computed once per case and shared."""
import functools

import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib as L
from tests.helpers import rnd
from tests.trunk_walk_harness import SPREAD_FACTOR

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 16, 1), (3, 7, 7, 96, 1), (2, 7, 8, 144, 2), (2, 8, 7, 24, 2), (1, 5, 5, 960, 1), (5, 14, 14, 32, 2)]


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


def _autograd(x, w, g, stride, dtype):
    x, w = x.clone().to(dtype).requires_grad_(True), w.clone().to(dtype).requires_grad_(True)
    y = F.conv2d(x, w, None, stride, 1, groups=x.shape[1])
    dx, dw = torch.autograd.grad(y, (x, w), g.to(dtype))
    return dx, dw


@functools.lru_cache(maxsize=None)
def _case(case):
    """-> x, w (c,1,3,3), g in PyTorch's layouts and the float64 / fp32 CPU gradients, computed once."""
    n, hh, ww, c, s = case
    i = CASES.index(case)
    x = rnd((n, c, hh, ww), 4000 + i)
    w = rnd((c, 1, 3, 3), 4100 + i, 1.0 / 3.0)
    g = rnd((n, c, (hh - 1) // s + 1, (ww - 1) // s + 1), 4200 + i)
    return x, w, g, _autograd(x, w, g, s, torch.float64), _autograd(x, w, g, s, torch.float32)


def _rel(got, ref64):
    return ((got.double() - ref64).abs().max() / ref64.abs().max()).item()


def _hold(tag, got, r32, r64):
    spread, err = _rel(r32, r64), _rel(got, r64)
    print("%s: rel err %.2e, fp32-fp64 spread %.2e, ratio %.3f" % (tag, err, spread, err / spread if spread else float("inf")))
    assert torch.isfinite(got).all(), tag
    assert spread > 0 and err <= SPREAD_FACTOR * spread, (tag, err, spread)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_c%d_s%d" % c)
def test_dgrad_and_wgrad_against_fp64_autograd(dev, ops, case):
    s = case[4]
    x, w, g, (dx64, dw64), (dx32, dw32) = _case(case)
    xd, gd = _nhwc(x).to(dev), _nhwc(g).to(dev)
    w33 = ops.pack_dw_weight(w.to(dev))
    dx = ops.dwconv3x3_dgrad(gd, w33, tuple(xd.shape), s)
    assert tuple(dx.shape) == tuple(xd.shape)
    _hold("%s dgrad" % (case,), dx.permute(0, 3, 1, 2).cpu(), dx32, dx64)
    dw = ops.dwconv3x3_wgrad(xd, gd, s)
    assert tuple(dw.shape) == tuple(w.shape)
    _hold("%s wgrad" % (case,), dw.cpu(), dw32, dw64)
    # twice on the same inputs: the same bits
    assert torch.equal(dx, ops.dwconv3x3_dgrad(gd, w33, tuple(xd.shape), s))
    assert torch.equal(dw, ops.dwconv3x3_wgrad(xd, gd, s))


@pytest.mark.parametrize("case", [(2, 7, 8, 144, 2), (3, 7, 7, 96, 1)], ids=lambda c: "n%d_%dx%d_c%d_s%d" % c)
def test_padding_taps_are_skipped_not_multiplied(dev, ops, case):
    """x holds 1e30 in its border rows and g is zero wherever a window touches them, so every product that meets a 1e30 is 0 * 1e30 and
    the float64 reference stays at the size of the inner map.  The kernel reads a padding tap from a clamped address -- a border row for
    the rows above and below the map -- and must drop the term: dw finite and within the rule."""
    n, hh, ww, c, s = case
    x, w, g = (t.clone() for t in _case(case)[:3])
    x[:, :, 0, :] = 1e30
    x[:, :, -1, :] = 1e30
    oh = g.shape[2]
    for oy in range(oh):
        if oy * s - 1 <= 0 or oy * s + 1 >= hh - 1:
            g[:, :, oy, :] = 0.0
    assert g.abs().sum() > 0
    _, dw64 = _autograd(x, w, g, s, torch.float64)
    _, dw32 = _autograd(x, w, g, s, torch.float32)
    assert torch.isfinite(dw64).all() and dw64.abs().max().item() < 1e6          # the reference never met a 1e30
    dw = ops.dwconv3x3_wgrad(_nhwc(x).to(dev), _nhwc(g).to(dev), s)
    _hold("%s wgrad with 1e30 border rows" % (case,), dw.cpu(), dw32, dw64)


@pytest.mark.parametrize("case", [(3, 7, 7, 96, 1), (5, 14, 14, 32, 2)], ids=lambda c: "n%d_%dx%d_c%d_s%d" % c)
def test_wgrad_workspace_contract(dev, ops, case):
    from tests.test_workspace_contract_gpu import contract
    lib, h = L.load_library(), L.handle(dev)
    n, hh, ww, c, s = case
    x, w, g = _case(case)[:3]
    xs = [_nhwc(x).to(dev), _nhwc(x.flip(0) * 0.5).to(dev)]
    gd = _nhwc(g).to(dev)
    need = lib.adaf_dwconv3x3_wgrad_workspace_bytes(n, hh, ww, c, s)

    def call(ws, nbytes, outs, alt):
        return lib.adaf_dwconv3x3_wgrad_f32(h, L.ptr(xs[1 if alt else 0]), L.ptr(gd), n, hh, ww, c, s, L.ptr(outs["dw"]), L.ptr(ws), nbytes,
                                            L.stream_ptr())

    contract("dwconv_wgrad", "dwconv_wgrad %s" % (case,), dev, need, call, {"dw": (3, 3, c)}, align=True,
             wrapper=lambda: {"dw": ops.dwconv3x3_wgrad(xs[0], gd, s).reshape(c, 3, 3).permute(1, 2, 0).contiguous()})
    for bad in ((0, hh, ww, c, s), (n, hh, ww, c + 2, s), (n, hh, ww, c, 3)):      # descriptions the call refuses: the query says 0
        assert lib.adaf_dwconv3x3_wgrad_workspace_bytes(*bad) == 0


def test_refused_arguments(dev, ops):
    g = torch.zeros(1, 4, 4, 6, device=dev)
    with pytest.raises(L.AdafError):
        ops.dwconv3x3_dgrad(g, torch.zeros(3, 3, 6, device=dev), (1, 4, 4, 6), 1)         # c % 4
    with pytest.raises(ValueError):
        ops.dwconv3x3_dgrad(torch.zeros(1, 4, 4, 8, device=dev), torch.zeros(3, 3, 8, device=dev), (1, 8, 8, 8), 1)      # g's shape
    with pytest.raises(L.AdafError):
        ops.dwconv3x3_wgrad(torch.zeros(1, 8, 8, 8, device=dev), torch.zeros(1, 3, 3, 8, device=dev), 3)       # stride
