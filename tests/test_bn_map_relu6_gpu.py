"""ReLU6 in the batch-statistics BatchNorm over maps (adaf_bn_map_train_forward_act_f32 / adaf_bn_map_train_backward_act_f32, csrc/bn_map.hip,
DESIGN 3.16): the forward clips to [0, 6], the backward passes the gradient where 0 < y < 6 on the stored output.

Reference: torch's CPU batch norm in train mode followed by the clip, and its autograd, in float64.  The backward is checked on the fp32
forward's own branches: the reference multiplies the upstream gradient by the mask 0 < y < 6 of the DEVICE's y, as tests/test_bn_map_gpu.py
masks from the device's output, so a unit whose pre-activation sits within rounding of a kink does not decide the comparison.

Tolerance: the error against the float64 result, relative to that quantity's largest entry, is at most 50x the distance between the same
CPU computation in fp32 and in fp64 (G17's rule, tests/test_stage3_gpu.py, SPREAD_FACTOR of tests/trunk_walk_harness.py).

Shapes rows x cols: (16, 16) one slice round of a narrow map, (50, 24) ragged lanes and a column count that is no multiple of 16,
(4099, 144) more rows than slices and more than one column block."""
import functools

import pytest
import torch

from adafocus_amd import _lib as L
from adafocus_amd import hip_ops
from tests.helpers import rnd
from tests.trunk_walk_harness import SPREAD_FACTOR

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-5, 0.1
SHAPES = [(16, 16), (50, 24), (4099, 144)]
ZERO_CH, SIX_CH = 1, 2          # gamma = 0 with beta = 0 / beta = 6: every output exactly 0 / exactly 6 before the clip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols):
    seed = 6000 + rows + cols
    x = rnd((rows, cols), seed) * (1 + rnd((cols,), seed + 1).abs()) + rnd((cols,), seed + 2)
    gamma, beta = 3 + 0.5 * rnd((cols,), seed + 3), 3 + 0.5 * rnd((cols,), seed + 4)      # a sixth of the units below 0, a sixth above 6
    gamma[ZERO_CH], beta[ZERO_CH] = 0.0, 0.0
    gamma[SIX_CH], beta[SIX_CH] = 0.0, 6.0
    return dict(x=x, gamma=gamma, beta=beta, rmean=0.1 * rnd((cols,), seed + 5), rvar=1 + 0.1 * rnd((cols,), seed + 6).abs(),
                res=rnd((rows, cols), seed + 7), dy=rnd((rows, cols), seed + 8))


def _reference(inp, dtype, mask, residual=False, relu6=True):
    """mask: 0 < y < 6 of the device's output (None: no activation)."""
    x, gamma, beta = (inp[k].clone().to(dtype).requires_grad_() for k in ("x", "gamma", "beta"))      # (clones: the inputs are shared)
    rmean, rvar = inp["rmean"].to(dtype).clone(), inp["rvar"].to(dtype).clone()
    z, mean, invstd = torch.native_batch_norm(x, gamma, beta, rmean, rvar, True, MOMENTUM, EPS)
    if residual:
        z = z + inp["res"].to(dtype)
    y = z.clamp(0, 6) if relu6 else z
    dy = inp["dy"].to(dtype)
    z.backward(dy if mask is None else dy * mask.to(dtype))
    return dict(y=y.detach(), mean=mean.detach(), invstd=invstd.detach(), running_mean=rmean, running_var=rvar, dx=x.grad, dgamma=gamma.grad,
                dbeta=beta.grad)


def _device(inp, dev, act, residual=False):
    x, gamma = inp["x"].to(dev), inp["gamma"].to(dev)
    rm, rv = inp["rmean"].to(dev), inp["rvar"].to(dev)
    y, mean, invstd = hip_ops.bn_map_train_forward_act(x, gamma, inp["beta"].to(dev), rm, rv, EPS, MOMENTUM,
                                                       residual=inp["res"].to(dev) if residual else None, act=act)
    dx, dgamma, dbeta = hip_ops.bn_map_train_backward_act(x, y, inp["dy"].to(dev), gamma, mean, invstd, act=act)
    return dict(y=y, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, dx=dx, dgamma=dgamma, dbeta=dbeta)


def _hold(tag, got, r64, r32):
    bad = []
    for k, v in got.items():
        scale = r64[k].abs().max().item()
        spread = (r32[k].double() - r64[k]).abs().max().item() / scale
        err = (v.double().cpu() - r64[k]).abs().max().item() / scale
        print("%-26s %-12s err %.2e  spread %.2e  ratio %.3f" % (tag, k, err, spread, err / spread if spread else float("inf")))
        assert torch.isfinite(v).all(), k
        if not (spread > 0 and err <= SPREAD_FACTOR * spread):
            bad.append((k, err, spread))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_relu6_forward_backward_against_float64(dev, rows, cols):
    inp = _inputs(rows, cols)
    got = _device(inp, dev, L.ACT_RELU6)
    y = got["y"].cpu()
    assert y.min().item() == 0.0 and y.max().item() == 6.0 and ((y > 0) & (y < 6)).any()          # both kinks are met
    mask = (y > 0) & (y < 6)
    r64, r32 = (_reference(inp, dt, mask) for dt in (torch.float64, torch.float32))
    _hold("%d x %d relu6" % (rows, cols), got, r64, r32)
    # the planted channels: exactly 0 and exactly 6 before the clip, on the closed side of both kinks
    assert not y[:, ZERO_CH].any() and bool((y[:, SIX_CH] == 6.0).all())
    for ch in (ZERO_CH, SIX_CH):
        assert not got["dx"][:, ch].any() and got["dbeta"][ch].item() == 0.0 and got["dgamma"][ch].item() == 0.0
    again = _device(inp, dev, L.ACT_RELU6)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_relu6_after_a_residual(dev):
    """The residual joins in front of the clip (the walk does not use it, the kernel allows it)."""
    inp = _inputs(50, 24)
    got = _device(inp, dev, L.ACT_RELU6, residual=True)
    y = got["y"].cpu()
    mask = (y > 0) & (y < 6)
    r64, r32 = (_reference(inp, dt, mask, residual=True) for dt in (torch.float64, torch.float32))
    _hold("50 x 24 residual relu6", got, r64, r32)


def test_no_activation_with_a_residual_against_float64(dev):
    """ADAF_ACT_NONE with the identity as residual: a project layer of a block with use_res_connect."""
    inp = _inputs(4099, 144)
    got = _device(inp, dev, L.ACT_NONE, residual=True)
    r64, r32 = (_reference(inp, dt, None, residual=True, relu6=False) for dt in (torch.float64, torch.float32))
    _hold("4099 x 144 residual none", got, r64, r32)
    assert (got["y"] < 0).any() and (got["y"] > 6).any()


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("residual", [False, True])
def test_relu_and_none_give_the_bits_of_the_exports_without_act(dev, rows, cols, residual):
    inp = _inputs(rows, cols)
    x, gamma, beta, dy = (inp[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
    res = inp["res"].to(dev) if residual else None
    for act, relu in ((L.ACT_RELU, True), (L.ACT_NONE, False)):
        rm0, rv0, rm1, rv1 = (inp[k].to(dev) for k in ("rmean", "rvar", "rmean", "rvar"))
        old = hip_ops.bn_map_train_forward(x, gamma, beta, rm0, rv0, EPS, MOMENTUM, residual=res, relu=relu)
        new = hip_ops.bn_map_train_forward_act(x, gamma, beta, rm1, rv1, EPS, MOMENTUM, residual=res, act=act)
        for a, b in zip(old + (rm0, rv0), new + (rm1, rv1)):
            assert torch.equal(a, b)
        y, mean, invstd = old
        old_b = hip_ops.bn_map_train_backward(x, y if relu else None, dy, gamma, mean, invstd)
        new_b = hip_ops.bn_map_train_backward_act(x, y, dy, gamma, mean, invstd, act=act)
        for a, b in zip(old_b, new_b):
            assert torch.equal(a, b)


def test_refused_arguments(dev):
    x = torch.zeros(8, 16, device=dev)
    v = torch.ones(16, device=dev)
    with pytest.raises(ValueError):
        hip_ops.bn_map_train_forward_act(x, v, v, act=L.ACT_SWISH)
    with pytest.raises(ValueError):
        hip_ops.bn_map_train_backward_act(x, None, x, v, v, v, act=L.ACT_RELU6)
    lib, h = L.load_library(), L.handle(dev)
    ws = torch.empty(lib.adaf_bn_map_workspace_bytes(8, 16) // 4, device=dev)
    y, m, i = torch.empty_like(x), torch.empty_like(v), torch.empty_like(v)
    rc = lib.adaf_bn_map_train_forward_act_f32(h, L.ptr(x), 8, 16, L.ptr(v), L.ptr(v), EPS, MOMENTUM, None, None, None, L.ACT_SIGMOID, L.ptr(y),
                                               L.ptr(m), L.ptr(i), L.ptr(ws), ws.numel() * 4, L.stream_ptr())
    assert rc == -1                                                  # ADAF_E_BADARG
    rc = lib.adaf_bn_map_train_backward_act_f32(h, L.ptr(x), None, L.ACT_RELU, L.ptr(x), 8, 16, L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(y), L.ptr(m),
                                                L.ptr(i), L.ptr(ws), ws.numel() * 4, L.stream_ptr())
    assert rc == -1
    torch.cuda.synchronize()
