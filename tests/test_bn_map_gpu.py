"""BatchNorm with batch statistics over tall pixel-major maps (csrc/bn_map.hip): the kernels alone.

Reference and bound.  Every case is compared with torch's CPU batch norm in train mode (+ residual + ReLU) and its autograd in float64.
The bound is the BatchNorm rule of DESIGN 3.12: the error against float64 is at most 8x the distance of torch's own fp32 run from
float64 on the same inputs, for each of y, mean, invstd, the running statistics, dx, dgamma and dbeta, all relative to the quantity's
scale (its largest float64 entry).  A quantity torch's fp32 run gets exactly (two rows: a sum of two values is exact) or nearly so
gets the floor 2^-22 of its scale: four units in the last place of an fp32 number of that size, what the two or three fp32 roundings
between the double statistics and a stored value may cost.  dx of a two-row map is pure cancellation -- xhat is +-1 and
n dy - dbeta - xhat dgamma vanishes up to eps --, so its scale is that of the terms that cancel, max |gamma invstd| max |dy|.
The CPU references are computed once per case and shared.

Shapes: the smallest at which these kernels can go wrong -- 64, 256 and 2048 columns (both column-chunk widths, one and eight column
blocks), 2 and 16 rows, one row fewer and one more than the slice count (2048, 2048, 256), rows that leave the last used slice and the
row lanes ragged, 40 013 x 64 (twenty rows per slice), and one map past 2^32 bytes."""
import ctypes

import pytest
import torch

from adafocus_amd import _lib as L
from adafocus_amd import hip_ops
from tests.helpers import rnd

pytestmark = pytest.mark.gpu

FACTOR = 8
FLOOR = 2.0 ** -22
EPS, MOMENTUM = 1e-5, 0.1
SLICES = {64: 2048, 256: 2048, 2048: 256}        # bn_map_slices(cols): about 2048 blocks over the column blocks
E_BADARG, E_LAYOUT, E_NOMEM = -1, -2, -6

SHAPES = [(2, 64), (2, 256), (2, 2048), (16, 64), (16, 256), (16, 2048), (2047, 64), (2049, 64), (2047, 256), (2049, 256), (255, 2048),
          (257, 2048), (5000, 64), (4102, 256), (777, 2048), (40013, 64)]
# (residual, relu, running statistics): the variants, on a small map and on one with a slice per row
VARIANTS = [(False, False, True), (False, True, True), (True, False, True), (True, True, False)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _inputs(rows, cols, seed, ratio=None):
    """x with per-column spread and offset, a gamma = 0 channel and a negative gamma; ratio: columns 0, 3, 6, ... get a mean of `ratio`
    standard deviations."""
    std = 1 + rnd((cols,), seed + 1).abs()
    mean = rnd((cols,), seed + 2)
    if ratio is not None:
        mean = torch.where(torch.arange(cols) % 3 == 0, ratio * std, mean)
    x = rnd((rows, cols), seed) * std + mean
    gamma, beta = 1 + 0.1 * rnd((cols,), seed + 3), 0.1 * rnd((cols,), seed + 4)
    gamma[1], gamma[2] = 0.0, -gamma[2].abs() - 0.5
    return dict(x=x, gamma=gamma, beta=beta, rmean=0.1 * rnd((cols,), seed + 5), rvar=1 + 0.1 * rnd((cols,), seed + 6).abs(),
                res=rnd((rows, cols), seed + 7), dy=rnd((rows, cols), seed + 8))


def _reference(inp, dtype, residual, relu):
    x = inp["x"].to(dtype).requires_grad_()
    gamma, beta = inp["gamma"].to(dtype).requires_grad_(), inp["beta"].to(dtype).requires_grad_()
    rmean, rvar = inp["rmean"].to(dtype).clone(), inp["rvar"].to(dtype).clone()
    y, mean, invstd = torch.native_batch_norm(x, gamma, beta, rmean, rvar, True, MOMENTUM, EPS)
    if residual:
        y = y + inp["res"].to(dtype)
    if relu:
        y = torch.relu(y)
    y.backward(inp["dy"].to(dtype))
    return dict(y=y.detach(), mean=mean.detach(), invstd=invstd.detach(), running_mean=rmean, running_var=rvar, dx=x.grad, dgamma=gamma.grad,
                dbeta=beta.grad)


def _device(inp, dev, residual, relu, running=True):
    x, gamma = inp["x"].to(dev), inp["gamma"].to(dev)
    rm, rv = (inp["rmean"].to(dev), inp["rvar"].to(dev)) if running else (None, None)
    y, mean, invstd = hip_ops.bn_map_train_forward(x, gamma, inp["beta"].to(dev), rm, rv, EPS, MOMENTUM, residual=inp["res"].to(dev) if residual else None,
                                                   relu=relu)
    dx, dgamma, dbeta = hip_ops.bn_map_train_backward(x, y if relu else None, inp["dy"].to(dev), gamma, mean, invstd)
    out = dict(y=y, mean=mean, invstd=invstd, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if running:
        out.update(running_mean=rm, running_var=rv)
    return out


def _scale(k, r64, inp):
    s = r64[k].abs().max().item()
    if k == "dx":        # the terms dx is the difference of (module docstring)
        s = max(s, (inp["gamma"].double() * r64["invstd"]).abs().max().item() * inp["dy"].abs().max().item())
    return s


def _hold(tag, got, r64, r32, inp):
    bad = []
    for k, v in got.items():
        scale = _scale(k, r64, inp)
        assert scale > 0, k
        spread = (r32[k].double() - r64[k]).abs().max().item() / scale
        tol = max(FACTOR * spread, FLOOR)
        err = (v.double().cpu() - r64[k]).abs().max().item() / scale
        print("%-22s %-12s err %.2e  torch fp32 %.2e  tol %.2e" % (tag, k, err, spread, tol))
        assert torch.isfinite(v).all(), k
        if not err <= tol:
            bad.append((k, err, tol))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_forward_backward_against_float64(dev, rows, cols):
    """Residual + ReLU on every shape; two runs give the same bits."""
    inp = _inputs(rows, cols, 100 + rows % 97 + cols)
    r64, r32 = (_reference(inp, dt, True, True) for dt in (torch.float64, torch.float32))
    assert (r64["y"] == 0).any() and (r64["y"] > 0).any()
    a, b = _device(inp, dev, True, True), _device(inp, dev, True, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    _hold("%d x %d" % (rows, cols), a, r64, r32, inp)
    assert a["dgamma"][1].item() != 0.0 and not a["dx"][:, 1].any()          # the gamma = 0 channel: a dgamma, no dx


@pytest.mark.parametrize("residual,relu,running", VARIANTS)
@pytest.mark.parametrize("rows,cols", [(16, 256), (2049, 64)])
def test_variants(dev, rows, cols, residual, relu, running):
    inp = _inputs(rows, cols, 300 + cols)
    r64, r32 = (_reference(inp, dt, residual, relu) for dt in (torch.float64, torch.float32))
    got = _device(inp, dev, residual, relu, running)
    assert ("running_mean" in got) == running
    _hold("%d x %d res %d relu %d" % (rows, cols, residual, relu), got, r64, r32, inp)


@pytest.mark.parametrize("ratio", [1e3, 1e4])
def test_columns_far_from_zero(dev, ratio):
    """THE PASS-COUNT DECISION: a third of the columns has a mean of 10^3 / 10^4 standard deviations.  The single pass
    over x holds the bound because its sums are of x - x[0, column]; the plain sum of squares loses 6 / 8 digits of the variance."""
    rows, cols = 40013, 64
    inp = _inputs(rows, cols, 500, ratio=ratio)
    r64, r32 = (_reference(inp, dt, False, True) for dt in (torch.float64, torch.float32))
    got = _device(inp, dev, False, True)
    _hold("mean / std %g" % ratio, got, r64, r32, inp)
    # per column, not only against the largest entry: the far columns' invstd and the near columns' mean
    far = torch.arange(cols) % 3 == 0
    for k in ("invstd", "mean", "running_var"):
        rel = ((got[k].double().cpu() - r64[k]) / r64[k]).abs()
        rel32 = ((r32[k].double() - r64[k]) / r64[k]).abs()
        for sel in (far, ~far):
            tol = max(FACTOR * rel32[sel].max().item(), FLOOR)
            assert rel[sel].max().item() <= tol, (k, rel[sel].max().item(), tol)


def _raw_forward(lib, h, x, gamma, beta, y, mean, invstd, ws_ptr, ws_bytes, rows=None, cols=None):
    rows, cols = (x.shape[0] if rows is None else rows), (x.shape[1] if cols is None else cols)
    return lib.adaf_bn_map_train_forward_f32(h, L.ptr(x), rows, cols, L.ptr(gamma), L.ptr(beta), EPS, MOMENTUM, None, None, None, 1, L.ptr(y),
                                             L.ptr(mean), L.ptr(invstd), ws_ptr, ws_bytes, L.stream_ptr())


def _raw_backward(lib, h, x, y, dy, gamma, mean, invstd, dx, dgamma, dbeta, ws_ptr, ws_bytes, rows=None, cols=None):
    rows, cols = (x.shape[0] if rows is None else rows), (x.shape[1] if cols is None else cols)
    return lib.adaf_bn_map_train_backward_f32(h, L.ptr(x), L.ptr(y), L.ptr(dy), rows, cols, L.ptr(gamma), L.ptr(mean), L.ptr(invstd), L.ptr(dx),
                                              L.ptr(dgamma), L.ptr(dbeta), ws_ptr, ws_bytes, L.stream_ptr())


@pytest.mark.parametrize("rows,cols", [(333, 64), (300, 2048)])
def test_workspace_contract(dev, rows, cols):
    """Exact bytes suffice, one byte fewer is ADAF_E_NOMEM, a misaligned pointer ADAF_E_LAYOUT; what the workspace holds on entry does not
    matter (NaN-filled and zero-filled give the same bits) and nothing is written past the bytes asked for."""
    lib, h = L.load_library(), L.handle(dev)
    need = lib.adaf_bn_map_workspace_bytes(rows, cols)
    assert need == 2 * SLICES[cols] * cols * 8 and need % 16 == 0
    inp = _inputs(rows, cols, 700)
    x, gamma, beta, dy = (inp[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
    guard = 64
    runs = []
    for fill in (float("nan"), 0.0):
        buf = torch.full(((need + guard) // 4,), fill, device=dev, dtype=torch.float32)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, invstd, dgamma, dbeta = (torch.empty(cols, device=dev) for _ in range(4))
        assert _raw_forward(lib, h, x, gamma, beta, y, mean, invstd, L.ptr(buf), need) == 0
        assert _raw_backward(lib, h, x, y, dy, gamma, mean, invstd, dx, dgamma, dbeta, L.ptr(buf), need) == 0
        torch.cuda.synchronize()
        tail = buf[need // 4:]
        assert bool(torch.isnan(tail).all()) if fill != fill else not tail.any(), "written past the workspace"
        runs.append((y, mean, invstd, dx, dgamma, dbeta))
        assert _raw_forward(lib, h, x, gamma, beta, y, mean, invstd, L.ptr(buf), need - 1) == E_NOMEM
        assert _raw_backward(lib, h, x, y, dy, gamma, mean, invstd, dx, dgamma, dbeta, L.ptr(buf), need - 1) == E_NOMEM
        assert _raw_forward(lib, h, x, gamma, beta, y, mean, invstd, ctypes.c_void_p(buf.data_ptr() + 4), need) == E_LAYOUT
        assert _raw_backward(lib, h, x, y, dy, gamma, mean, invstd, dx, dgamma, dbeta, ctypes.c_void_p(buf.data_ptr() + 4), need) == E_LAYOUT
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_refused_arguments(dev):
    lib, h = L.load_library(), L.handle(dev)
    for bad in ((0, 64), (64, 0), (-1, 64)):
        assert lib.adaf_bn_map_workspace_bytes(*bad) == 0
    x = torch.zeros(8, 64, device=dev)
    v = torch.ones(64, device=dev)
    ws = torch.empty(lib.adaf_bn_map_workspace_bytes(8, 64) // 4, device=dev)
    nb = ws.numel() * 4
    out = (torch.empty_like(x), torch.empty_like(v), torch.empty_like(v))
    grads = (torch.empty_like(x), torch.empty_like(v), torch.empty_like(v))
    for rows, cols, code in ((1, 64, E_BADARG), (0, 64, E_BADARG), (8, 0, E_BADARG), (8, 62, E_LAYOUT), (8, 6, E_LAYOUT)):
        assert _raw_forward(lib, h, x, v, v, *out, L.ptr(ws), nb, rows, cols) == code, (rows, cols)
        assert _raw_backward(lib, h, x, x, x, v, v, v, *grads, L.ptr(ws), nb, rows, cols) == code, (rows, cols)
    assert _raw_forward(lib, h, x, v, v, *out, L.ptr(ws), nb) == 0
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hip_ops.bn_map_train_forward(x[:1], v, v)
    with pytest.raises(L.AdafError):
        hip_ops.bn_map_train_forward(torch.zeros(8, 62, device=dev), torch.ones(62, device=dev), torch.ones(62, device=dev))
    torch.cuda.synchronize()


def test_map_past_4_gib(dev):
    """4 200 000 x 256 floats are 4.3 GB: every offset past 2^32 bytes.  The map is generated on the device; its per-column statistics and
    a strided sample of y (rows from both ends and across the 2^32-byte line) are held to float64 computed on the device, under the same
    rule with torch's fp32 reductions on the device as the fp32 yardstick."""
    rows, cols = 4_200_000, 256
    assert rows * cols * 4 > 2 ** 32
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.empty((rows, cols), device=dev)
    chunk = 600_000
    for r in range(0, rows, chunk):       # (in chunks: the generator's temporaries stay small)
        x[r:r + chunk].normal_(generator=g)
    x.mul_(1 + torch.arange(cols, device=dev).remainder(5).float()).add_(torch.arange(cols, device=dev).float() * 0.25 - 8)
    gamma = (1 + 0.1 * rnd((cols,), 901)).to(dev)
    beta = (0.1 * rnd((cols,), 902)).to(dev)
    rm, rv = torch.zeros(cols, device=dev), torch.ones(cols, device=dev)
    y, mean, invstd = hip_ops.bn_map_train_forward(x, gamma, beta, rm, rv, EPS, MOMENTUM, relu=True)
    # float64 on the device, column chunks of 32 (1 GB of doubles at a time)
    m64, v64 = torch.empty(cols, dtype=torch.float64, device=dev), torch.empty(cols, dtype=torch.float64, device=dev)
    for c in range(0, cols, 32):
        xd = x[:, c:c + 32].double()
        m64[c:c + 32] = xd.mean(0)
        v64[c:c + 32] = xd.var(0, unbiased=False)
        del xd
    i64 = 1 / torch.sqrt(v64 + EPS)
    v32, m32 = torch.var_mean(x, 0, unbiased=False)
    i32 = 1 / torch.sqrt(v32 + EPS)
    ref = dict(mean=(mean, m64, m32), invstd=(invstd, i64, i32), running_mean=(rm, MOMENTUM * m64, MOMENTUM * m32),
               running_var=(rv, (1 - MOMENTUM) + MOMENTUM * v64 * rows / (rows - 1), (1 - MOMENTUM) + MOMENTUM * v32 * rows / (rows - 1)))
    for k, (got, r64, r32) in ref.items():
        scale = r64.abs().max().item()
        tol = max(FACTOR * (r32.double() - r64).abs().max().item() / scale, FLOOR)
        err = (got.double() - r64).abs().max().item() / scale
        print("%-12s err %.2e tol %.2e" % (k, err, tol))
        assert err <= tol, (k, err, tol)
    line = 2 ** 32 // (cols * 4)           # the row that holds byte 2^32
    sample = torch.cat([torch.arange(0, rows, 4099, device=dev), torch.arange(line - 3, line + 3, device=dev), torch.tensor([rows - 1], device=dev)])
    xs = x[sample].double()
    y64 = torch.relu((xs - m64) * i64 * gamma.double() + beta.double())
    y32 = torch.relu((x[sample] - m32) * i32 * gamma + beta)
    scale = y64.abs().max().item()
    tol = max(FACTOR * (y32.double() - y64).abs().max().item() / scale, FLOOR)
    err = (y[sample].double() - y64).abs().max().item() / scale
    print("y sample     err %.2e tol %.2e" % (err, tol))
    assert err <= tol and (y64 > 0).any() and (y64 == 0).any()
    # the backward reaches every row too: dbeta of dy = 1 under the mask counts the positive outputs, exactly (integers below 2^24)
    dx, dgamma, dbeta = hip_ops.bn_map_train_backward(x, y, torch.ones_like(y), gamma, mean, invstd)
    assert torch.equal(dbeta, (y > 0).sum(0).float())
    assert torch.isfinite(dx[sample]).all()
