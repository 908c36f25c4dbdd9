"""adaf_ce_steps_f32 / hip_ops.ce_steps / hip_ops.CeStepsFn on the MI355X: the stage-1 loss, the mean cross-entropy of every
step's logits against its clip's label, with its gradient.

Accuracy: torch's float64 F.cross_entropy and its autograd on the CPU are the reference, under the single-reduction rule of
tests/heads_reference.py: err = max |got - f64| / max |f64| <= max(2^-22, 8 x the same distance of torch's own fp32 CPU result), for the
loss and for dlogits.  Everything else here is exact (torch.equal, NaN where specified, return codes)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib as L
from tests.heads_reference import FLOOR, SINGLE_FACTOR
from tests.helpers import rnd
from tests.test_workspace_contract_gpu import E_BADARG, E_LAYOUT, E_NOMEM, OK, contract

pytestmark = pytest.mark.gpu

# (B, T, C): one row of two classes; a small odd one; the shipped stage-1 class count; FCVID's; the lane-strided sum's edge (one column per
# lane / one lane with two); 258 rows = the second level of the row sum; one GPU's share of a 128-clip batch
SHAPES = [(1, 1, 2), (2, 3, 10), (3, 16, 200), (2, 5, 239), (5, 4, 64), (5, 4, 65), (129, 2, 7), (64, 16, 200)]
DATA = ["unit", "shifted", "equal_maxima", "target_100_below"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


def _case(shape, data):
    """(logits (B*T, C) fp32, target (B,) int64) on the CPU: unit-variance logits; "shifted": whole rows moved by +1e4 (even rows) and -1e4
    (odd rows); "equal_maxima": row 0 has its maximum twice; "target_100_below": the last row's target logit is 100 below its maximum."""
    b, t, c = shape
    seed = 2300 + 7 * b + 3 * t + c
    logits = rnd((b * t, c), seed)
    target = torch.from_numpy(np.random.Generator(np.random.PCG64([seed + 1, 0xBEEF])).integers(0, c, size=b, dtype=np.int64))
    if data == "shifted":
        logits = logits.clone()
        logits[0::2] += 1e4
        logits[1::2] -= 1e4
    elif data == "equal_maxima":
        logits = logits.clone()
        top = logits[0].max() + 1
        logits[0, 0] = logits[0, c - 1] = top
    elif data == "target_100_below":
        logits = logits.clone()
        tg = int(target[b - 1])
        other = (tg + 1) % c
        logits[-1, other] = logits[-1].max() + 0.5
        logits[-1, tg] = logits[-1, other] - 100
    return logits, target


def _reference(logits, target, steps, dtype):
    l = logits.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(l, target.repeat_interleave(steps))
    loss.backward()
    return loss.detach().reshape(1), l.grad


def _rel(got, ref):
    scale = ref.abs().max().item()
    return (got.double().cpu() - ref).abs().max().item() / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-T%d-C%d" % s)
def test_loss_and_gradient_against_float64(dev, ops, shape, data):
    b, t, c = shape
    logits, target = _case(shape, data)
    loss64, d64 = _reference(logits, target, t, torch.float64)
    loss32, d32 = _reference(logits, target, t, torch.float32)
    loss, dlogits = ops.ce_steps(logits.to(dev), target.to(dev), t)
    assert loss.shape == (1,) and dlogits.shape == (b * t, c)
    for tag, got, f32, f64 in (("loss", loss, loss32, loss64), ("dlogits", dlogits, d32, d64)):
        spread, err = _rel(f32, f64), _rel(got, f64)
        print("%s %s %s: err %.3e, torch fp32 %.3e, bound %.3e" % (shape, data, tag, err, spread, max(FLOOR, SINGLE_FACTOR * spread)))
        assert err <= max(FLOOR, SINGLE_FACTOR * spread), (tag, err, spread)


def test_single_class_is_exactly_zero(dev, ops):
    logits = rnd((6, 1), 2390).to(dev)
    loss, dlogits = ops.ce_steps(logits, torch.zeros(2, dtype=torch.int64, device=dev), 3)
    assert loss.item() == 0.0 and not dlogits.any()


@pytest.mark.parametrize("shape", [(3, 16, 200), (129, 2, 7)], ids=lambda s: "B%d-T%d-C%d" % s)
def test_expanded_target_and_rerun_give_the_same_bits(dev, ops, shape):
    b, t, c = shape
    logits, target = _case(shape, "unit")
    logits, target = logits.to(dev), target.to(dev)
    loss, dlogits = ops.ce_steps(logits, target, t)
    flat = ops.ce_steps(logits, target.repeat_interleave(t), 1)
    again = ops.ce_steps(logits, target, t)
    for other in (flat, again):
        assert torch.equal(other[0], loss) and torch.equal(other[1], dlogits)
    only_loss, none = ops.ce_steps(logits, target, t, want_grad=False)            # dlogits_out = NULL
    assert none is None and torch.equal(only_loss, loss)


@pytest.mark.parametrize("bad", [-1, 10])
def test_target_out_of_range_poisons_its_clip_only(dev, ops, bad):
    b, t, c = 3, 4, 10
    logits = rnd((b * t, c), 2391).to(dev)
    good = ops.ce_steps(logits, torch.tensor([2, 0, 5], device=dev), t)
    loss, dlogits = ops.ce_steps(logits, torch.tensor([2, bad, 5], device=dev), t)
    assert torch.isnan(loss).all()
    assert torch.isnan(dlogits[t:2 * t]).all()
    assert torch.equal(dlogits[:t], good[1][:t]) and torch.equal(dlogits[2 * t:], good[1][2 * t:])
    assert torch.isfinite(good[0]).all() and torch.isfinite(good[1]).all()


def test_autograd_function_scales_the_stored_gradient(dev, ops):
    b, t, c = 2, 3, 10
    logits, target = _case((b, t, c), "unit")
    target = target.to(dev)
    leaf = logits.to(dev).requires_grad_(True)
    loss = ops.CeStepsFn.apply(leaf, target, t)
    (2 * loss).backward()
    want_loss, want = ops.ce_steps(leaf.detach(), target, t)
    assert torch.equal(loss.detach(), want_loss) and torch.equal(leaf.grad, 2 * want)


@pytest.mark.parametrize("shape", [(3, 16, 200), (129, 2, 7)], ids=lambda s: "B%d-T%d-C%d" % s)
def test_workspace_contract(dev, ops, shape):
    b, t, c = shape
    lib = L.load_library()
    need = lib.adaf_ce_steps_workspace_bytes(b, t)
    assert need == b * t * 4
    inputs = [(l.to(dev), tg.to(dev)) for l, tg in (_case(shape, "unit"), _case(shape, "equal_maxima"))]

    def call(ws, nbytes, outs, alt):
        l, tg = inputs[1 if alt else 0]
        return lib.adaf_ce_steps_f32(L.handle(dev), L.ptr(l), L.ptr(tg), b, t, c, outs["loss"].data_ptr(), outs["dlogits"].data_ptr(),
                                     ws.data_ptr(), nbytes, L.stream_ptr())

    def wrapper():
        loss, dlogits = ops.ce_steps(*inputs[0], t)
        return {"loss": loss, "dlogits": dlogits}

    contract("ce_steps", "ce_steps B%d T%d C%d" % shape, dev, need, call, {"loss": (1,), "dlogits": (b * t, c)}, wrapper=wrapper, align=True)


def test_error_codes(dev):
    lib = L.load_library()
    h = L.handle(dev)
    b, t, c = 2, 3, 10
    l = rnd((b * t, c), 2392).to(dev)
    tg = torch.tensor([1, 2], device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    d = torch.full((b * t, c), 7.0, device=dev)
    ws = torch.empty(64, device=dev)
    need = lib.adaf_ce_steps_workspace_bytes(b, t)
    st = L.stream_ptr()

    def run(handle=h, logits=l, target=tg, bb=b, tt=t, cc=c, out=loss, ws_ptr=None, nbytes=need):
        return lib.adaf_ce_steps_f32(handle, L.ptr(logits), L.ptr(target), bb, tt, cc, L.ptr(out), L.ptr(d), ws.data_ptr() if ws_ptr is None else ws_ptr,
                                     nbytes, st)

    assert run(handle=None) == E_BADARG
    assert run(logits=None) == E_BADARG and run(target=None) == E_BADARG and run(out=None) == E_BADARG and run(ws_ptr=C.c_void_p(None)) == E_BADARG
    for kw in ({"bb": 0}, {"tt": 0}, {"cc": 0}, {"bb": -2}):
        assert run(**kw) == E_BADARG, kw
    assert run(nbytes=need - 4) == E_NOMEM
    assert run(ws_ptr=ws.data_ptr() + 4) == E_LAYOUT
    torch.cuda.synchronize()
    assert (loss == 7.0).all() and (d == 7.0).all()                  # nothing was launched by a refused call
    assert run() == OK
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(d).all()
