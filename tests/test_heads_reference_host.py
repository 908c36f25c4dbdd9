"""The float64 references of tests/heads_reference.py checked against torch's own modules, and every case table of
tests/test_heads_domain_gpu.py checked for what makes a wrong kernel visible -- reference only, no GPU."""
import numpy as np
import pytest
import torch

from tests import heads_reference as R
from tests.helpers import rnd


def _modules(f, h, c, params):
    gru = torch.nn.GRU(f, h, batch_first=True).double()
    fc = torch.nn.Linear(h, c).double()
    with torch.no_grad():
        for dst, src in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, fc.weight, fc.bias), params):
            dst.copy_(src.double())
    return gru, fc


@pytest.mark.parametrize("with_h0", [False, True])
def test_written_out_gru_is_nn_gru(with_h0):
    b, t, f, h, c = 4, 5, 12, 24, 7
    params = R.cls_params(f, h, c, 11)
    x = rnd((b, t, f), 12)
    h0 = rnd((b, h), 13) if with_h0 else None
    gru, _ = _modules(f, h, c, params)
    want, _ = gru(x.double(), None if h0 is None else h0.double().unsqueeze(0))
    got = R.gru_seq(x, *params[:4], h0=h0)
    assert got.dtype == torch.float64 and got.shape == (b, t, h)
    assert (got - want.detach()).abs().max().item() < 1e-12
    assert want.abs().max().item() > 0.1


def test_reference_gradients_are_nn_gru_plus_linear_autograd():
    b, t, f, h, c = 4, 5, 12, 24, 7
    params = R.cls_params(f, h, c, 21)
    x, mask, dlogits = rnd((b, t, f), 22), R.dropout_mask(b, t, h, 23), rnd((b * t, c), 24)
    got = R.gru_cls_grads(x, params, mask, dlogits)
    gru, fc = _modules(f, h, c, params)
    xs = x.double().requires_grad_(True)
    logits = fc((gru(xs)[0] * mask.double()).reshape(b * t, h))
    logits.backward(dlogits.double())
    want = {"logits": logits.detach(), "dx": xs.grad, "gru.weight_ih_l0": gru.weight_ih_l0.grad, "gru.weight_hh_l0": gru.weight_hh_l0.grad,
            "gru.bias_ih_l0": gru.bias_ih_l0.grad, "gru.bias_hh_l0": gru.bias_hh_l0.grad, "fc.weight": fc.weight.grad, "fc.bias": fc.bias.grad}
    assert set(got) == set(want) == set(R.STAGE3_OUTPUTS)
    for k in want:
        assert want[k].abs().max().item() > 1e-3, k
        assert (got[k] - want[k]).abs().max().item() < 1e-12 * max(1.0, want[k].abs().max().item()), k


def test_tolerance_rule():
    assert R.FLOOR == 2.0 ** -22 and R.SINGLE_FACTOR == 8 and R.RECURRENCE_FACTOR == 50
    assert R.bound_single(0.0) == R.FLOOR and R.bound_single(1e-6) == 8e-6 and R.bound_recurrence(1e-7) == 50 * 1e-7
    r = R.measure(lambda dt: {"a": torch.tensor([1.0, 3.0]).to(dt) / 3, "z": torch.zeros(2, dtype=dt)})
    assert 0 < r.spread["a"] < 1e-7 and r.scale["a"] == 1.0 and r.scale["z"] == 1.0 and r.spread["z"] == 0.0
    assert R.rel_err(torch.tensor([1 / 3, 1.5]), r, "a") == pytest.approx(0.5)


def _visible(r, names=None, floor=1e-3):
    for k in names or r.ref:
        assert np.isfinite(r.spread[k]) and r.spread[k] > 0, (k, r.spread[k])
        assert r.ref[k].abs().max().item() > floor, (k, r.ref[k].abs().max().item())


def _columns_differ(logits):
    """No two class columns hold the same values: swapped or duplicated columns change the result."""
    c = logits.shape[1]
    assert torch.unique(logits.t().contiguous(), dim=0).shape[0] == c


@pytest.mark.parametrize("c,fin,rows", R.LINEAR_CASES)
def test_linear_cases(c, fin, rows):
    _, r = R.linear_case(c, fin, rows)
    _visible(r)
    assert r.ref["y"].shape == (rows, c)
    _columns_differ(r.ref["y"])


def test_linear_table():
    assert len(R.LINEAR_CASES) == 30 and len(set(R.LINEAR_CASES)) == 30
    assert all(fin % 64 == 0 and fin >= 512 for _, fin, _ in R.LINEAR_CASES)      # the small-batch form takes every one of them
    assert {rows for _, _, rows in R.LINEAR_CASES} == {1, 16, 37, 128, 129}        # both sides of linear_launch's 128-row switch


@pytest.mark.parametrize("k", R.GRU_CASES, ids=R.gru_case_id)
def test_gru_cases(k):
    (x, h0, params), r = R.gru_case(k)
    _visible(r)
    assert r.ref["logits"].shape == (k.b * k.t, k.c) and r.ref["hs_h0"].shape == (k.b, k.t, k.h)
    _columns_differ(r.ref["logits"])
    # the initial state matters at every step, the last one included
    no_h0 = R.gru_seq(x, *params[:4])
    assert (no_h0[:, -1] - r.ref["hs_h0"][:, -1]).abs().max().item() > (1e-3 if k.t < 100 else 0)


def test_gru_table():
    assert len(R.GRU_CASES) == 21 and len(set(R.GRU_CASES)) == 21
    assert [R.barrier_layout(k.b, k.t) for k in R.GRU_BARRIER_CASES] == ["padded", "packed", "packed", "flat"]
    assert all(17 * (k.t + 1) > 3072 * k.b for k in R.GRU_BARRIER_CASES[3:]) and 17 * (179 + 1) <= 3072
    assert sorted(-(-k.c // 128) for k in R.GRU_CLASS_CASES) == [1, 1, 1, 2, 2, 8, 8, 9]          # classes per block; 9 must fall back
    assert [k.b for k in R.GRU_BATCH_CASES] == [32, 33, 129, 256, 257]


@pytest.mark.parametrize("k", R.STAGE3_CASES, ids=lambda k: "B%d-T%d-H%d-C%d" % k)
def test_stage3_cases(k):
    (x, params, mask, dlogits), r = R.stage3_case(k)
    assert set(r.ref) == set(R.STAGE3_OUTPUTS)
    names = [n for n in R.STAGE3_OUTPUTS if not (k.t == 1 and n == "gru.weight_hh_l0")]      # one step from h = 0: no gradient for W_hh
    _visible(r, names)
    _columns_differ(r.ref["logits"])
    assert 0.3 < float((mask == 0).float().mean()) < 0.7 and set(mask.unique().tolist()) == {0.0, 2.0}
    for n in names:
        assert r.ref[n].shape == dict(zip(R.STAGE3_OUTPUTS, (dlogits, x) + params))[n].shape, n


@pytest.mark.parametrize("c,t,tg,glob", R.MEANPOOL_CASES)
def test_meanpool_cases(c, t, tg, glob):
    (feat, w, b, glog), r = R.meanpool_case(c, t, tg, glob)
    _visible(r)
    assert r.ref["out"].shape == (R.MEANPOOL_B, c) and (glog is not None) == glob
    _columns_differ(r.ref["out"])
    if glob:
        assert glog.shape == (R.MEANPOOL_B, tg, c)
        if tg != t:           # dividing the global sum by T instead of Tg is far outside the bound
            wrong = r.ref["out"] - glog.double().mean(1) + glog.double().sum(1) / t
            assert (wrong - r.ref["out"]).abs().max().item() / r.scale["out"] > 1e3 * R.bound_single(r.spread["out"])


@pytest.mark.parametrize("c,b", R.REWARD_CASES)
def test_reward_cases(c, b):
    (logits, base, target), r = R.reward_case(c, b)
    t = R.REWARD_T
    assert logits.shape == base.shape == (b * t, c) and target.shape == (b,) and target.dtype == torch.int64
    assert int(target.min()) >= 0 and int(target.max()) < c
    conf = r.ref["conf"]
    rows = logits.reshape(b, t, c)
    assert int(target[0]) == c - 1 and (b < 2 or int(target[1]) == 0)                         # targets at both ends of the row
    assert bool((rows[0, 0] == rows[0, 0, 0]).all()) and abs(conf[0, 0].item() - 1.0 / c) < 1e-12       # a uniform row
    assert conf[1, 0].item() > 1 - 1e-12                                                       # a saturated one
    if b >= 3:
        assert bool((conf[:, 1] > 1 - 1e-12).all()) and bool(((conf[:, 2] - 1.0 / c).abs() < 1e-12).all())
    if c == 1:
        # one class: every confidence is exactly 1 and the cross-entropy exactly 0 in any precision -- no spread, the bound is the floor
        assert bool((conf == 1).all()) and r.ref["ce"].item() == 0 and all(s == 0 for s in r.spread.values())
        assert r.ref["r_random"].abs().max().item() == 0 and bool((r.ref["r_prev"][1:] == 0).all())
        return
    _visible(r, ("conf", "ce", "r_conf") + (("r_prev", "r_random") if b > 1 else ()))
    assert r.ref["r_prev"].abs().max().item() > 1e-3 and r.ref["r_random"].abs().max().item() > 1e-3
    assert (r.ref["r_prev"].sum(0) - conf[-1]).abs().max().item() < 1e-12                      # the increments telescope


def test_reward_table():
    assert len(R.REWARD_CASES) == 28
    assert {b for _, b in R.REWARD_CASES} == {1, 255, 256, 257} and {c for c, _ in R.REWARD_CASES} == {1, 27, 63, 64, 65, 239, 1000}


@pytest.mark.parametrize("a,rows", R.ARGMAX_CASES)
def test_argmax_cases(a, rows):
    x, table = R.argmax_inputs(a, rows)
    want = R.argmax_first(x)
    assert x.shape == (rows, a) and table.shape == (a, 2) and want.shape == (rows,) and want.dtype == np.int64
    assert len({tuple(r) for r in table.tolist()}) == a
    top = x.max(1, keepdim=True)[0]
    ties = (x == top).sum(1)
    if a > 1:
        assert bool((ties > 1).any())                                                          # rows whose maximum is not unique
        assert bool((want != (a - 1 - np.argmax(x.numpy()[:, ::-1], axis=1)))[ties.numpy() > 1].all())     # ... where last-maximum differs
    if rows > 1:
        assert bool((ties == a).any()) and bool(torch.isposinf(x).any()) and bool(torch.isneginf(x).any())
        assert bool(torch.isneginf(x).all(1).any())                                            # a row of -inf only: index 0
        assert want[torch.isneginf(x).all(1).numpy()].max() == 0
        if a > 1:
            assert len(set(want.tolist())) > 2


def test_argmax_first_is_first():
    x = torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [float("-inf"), float("inf"), float("inf")]])
    assert R.argmax_first(x).tolist() == [1, 0, 1]
