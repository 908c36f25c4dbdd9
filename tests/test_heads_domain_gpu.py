"""The classifier and reward heads at every dataset's class count (27 Jester, 101, 174, 200, 239 FCVID, 1000+) and at the batch, step
and width boundaries of their kernels, each against the float64 statement of the same operation in tests/heads_reference.py and under
its one tolerance rule (8 x / 50 x the fp32-vs-fp64 spread of the reference itself; moves and arg-max exact).  The golden end-to-end
tests run 200 and 174 classes only: a wrong column ownership or tail predicate at another count gives plausible logits for the wrong
class.  Every case prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from adafocus_amd import _lib, hip_ops
from adafocus_amd.gfv_net import RecurrentClassifier
from tests import heads_reference as R
from tests import strided as S
from tests.helpers import rnd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LATENCY_TILE = 95


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _check(tag, got, r, name, bound):
    err = R.rel_err(got, r, name)
    print("%s %s: err %.3e  bound %.3e  spread %.3e  scale %.3e" % (tag, name, err, bound, r.spread[name], r.scale[name]))
    assert bool(torch.isfinite(got).all()), (tag, name)
    assert err <= bound, (tag, name, err, bound)


# ---- linear: the engine and the small-batch form ---------------------------------------------------------------------------------------------
def _latency_takes(fin):
    """The small-batch form's documented limit for a plain fp32 linear (include/adafocus.h, tile 95): in % 64 == 0."""
    return fin % 64 == 0


@pytest.mark.parametrize("c,fin,rows", R.LINEAR_CASES)
def test_linear_engine_and_latency_form(c, fin, rows):
    (x, w, b), r = R.linear_case(c, fin, rows)
    xd, wd, bd = _dev(x, w, b)
    tag = "linear C=%d in=%d rows=%d" % (c, fin, rows)
    bound = R.bound_single(r.spread["y"])
    engine = hip_ops.linear(xd, wd, bd)
    assert engine.shape == (rows, c)
    _check(tag + " engine", engine, r, "y", bound)
    forms = [("engine", 0)]
    if _latency_takes(fin):
        lat = hip_ops.linear(xd, wd, bd, tile=LATENCY_TILE)
        _check(tag + " latency", lat, r, "y", bound)
        assert torch.equal(lat, engine), "%s: the small-batch form differs from the engine in %d elements" % (tag, int((lat != engine).sum()))
        forms.append(("latency", LATENCY_TILE))
    else:
        with pytest.raises(_lib.AdafError):
            hip_ops.linear(xd, wd, bd, tile=LATENCY_TILE)
    # guard columns: the same product into a view whose row stride is larger than C, inside a canary allocation
    ld = c + 7
    for name, tile in forms:
        buf, view = S.guarded((rows, 1, 1), c, ld, S.lead_for(ld), ld + 8, torch.float32, DEV)
        S.conv_call("engine", xd.view(rows, 1, 1, fin), wd.view(c, 1, 1, fin), None, bd, None, view, tile=tile)
        S.assert_guards_intact(buf, view, "%s %s ldo=%d" % (tag, name, ld))
        assert torch.equal(S.payload(view).view(rows, c), engine), (tag, name, "strided store differs from the dense one")


# ---- the GRU scan with and without the classifier ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.GRU_CASES, ids=R.gru_case_id)
def test_gru_forward_every_mode(k):
    (x, h0, params), r = R.gru_case(k)
    xd, h0d = _dev(x, h0)
    pd = _dev(*params)
    tag = "gru " + R.gru_case_id(k)
    b_logits, b_hs = R.bound_recurrence(r.spread["logits"]), R.bound_recurrence(r.spread["hs_h0"])
    assert hip_ops.gru_scan_timeouts() == 0
    out = {}
    try:
        for mode in (1, 2, 0):
            hip_ops.set_gru_persistent(mode, DEV)
            logits, last = hip_ops.gru_cls_forward(xd, *pd)
            hs = hip_ops.gru_seq_forward(xd, *pd[:4], h0=h0d)
            out[mode] = (logits, last, hs)
    finally:
        hip_ops.set_gru_persistent(1, DEV)
    assert hip_ops.gru_scan_timeouts() == 0
    for mode, (logits, last, hs) in out.items():
        assert logits.shape == (k.b * k.t, k.c) and last.shape == (k.b, k.c) and hs.shape == (k.b, k.t, k.h)
        _check("%s mode %d" % (tag, mode), logits, r, "logits", b_logits)
        _check("%s mode %d" % (tag, mode), hs, r, "hs_h0", b_hs)
        assert torch.equal(last, logits.view(k.b, k.t, k.c)[:, -1]), (tag, mode, "`last` is not the last step's rows")
    for i, name in enumerate(("logits", "last", "hs_h0")):
        assert torch.equal(out[1][i], out[2][i]), (tag, name, "plain and cooperative launch differ")


# ---- stage 3: RecurrentClassifier in train mode, fixed mask ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.STAGE3_CASES, ids=lambda k: "B%d-T%d-H%d-C%d" % k)
def test_stage3_forward_and_backward(k):
    (x, params, mask, dlogits), r = R.stage3_case(k)
    tag = "stage3 B%d-T%d-H%d-C%d" % k
    cls = RecurrentClassifier(seq_len=k.t, input_dim=R.STAGE3_F, batch_size=k.b, hidden_dim=k.h, num_classes=k.c, dropout=0.5)
    cls.load_state_dict(dict(zip(R.CLS_KEYS, params)))
    cls = cls.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    maskd, dld = _dev(mask, dlogits)
    assert hip_ops.gru_scan_timeouts() == 0
    logits, last = cls(xd, mask=maskd)
    logits.backward(dld)
    got = {"logits": logits.detach(), "dx": xd.grad}
    got.update({n: p.grad for n, p in cls.named_parameters()})
    assert set(got) == set(R.STAGE3_OUTPUTS)
    assert torch.equal(last.detach(), logits.detach().view(k.b, k.t, k.c)[:, -1])
    fails = []
    for name in R.STAGE3_OUTPUTS:
        try:
            _check(tag, got[name], r, name, R.bound_recurrence(r.spread[name]))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
    # the persistent and the launch-per-step backward on the same saved activations: the same bits
    pd = [p.detach() for p in (cls.gru.weight_ih_l0, cls.gru.weight_hh_l0, cls.gru.bias_ih_l0, cls.gru.bias_hh_l0, cls.fc.weight, cls.fc.bias)]
    xs = xd.detach()
    logits2, gi, hs = hip_ops.gru_cls_train_forward(xs, *pd, mask=maskd)
    assert torch.equal(logits2, got["logits"])
    runs = {}
    try:
        for mode in (1, 0):
            hip_ops.set_gru_persistent(mode, DEV)
            runs[mode] = hip_ops.gru_cls_backward(xs, pd[0], pd[1], pd[3], pd[4], gi, hs, maskd, dld)
    finally:
        hip_ops.set_gru_persistent(1, DEV)
    assert hip_ops.gru_scan_timeouts() == 0
    names = ("dx", "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "fc.weight", "fc.bias")
    for name, u, v in zip(names, runs[1], runs[0]):
        assert torch.equal(u, v), (tag, name, "persistent and launch-per-step backward differ")
        assert torch.equal(u, got[name]), (tag, name, "the autograd function's gradient differs from the direct call")


# ---- FC + segment mean ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,t,tg,glob", R.MEANPOOL_CASES)
def test_fc_meanpool(c, t, tg, glob):
    (feat, w, b, glog), r = R.meanpool_case(c, t, tg, glob)
    out = hip_ops.fc_meanpool_forward(*_dev(feat), R.MEANPOOL_B, *_dev(w, b, glog))
    assert out.shape == (R.MEANPOOL_B, c)
    _check("meanpool C=%d T=%d Tg=%d global=%d" % (c, t, tg, glob), out, r, "out", R.bound_single(r.spread["out"]))


# ---- rewards, confidences, the last step's cross-entropy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.REWARD_KINDS)
@pytest.mark.parametrize("c,b", R.REWARD_CASES)
def test_rewards(c, b, kind):
    (logits, base, target), r = R.reward_case(c, b)
    ld, bd, td = _dev(logits, base, target)
    t = R.REWARD_T
    tag = "rewards C=%d B=%d %s" % (c, b, kind)
    rewards, conf, ce = hip_ops.ppo_rewards(ld, bd if kind == "random" else None, td, t, kind, want_conf=True, want_ce_last=True)
    assert rewards.shape == (t, b) and conf.shape == (t, b) and ce.shape == (1,)
    fails = []
    for got, name in ((rewards, "r_" + kind), (conf, "conf"), (ce, "ce")):
        try:
            _check(tag, got, r, name, R.bound_single(r.spread[name]))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
    # the outputs that were not asked for change nothing, and the structural identities of tests/test_stage2_rollout_gpu.py
    assert torch.equal(hip_ops.ppo_rewards(ld, bd if kind == "random" else None, td, t, kind), rewards)
    if kind == "prev":
        assert torch.equal(rewards[0], conf[0]) and torch.equal(rewards[1:], conf[1:] - conf[:-1])
    elif kind == "conf":
        assert torch.equal(rewards, conf)
    else:
        assert torch.equal(rewards, conf - hip_ops.ppo_rewards(bd, None, td, t, "conf"))


# ---- exact: arg-max / table lookup, row transpose ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,rows", R.ARGMAX_CASES)
def test_argmax_rows_and_grid_actions(a, rows):
    x, table = R.argmax_inputs(a, rows)
    want = R.argmax_first(x)
    xd, td = _dev(x, table)
    idx = hip_ops.argmax_rows(xd)
    assert idx.dtype == torch.int64 and idx.shape == (rows,)
    assert np.array_equal(idx.cpu().numpy(), want)
    idx2, act = hip_ops.grid_actions(xd, td)
    assert np.array_equal(idx2.cpu().numpy(), want)
    assert act.shape == (rows, 2) and torch.equal(act.cpu(), table[torch.from_numpy(want)])


@pytest.mark.parametrize("ni,nj,width", R.TRANSPOSE_CASES)
def test_rows_transpose(ni, nj, width):
    x = rnd((ni * nj, width), 9000 + width)
    out = hip_ops.rows_transpose(x.to(DEV), ni, nj)
    assert out.shape == x.shape
    assert torch.equal(out.cpu(), x.view(ni, nj, width).permute(1, 0, 2).reshape(nj * ni, width))
    assert torch.equal(hip_ops.rows_transpose(out, nj, ni).cpu(), x)
