"""Every operand a wrapper takes BY VALUE may be a non-contiguous view: hip_ops makes the dense copy, and the copy lives until the launch
(hip_ops._call's operand rule).  The failure this module is for: a wrapper that takes the pointer of `t.contiguous()` and lets the
temporary die hands the next operand's temporary the same block of the caching allocator, so the kernel reads one operand twice -- silently.

Each case runs a wrapper twice on the same seeded data and requires torch.equal on every output:
  dense  every operand cloned to a contiguous tensor bound to a name;
  views  every by-value operand replaced by torch.stack([t, NaN], -1)[..., 0] (is_contiguous() False, NaN in the gaps).
Operands that a wrapper reads through a stride (the GRU's x, out= views: tests/test_strided_operands_gpu.py) or updates in place
(running_mean, running_var) stay dense in both calls.  The shapes are the smallest the entry points take, so that the temporaries share
the allocator's smallest bucket, where the reuse is certain.
"""
import pytest
import torch

from tests.helpers import rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


def _view(t):
    v = torch.stack([t, torch.full_like(t, float("nan"))], -1)[..., 0]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def _dense_equals_views(fn, by_value, **dense_only):
    """fn(**operands) -> tensor or tuple of tensors (None allowed), called with dense operands and with views of `by_value`."""
    dense = {k: None if v is None else v.clone().contiguous() for k, v in by_value.items()}
    want = fn(**dense, **dense_only)
    views = {k: None if v is None else _view(v) for k, v in dense.items()}
    got = fn(**views, **dense_only)
    want, got = (o if isinstance(o, tuple) else (o,) for o in (want, got))
    assert len(want) == len(got)
    for i, (w, g) in enumerate(zip(want, got)):
        if w is None:
            assert g is None, i
            continue
        assert torch.isfinite(w.float()).all(), i
        assert torch.equal(w, g), (i, float((w.float() - g.float()).abs().max()))


def _gru_params(dev, feat, hid, classes, seed):
    shapes = dict(w_ih=(3 * hid, feat), w_hh=(3 * hid, hid), b_ih=(3 * hid,), b_hh=(3 * hid,), fc_w=(classes, hid), fc_b=(classes,))
    return {k: rnd(s, seed + i, 0.3).to(dev) for i, (k, s) in enumerate(shapes.items())}


def test_fold_bn(dev, ops):
    c = 16
    _dense_equals_views(ops.fold_bn, dict(gamma=rnd((c,), 1).to(dev), beta=rnd((c,), 2).to(dev), mean=rnd((c,), 3).to(dev),
                                          var=rnd((c,), 4).abs().to(dev) + 0.5))


def test_gru_cls_forward(dev, ops):
    b, t, feat, hid, classes = 2, 3, 8, 8, 4
    x = rnd((b, t, feat), 10).to(dev)
    _dense_equals_views(lambda **p: ops.gru_cls_forward(x, **p), _gru_params(dev, feat, hid, classes, 11))


def test_gru_seq_forward(dev, ops):
    b, t, feat, hid = 2, 3, 8, 8
    x = rnd((b, t, feat), 20).to(dev)
    p = _gru_params(dev, feat, hid, 4, 21)
    for h0 in (None, rnd((b, hid), 27).to(dev)):
        _dense_equals_views(lambda **q: ops.gru_seq_forward(x, **q), dict(w_ih=p["w_ih"], w_hh=p["w_hh"], b_ih=p["b_ih"], b_hh=p["b_hh"], h0=h0))


@pytest.mark.parametrize("masked", [False, True])
def test_gru_cls_training_pair(dev, ops, masked):
    """hidden = 16, not 8: the two training entry points take hidden sizes that are multiples of 16 only."""
    b, t, feat, hid, classes = 2, 3, 8, 16, 4
    x = rnd((b, t, feat), 30).to(dev)
    p = _gru_params(dev, feat, hid, classes, 31)
    mask = ((rnd((b, t, hid), 37) > 0).float() * 2.0).to(dev) if masked else None
    _dense_equals_views(lambda **q: ops.gru_cls_train_forward(x, **q), dict(p, mask=mask))
    _, gi, hs = ops.gru_cls_train_forward(x, mask=mask, **p)
    _dense_equals_views(lambda **q: ops.gru_cls_backward(x, **q),
                        dict(w_ih=p["w_ih"], w_hh=p["w_hh"], b_hh=p["b_hh"], fc_w=p["fc_w"], gi=gi, hs=hs, mask=mask,
                             dlogits=rnd((b * t, classes), 38).to(dev)))


def test_bn_train_pair(dev, ops):
    rows, cols = 4, 8
    x = rnd((rows, cols), 40).to(dev)
    gamma, beta = rnd((cols,), 41).to(dev) + 1.5, rnd((cols,), 42).to(dev)
    running = rnd((cols,), 43).to(dev), rnd((cols,), 44).abs().to(dev) + 0.5

    def forward(gamma, beta):
        rm, rv = running[0].clone(), running[1].clone()           # updated in place: dense, and part of the result
        return ops.bn_train_forward(x, gamma, beta, rm, rv) + (rm, rv)
    _dense_equals_views(forward, dict(gamma=gamma, beta=beta))
    y, mean, invstd = ops.bn_train_forward(x, gamma, beta)
    for relu_out in (y, None):
        _dense_equals_views(ops.bn_train_backward, dict(x=x, y=relu_out, dy=rnd((rows, cols), 45).to(dev), gamma=gamma, mean=mean, invstd=invstd))


def test_fc_meanpool_forward(dev, ops):
    b, t, f, c = 2, 2, 8, 4
    _dense_equals_views(lambda **q: ops.fc_meanpool_forward(q.pop("feat"), b, **q),
                        dict(feat=rnd((b * t, f), 50).to(dev), fc_w=rnd((c, f), 51).to(dev), fc_b=rnd((c,), 52).to(dev),
                             global_logit=rnd((b, t, c), 53).to(dev)))


def test_se_gate(dev, ops):
    n, c, sq = 2, 16, 4
    _dense_equals_views(ops.se_gate, dict(pool_mean=rnd((n, c), 60, 0.5).to(dev), w_reduce=rnd((sq, c, 1, 1), 61, 0.2).to(dev),
                                          b_reduce=rnd((sq,), 62, 0.1).to(dev), w_expand=rnd((c, sq, 1, 1), 63, 0.3).to(dev),
                                          b_expand=rnd((c,), 64, 0.1).to(dev)))


def test_depthwise_3x3(dev, ops):
    """(n, h, w, c, stride) = (2, 16, 16, 32, 1) and, for fp16 storage, (4, 1, 1, 32, 1): the smallest cases of test_depthwise_conv_vs_torch
    and test_dwconv_f16_and_casts."""
    c = 32
    w = ops.pack_dw_weight(rnd((c, 1, 3, 3), 70, 0.3).to(dev))
    scale, bias = rnd((c,), 71, 0.2).to(dev) + 1.0, rnd((c,), 72, 0.1).to(dev)
    _dense_equals_views(ops.dwconv3x3_bn_act, dict(x=rnd((2, 16, 16, c), 73).to(dev), w_33c=w, scale=scale, bias=bias))
    _dense_equals_views(ops.dwconv3x3_bn_act_f16, dict(x=rnd((4, 1, 1, c), 74).half().to(dev), w_33c=w, scale=scale, bias=bias))


def test_dwconv_same(dev, ops):
    """(k, stride, size, c) = (5, 1, 10, 8) with n = 3: the smallest map x channels of test_dwconv_same_vs_torch, fp32 and fp16 storage."""
    n, k, size, c = 3, 5, 10, 8
    w = ops.pack_dw_weight_kxk(rnd((c, 1, k, k), 80, 0.3).to(dev))
    operands = dict(x=rnd((n, size, size, c), 81).to(dev), w_kkc=w, scale=rnd((c,), 82, 0.2).to(dev) + 1.0, bias=rnd((c,), 83, 0.1).to(dev))
    for want_pool in (True, False):
        _dense_equals_views(lambda **q: ops.dwconv_same_bn_act(k=k, want_pool=want_pool, **q), operands)
    _dense_equals_views(lambda **q: ops.dwconv_same_bn_act(k=k, want_pool=True, **q), dict(operands, x=operands["x"].half()))


@pytest.mark.parametrize("hw,cin,cout,res", [(7, 8, 100, False), (10, 24, 24, True)])
def test_conv1x1_gated_bn(dev, ops, hw, cin, cout, res):
    """The two smallest cases of test_conv1x1_gated_bn_vs_torch (n = 3, a 1 x hw map), one of them with the identity skip."""
    n = 3
    operands = dict(x=rnd((n, 1, hw, cin), 90 + cin).to(dev), gate=torch.sigmoid(rnd((n, cin), 91)).to(dev),
                    w=rnd((cout, cin), 92, (1.0 / cin) ** 0.5).to(dev), scale=rnd((cout,), 93, 0.2).to(dev) + 1.0,
                    bias=rnd((cout,), 94, 0.1).to(dev), residual=rnd((n, 1, hw, cout), 95).to(dev) if res else None)
    _dense_equals_views(ops.conv1x1_gated_bn, operands)
    _dense_equals_views(ops.conv1x1_gated_bn, dict(operands, gate=None))
    half = {k: v.half() if k in ("x", "w", "residual") and v is not None else v for k, v in operands.items()}
    _dense_equals_views(ops.conv1x1_gated_bn, half)
