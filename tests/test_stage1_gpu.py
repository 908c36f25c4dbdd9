"""Stage-1 training on the MI355X: ``train.train_stage1_batch`` against the reference's own step (G22:
tests/golden/g22_act_stage1_*.npz, tools/gen_golden_stage1.py), the step as the composition of its tested parts, the frozen glancer,
reproducibility and the surface of ``GFV.stage1_train_mode()``.

Tolerance of the fixture comparison: G17's rule as tests/test_stage0_gpu.py states it -- the error against the float64 result, relative to
that quantity's largest entry, is at most SPREAD_FACTOR (50) x the stored distance between the reference's own fp32 and fp64 runs.
Everything else is exact (torch.equal)."""
import numpy as np
import pytest
import torch

from adafocus_amd import hip_ops, synth, trunk_train
from adafocus_amd.gfv_net import GFV
from adafocus_amd.train import train_stage1_batch
from adafocus_amd.utils import get_patch_nhwc4
from tests import stage1_reference as R
from tests import test_stage1_host as H
from tests.helpers import golden, rnd
from tests.test_trunk_backward_gpu import SPREAD_FACTOR

pytestmark = pytest.mark.gpu

CASES = H.CASES
FORM = dict(backbone_pred=False, one_step=False)
_STEPS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _model(g, dev, **over):
    m = GFV(H.args_of(g, **over))
    m.load_state_dict(H.state_dict_of(g, m), strict=True)
    m.focuser.net.set_math("f32")
    return m.to(dev)


def _inputs(g, dev, size=None):
    """images (B, T*3, S, S), target (B,), the gather's actions of the stored origins (B*T, 2), the dropout multipliers or None."""
    b, t, s, p = (int(v) for v in g["dims"][:4])
    images = torch.from_numpy(synth.synth_frames(b, t, size or s, seed=int(g["seeds"][1]))).to(dev)
    actions = torch.from_numpy(((g["origins"].astype(np.float64) + 0.5) / (s - p)).astype(np.float32)).to(dev)
    mask = torch.from_numpy(g["mask"]).to(dev) if "mask" in g.files else None
    return images, torch.from_numpy(g["target"]).to(dev), actions, mask


def _optimizer(m, g):
    lr, momentum, wd = (float(v) for v in g["sgd"])
    return torch.optim.SGD([{"params": m.focuser.parameters()}, {"params": m.classifier.parameters()}], lr=lr, momentum=momentum, weight_decay=wd)


def _step(case, dev, fresh=False):
    """One train_stage1_batch on a model of the fixture's weights, crops and mask: (model, pred, loss, the glancer's state before)."""
    if fresh or case not in _STEPS:
        g = golden(case)
        images, target, actions, mask = _inputs(g, dev)
        m = _model(g, dev)
        m.stage1_train_mode()
        before = {k: v.detach().clone() for k, v in m.glancer.state_dict().items()}
        pred, loss = train_stage1_batch(m, images, target, H.args_of(g), _optimizer(m, g), crop_actions=actions, dropout_mask=mask)
        out = (m, pred, loss, before)
        if fresh:
            return out
        _STEPS[case] = out
    return _STEPS[case]


@pytest.mark.parametrize("case", CASES)
def test_train_stage1_batch_matches_the_reference_g22(dev, case):
    g = golden(case)
    b, t, s, p, glance, c, hidden = (int(v) for v in g["dims"])
    images, target, actions, mask = _inputs(g, dev)
    twin = _model(g, dev)
    twin.stage1_train_mode()
    with torch.no_grad():
        logits, _ = twin(input=images, scan=twin.glancer_input(images), training=True, crop_actions=actions, dropout_mask=mask, **FORM)
    assert logits.shape == (b * t, c)
    m, pred, loss, _ = _step(case, dev)
    assert not pred.requires_grad and not loss.requires_grad and pred.shape == (b, c)
    net = m.focuser.net
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    assert net.fc.weight.grad is None and net.fc.bias.grad is None
    # the eval forward after the step on the same crops: the new weights AND the moved running statistics reach the engine (_sync re-folds)
    m.eval()
    np.random.seed(int(g["seeds"][2]))
    with torch.no_grad():
        after, _ = m(input=images, scan=m.glancer_input(images), training=False, **FORM)
    m.stage1_train_mode()
    r = dict(logits=logits, last=pred, loss=loss.reshape(1), logits_after=after, grads={k: q.grad for k, q in m.named_parameters()},
             state=m.state_dict())
    rows = R.fixture_rows(g, r, rnd)
    rows.sort(key=lambda row: -(row[0] / row[1]))
    print("G22 %s: %d quantities; worst err / spread: %s" % (case, len(rows), ", ".join("%s %.2e / %.2e" % (row[2], row[0], row[1]) for row in rows[:5])))
    bad = [row for row in rows if not row[0] <= SPREAD_FACTOR * row[1]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", CASES)
def test_step_is_the_composition_of_its_parts(dev, case):
    g = golden(case)
    b, t, s, p = (int(v) for v in g["dims"][:4])
    images, target, actions, mask = _inputs(g, dev)
    m = _step(case, dev)[0]
    twin = _model(g, dev)
    twin.stage1_train_mode()
    frames = images.view(b * t, 3, s, s)
    with torch.no_grad():
        scan = twin.glancer_input(images)
        fvec = twin.glancer(scan.reshape(b * t, 3, scan.shape[2], scan.shape[3]))[1]
        patches = get_patch_nhwc4(frames, actions, p)
    local = trunk_train.trunk_features(twin.focuser.net, patches)
    feature = torch.cat([fvec, local], 1).view(b, t, -1)
    gru, fc = twin.classifier.gru, twin.classifier.fc
    logits = hip_ops.GruClassifierFn.apply(feature, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, fc.weight, fc.bias, mask)
    _, dlogits = hip_ops.ce_steps(logits.detach(), target, t)
    logits.backward(dlogits)
    want = dict(twin.named_parameters())
    for k, q in m.named_parameters():
        if want[k].grad is None:
            assert q.grad is None, k
        else:
            assert q.grad is not None and torch.equal(q.grad, want[k].grad), k
    assert sum(1 for q in want.values() if q.grad is not None) == 2 * 53 + 53 + 6
    stats = twin.state_dict()
    for k, v in m.state_dict().items():
        if "running_" in k or k.endswith("num_batches_tracked"):
            assert torch.equal(v, stats[k]), k


@pytest.mark.parametrize("case", CASES)
def test_glancer_is_untouched(dev, case):
    m, _, _, before = _step(case, dev)
    for k, q in m.glancer.named_parameters():
        assert q.grad is None, k
    for k, v in m.glancer.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_two_steps_from_the_same_state_give_the_same_bits(dev):
    case = CASES[1]
    m, pred, loss, _ = _step(case, dev)
    m2, pred2, loss2, _ = _step(case, dev, fresh=True)
    assert torch.equal(pred, pred2) and torch.equal(loss, loss2)
    other = dict(m2.named_parameters())
    for k, q in m.named_parameters():
        assert torch.equal(q, other[k]), k
        assert (q.grad is None and other[k].grad is None) or torch.equal(q.grad, other[k].grad), k
    buffers = dict(m2.named_buffers())
    for k, v in m.named_buffers():
        assert torch.equal(v, buffers[k]), k


def test_surface(dev):
    g = golden(CASES[0])
    images, target, actions, _ = _inputs(g, dev)
    m = _model(g, dev)
    H.test_stage1_train_mode_table(m)            # the module-state table, a plain .train() and eval mode with training=True still raise
    H.test_stage1_train_mode_refusals()
    # eval mode after stage1_train_mode() + .eval() is the existing stage-1 eval form, bit for bit
    plain = _model(g, dev).eval()
    m.stage1_train_mode()
    m.eval()
    outs = []
    for model in (plain, m):
        np.random.seed(11)
        with torch.no_grad():
            outs.append(model(input=images, scan=model.glancer_input(images), training=False, **FORM))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_without_glancer_features(dev):
    g = golden(CASES[0])
    b, t, s, p, glance, c, hidden = (int(v) for v in g["dims"])
    images, target, actions, _ = _inputs(g, dev)
    m = GFV(H.args_of(g, with_glancer=False)).to(dev)
    assert m.classifier.gru.weight_ih_l0.shape[1] == 2048
    m.stage1_train_mode()
    pred, loss = train_stage1_batch(m, images, target, H.args_of(g), _optimizer(m, g), crop_actions=actions)
    assert pred.shape == (b, c) and torch.isfinite(pred).all() and torch.isfinite(loss)
    assert m.classifier.gru.weight_ih_l0.grad is not None and m.focuser.net.conv1.weight.grad is not None


def test_frames_of_the_patch_size_take_no_draw(dev):
    g = golden(CASES[0])
    b, t, s, p, glance, c, hidden = (int(v) for v in g["dims"])
    images, target, _, _ = _inputs(g, dev, size=p)
    m = _model(g, dev, input_size=p)
    m.stage1_train_mode()
    np.random.seed(12)
    state = np.random.get_state()
    logits, last = m(input=images, scan=m.glancer_input(images), training=True, **FORM)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    assert logits.shape == (b * t, c) and logits.requires_grad and torch.isfinite(logits).all()
