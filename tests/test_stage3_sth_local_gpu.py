"""Stage-3 training of the Something-Something model with the local CNN fine-tuned, on the MI355X, against the reference's own step
(G20: tests/golden/g20_sth_stage3.npz and g20_sth_stage3_mask.npz, tools/gen_golden_stage3_sth.py): logits, loss, every gradient or its
projections and the logits after one SGD step; the flag-off path; the refusal of the other arithmetics; run-to-run bit identity.

Tolerance: the error against the reference's fp64 result, relative to that quantity's largest entry, is at most 50x the fp32-vs-fp64
spread of the same quantity recorded in the golden (G17's rule, tests/test_stage3_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import synth
from adafocus_amd.train import train_stage3_batch_sth
from tests.helpers import golden, rnd
from tests.test_state_dict_compat import sth_args

pytestmark = pytest.mark.gpu

SPREAD_FACTOR = 50
DEV = torch.device("cuda:0")
_G = {}


def _golden(case):
    if not _G:
        _G["p0"] = golden("g20_sth_stage3")
        _G["mask"] = golden("g20_sth_stage3_mask")
    return _G["p0"], _G[case]


def _model(dropout=0.5, math=None):
    """GFV of sth_args() with the generator's weights (seed in the golden), fc stripped as STH/stage3.py:87, the golden's gamma = 0."""
    from adafocus_amd.gfv_net_sth import GFV
    g, _ = _golden("p0")
    a = sth_args()
    a.gpu, a.dropout = 0, dropout
    m = GFV(a)
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])
    seed = int(g["seeds"][0])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()}, strict=True)
    pol_shapes = {"policy." + k: tuple(v.shape) for k, v in m.focuser.policy.policy_old.state_dict().items()}
    pol = {k[len("policy."):]: torch.from_numpy(v) for k, v in synth.synth_state_dict(pol_shapes, seed).items()}
    for p in (m.focuser.policy.policy_old, m.focuser.policy.policy):
        p.load_state_dict(pol)
    with torch.no_grad():
        m.state_dict(keep_vars=True)[str(g["zero_gamma_name"][0])][int(g["zero_gamma_channel"][0])] = 0.0
    # the arithmetic is pinned: training is fp32 only, whatever default the session's other modules run the trunk with
    m.focuser.net.base_model.set_math(math or "f32")
    return m.to(DEV), a


def _clips():
    if "clips" not in _G:
        gl = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=3)).to(DEV)
        fo = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=4)).to(DEV)
        _G["clips"] = (gl, fo)
    return _G["clips"]


def _optimizer(m, g):
    lr, momentum, wd = (float(v) for v in g["sgd"])
    groups = m.focuser.net.get_optim_policies() + [{"params": list(m.classifier.parameters())}]      # STH/stage3.py:189-193
    opt = torch.optim.SGD(groups, lr=0, momentum=momentum, weight_decay=wd)
    for grp in opt.param_groups:
        grp["lr"] = lr * grp.get("lr_mult", 1)
        grp["weight_decay"] = wd * grp.get("decay_mult", 1)
    return opt


def _mask(case):
    if case == "p0":
        return None
    return torch.from_numpy(_golden("mask")[1]["mask"].astype(np.float32) * np.float32(2.0)).to(DEV)


def _forward(m, a, mask, forced):
    gl, fo = _clips()
    with torch.no_grad():
        fm, glog = m.glance(gl)
    pred, _ = m.action_stage3(fo.view(2, 8, 3, 224, 224), fm, glog, 0, a, prev_local_patch=None, forced_action=forced, dropout_mask=mask)
    return pred


def _check(tag, got, ref, spread):
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref).max() / np.abs(ref).max()
    return err, float(spread), tag


def _project(grad):
    gm = grad.double().flatten(1).cpu()
    return gm @ rnd((gm.shape[1],), 174).double(), rnd((gm.shape[0],), 184).double() @ gm


@pytest.mark.parametrize("case", ["p0", "mask"])
def test_step_matches_the_reference_g20(case):
    g0, g = _golden(case)
    m, a = _model(dropout=0.0 if case == "p0" else 0.5)
    m.stage3_train_mode()
    opt = _optimizer(m, g0)
    forced = torch.from_numpy(g0["forced_action"]).to(DEV)
    target = torch.from_numpy(g0["target"]).to(DEV)
    opt.zero_grad()
    pred = _forward(m, a, _mask(case), forced)
    loss = F.cross_entropy(pred, target)
    loss.backward()
    params = m.state_dict(keep_vars=True)
    for k, p in params.items():
        if not (k.startswith("focuser.net.") or k.startswith("classifier.")) and isinstance(p, torch.nn.Parameter):
            assert p.grad is None, k                                   # glancer and policy take no gradient
    rows = [_check("logits", pred.detach().cpu(), g[case + "_logits"], g["spread_%s_logits" % case][0]),
            _check("loss", loss.detach().cpu().reshape(1), g[case + "_loss"], g["spread_%s_loss" % case][0]),
            _check("classifier.bias", m.classifier.bias.grad.cpu(), g[case + "_cls_bias"], g["spread_%s_cls_bias" % case][0])]
    gv, ug = _project(m.classifier.weight.grad)
    rows += [_check("classifier.weight@v", gv, g[case + "_cls_w_Gv"], g["spread_%s_cls_w_Gv" % case][0]),
             _check("u@classifier.weight", ug, g[case + "_cls_w_uG"], g["spread_%s_cls_w_uG" % case][0])]
    off = 0
    for i, n in enumerate(g0["names_bn"].tolist()):
        grad = params[n].grad
        assert grad is not None and torch.isfinite(grad).all(), n
        rows.append(_check(n, grad.cpu(), g[case + "_bn"][off:off + grad.numel()], g["spread_%s_bn" % case][i]))
        off += grad.numel()
    assert off == g[case + "_bn"].size
    off_v = off_u = 0
    for i, n in enumerate(g0["names_conv"].tolist()):
        grad = params[n].grad
        assert grad is not None and torch.isfinite(grad).all(), n
        gv, ug = _project(grad)
        rows.append(_check(n + "@v", gv, g[case + "_conv_Gv"][off_v:off_v + gv.numel()], g["spread_%s_conv_Gv" % case][i]))
        rows.append(_check("u@" + n, ug, g[case + "_conv_uG"][off_u:off_u + ug.numel()], g["spread_%s_conv_uG" % case][i]))
        off_v, off_u = off_v + gv.numel(), off_u + ug.numel()
    assert off_v == g[case + "_conv_Gv"].size and off_u == g[case + "_conv_uG"].size
    zero_name, ch = str(g0["zero_gamma_name"][0]), int(g0["zero_gamma_channel"][0])
    assert params[zero_name].grad[ch].item() != 0.0
    # one SGD step, then the eval forward: the optimizer's groups, the step and the engine's re-pack of the new weights meet here
    opt.step()
    m.eval()
    with torch.no_grad():
        after = _forward(m, a, None, forced)
    assert (after - pred.detach()).abs().max().item() > 1e-2 * pred.detach().abs().max().item()       # the step moved the model
    rows.append(_check("logits_after", after.cpu(), g[case + "_logits_after"], g["spread_%s_logits_after" % case][0]))
    rows.sort(key=lambda r: -(r[0] / r[1]))
    print("%s: %d quantities; worst err / spread: %s" % (case, len(rows), ", ".join("%s %.2e / %.2e" % (r[2], r[0], r[1]) for r in rows[:5])))
    bad = [r for r in rows if not r[0] <= SPREAD_FACTOR * r[1]]
    assert not bad, bad[:8]


def test_flag_off_is_the_classifier_only_path_with_the_same_logits():
    """stage3_train_mode(train_local=False): the engine's features, the same logits bit for bit, and no gradient in the backbone."""
    g0, _ = _golden("mask")
    forced = torch.from_numpy(g0["forced_action"]).to(DEV)
    m, a = _model()
    mask = _mask("mask")
    m.stage3_train_mode()
    on = _forward(m, a, mask, forced).detach().clone()
    m.stage3_train_mode(train_local=False)
    m.zero_grad(set_to_none=True)
    off = _forward(m, a, mask, forced)
    assert torch.equal(off.detach(), on)
    F.cross_entropy(off, torch.from_numpy(g0["target"]).to(DEV)).backward()
    assert m.classifier.weight.grad is not None and m.classifier.bias.grad is not None
    for k, p in m.focuser.net.named_parameters():
        assert p.grad is None, k


def test_other_arithmetics_refuse_to_train():
    g0, _ = _golden("p0")
    forced = torch.from_numpy(g0["forced_action"]).to(DEV)
    m, a = _model(math="f16")
    m.stage3_train_mode()
    with pytest.raises(NotImplementedError, match="f16"):
        _forward(m, a, None, forced)
    a.video_div = 2
    m.focuser.net.base_model.set_math("f32")
    with pytest.raises(NotImplementedError, match="video_div"):
        _forward(m, a, None, forced)


def test_train_stage3_batch_twice_gives_the_same_bits():
    """train_stage3_batch_sth (zero_grad, glance, action_stage3, cross-entropy, backward, SGD step) from the same state and mask."""
    g0, _ = _golden("mask")
    gl, fo = _clips()
    target = torch.from_numpy(g0["target"]).to(DEV)
    runs = []
    for _ in range(2):
        m, a = _model()
        m.stage3_train_mode()
        pred, loss = train_stage3_batch_sth(m, gl, fo, target, a, _optimizer(m, g0), dropout_mask=_mask("mask"))
        runs.append((pred, loss, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert torch.isfinite(runs[0][0]).all() and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k, v in runs[0][2].items():
        assert torch.equal(v, runs[1][2][k]), k
