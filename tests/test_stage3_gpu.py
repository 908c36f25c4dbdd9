"""Stage-3 training of the ActivityNet GRU classifier on the MI355X: the HIP training forward + backward (csrc/gru_bptt.hip) against the
reference (G17), against CPU autograd at full size, bit-identity across forms and runs, and GFV end to end."""
import os
import types

import numpy as np
import pytest
import torch

from adafocus_amd import hip_ops, synth
from adafocus_amd.gfv_net import GFV, RecurrentClassifier
from tests.helpers import manifest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g17_act_stage3.npz")
DEV = torch.device("cuda:0")
PARAMS = ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "fc.weight", "fc.bias")


def _rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64([seed, 0xBEEF]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def _classifier(f, h, c, seed, p=0.5):
    cls = RecurrentClassifier(seq_len=4, input_dim=f, batch_size=2, hidden_dim=h, num_classes=c, dropout=p)
    shapes = {k: tuple(v.shape) for k, v in cls.state_dict().items()}
    cls.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()})
    return cls


def _mask(b, t, h, seed, p=0.5):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy((g.random((b, t, h)) >= p).astype(np.float32) / np.float32(1 - p))


def _hip_step(cls, x, mask, target):
    """One stage-3 step of `cls` (on the GPU, train mode) with the given mask: (logits, loss, {param: grad}, dx)."""
    cls.zero_grad(set_to_none=True)
    x = x.to(DEV).requires_grad_(True)
    logits, last = cls(x, mask=None if mask is None else mask.to(DEV))
    b, t = x.shape[:2]
    loss = torch.nn.functional.cross_entropy(logits, target.to(DEV).view(b, 1).expand(b, t).reshape(-1))
    loss.backward()
    return logits.detach().cpu(), loss.detach().cpu(), {n: p.grad.detach().cpu() for n, p in cls.named_parameters()}, x.grad.cpu()


def _cpu_step(cls, x, mask, target):
    """The same step with CPU nn.GRU + Linear autograd on the same weights."""
    gru = torch.nn.GRU(cls.input_dim, cls.hidden_dim, batch_first=True)
    fc = torch.nn.Linear(cls.hidden_dim, cls.num_classes)
    with torch.no_grad():
        for n, p in cls.named_parameters():
            mod, name = n.split(".")
            getattr(gru if mod == "gru" else fc, name).copy_(p.detach().cpu())
    x = x.clone().requires_grad_(True)
    out, _ = gru(x)
    if mask is not None:
        out = out * mask
    b, t = x.shape[:2]
    logits = fc(out.reshape(b * t, -1))
    loss = torch.nn.functional.cross_entropy(logits, target.view(b, 1).expand(b, t).reshape(-1))
    loss.backward()
    grads = {"gru." + n: p.grad for n, p in gru.named_parameters()}
    grads.update({"fc." + n: p.grad for n, p in fc.named_parameters()})
    return logits.detach(), loss.detach(), grads, x.grad


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_train_mode_matches_reference_g17():
    """G17: the reference's RecurrentClassifier step (p = 0 and a fixed p = 0.5 mask).  Tolerance: 50x the fp32-vs-fp64 spread of the
    same step recorded in the golden (at most 1.1e-6 of the largest entry), relative to the largest entry: the HIP GEMMs and the scan sum
    in other orders than ATen, which moves results by about as much as fp32 rounding does."""
    g = np.load(GOLDEN)
    b, t, f, h, c = (int(v) for v in g["dims"])
    x = torch.from_numpy(_golden_x(b, t, f))
    target = torch.from_numpy(g["target"])
    for tag, p, mask in (("p0", 0.0, None), ("mask", 0.5, torch.from_numpy(g["mask"]))):
        cls = _classifier(f, h, c, int(g["seeds"][0]), p=p).to(DEV).train()
        logits, loss, grads, dx = _hip_step(cls, x, mask, target)
        spread = max(float(g[k][0]) for k in g.files if k.startswith("spread_%s_" % tag))
        tol = 50 * spread
        got = {"logits": logits, "loss": loss.reshape(1), "x@v": dx.double() @ torch.from_numpy(_golden_v(f, 194)).double()}
        for n in ("gru.bias_ih_l0", "gru.bias_hh_l0", "fc.bias"):
            got[n] = grads[n]
        for i, n in enumerate(("gru.weight_ih_l0", "gru.weight_hh_l0", "fc.weight")):
            gm = grads[n].double()
            got[n + "@v"] = gm @ torch.from_numpy(_golden_v(gm.shape[1], 174 + i)).double()
            got["u@" + n] = torch.from_numpy(_golden_v(gm.shape[0], 184 + i)).double() @ gm
        for k, v in got.items():
            ref = g["%s_%s" % (tag, k)].astype(np.float64)
            err = np.abs(v.double().numpy().reshape(ref.shape) - ref).max() / np.abs(ref).max()
            assert err < tol, (tag, k, err, tol)


def _golden_x(b, t, f):
    return _rnd((b, t, f), 171, 0.5).numpy()


def _golden_v(n, seed):
    return _rnd((n,), seed).numpy()


@pytest.mark.parametrize("b,t,h,mask_on", [(64, 16, 1024, True), (64, 16, 1024, False), (1, 16, 1024, True), (33, 4, 1024, True),
                                           (65, 3, 1024, True), (5, 1, 1024, True), (6, 5, 256, True)])
def test_grads_match_cpu_autograd(b, t, h, mask_on):
    """All six parameter grads and dX against CPU autograd on the same weights, features and mask; each non-trivially large.  H = 256
    takes the launch-per-step form (the persistent scan is H = 1024 only)."""
    f, c = 3328, 200
    cls = _classifier(f, h, c, 9000 + h, p=0.5 if mask_on else 0.0)
    x = _rnd((b, t, f), 70 + b, 0.5)
    mask = _mask(b, t, h, 80 + b) if mask_on else None
    target = torch.from_numpy(np.random.Generator(np.random.PCG64(b)).integers(0, c, size=b))
    ref = _cpu_step(cls, x, mask, target)
    got = _hip_step(cls.to(DEV).train(), x, mask, target)
    assert _rel(got[0], ref[0]) < 2e-5
    assert abs(got[1].item() - ref[1].item()) < 1e-5 * abs(ref[1].item())
    for n in PARAMS:
        if t == 1 and n == "gru.weight_hh_l0":          # one step from h = 0: W_hh gets no gradient
            assert not ref[2][n].any() and not got[2][n].any()
            continue
        assert ref[2][n].abs().max() > 1e-6, n
        assert _rel(got[2][n], ref[2][n]) < 1e-4, (n, _rel(got[2][n], ref[2][n]))
    assert ref[3].abs().max() > 1e-6
    assert _rel(got[3], ref[3]) < 1e-4, _rel(got[3], ref[3])


def test_persistent_and_per_step_forms_give_the_same_bits():
    """One training forward, then its backward three times: persistent scan twice, launch-per-step form once -- identical bits, and the
    barrier's time-out counter stays 0."""
    b, t, f, h, c = 64, 16, 3328, 1024, 200
    cls = _classifier(f, h, c, 4242).to(DEV)
    w = [p.detach() for p in (cls.gru.weight_ih_l0, cls.gru.weight_hh_l0, cls.gru.bias_ih_l0, cls.gru.bias_hh_l0, cls.fc.weight, cls.fc.bias)]
    x = _rnd((b, t, f), 42, 0.5).to(DEV)
    mask = _mask(b, t, h, 43).to(DEV)
    logits, gi, hs = hip_ops.gru_cls_train_forward(x, *w, mask=mask)
    dlogits = _rnd(tuple(logits.shape), 44, 1e-3).to(DEV)
    before = hip_ops.gru_scan_timeouts()
    runs = [hip_ops.gru_cls_backward(x, w[0], w[1], w[3], w[4], gi, hs, mask, dlogits) for _ in range(2)]
    hip_ops.set_gru_persistent(0, DEV)
    try:
        runs.append(hip_ops.gru_cls_backward(x, w[0], w[1], w[3], w[4], gi, hs, mask, dlogits))
    finally:
        hip_ops.set_gru_persistent(1, DEV)
    assert hip_ops.gru_scan_timeouts() == before == 0
    for r in runs[1:]:
        for i, (u, v) in enumerate(zip(runs[0], r)):
            assert torch.equal(u, v), i
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in runs[0])


def test_dropout_mask_from_torch_generator_is_reproducible():
    cls = _classifier(3328, 1024, 200, 77).to(DEV).train()
    x = _rnd((4, 6, 3328), 7, 0.5).to(DEV)
    with torch.no_grad():
        torch.manual_seed(5)
        a = cls(x)[0]
        torch.manual_seed(5)
        b = cls(x)[0]
        c = cls(x)[0]
    assert torch.equal(a, b) and not torch.equal(a, c)


def _act_args(**over):
    a = dict(num_segments=4, num_classes=200, reward="random", dataset="actnet", input_size=224, batch_size=2, patch_size=96,
             with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024, policy_conv=True,
             gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.0, consensus="gru", hidden_dim=1024,
             train_stage=3)
    a.update(over)
    return types.SimpleNamespace(**a)


def test_gfv_stage3_end_to_end():
    args = _act_args()
    model = GFV(args)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(manifest()["ACT"], 1007).items()}
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    b, t = 2, 4
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=3)).to(DEV)
    target = torch.tensor([3, 150])
    model.eval()
    with torch.no_grad():
        eval_logits, eval_last = model(input=images, scan=images, training=False, backbone_pred=False, one_step=True)
        _, _, feature, _ = model.offline_forward(images, images)
    model.train()
    model.train_mode(args)
    assert model.classifier.training and not model.glancer.training and not model.focuser.training
    logits, last = model(input=images, scan=images, training=False, backbone_pred=False, one_step=True)
    assert (logits.detach() - eval_logits).abs().max().item() < 1e-5
    assert (last.detach() - eval_last).abs().max().item() < 1e-5
    loss = torch.nn.functional.cross_entropy(logits, target.to(DEV).view(b, 1).expand(b, t).reshape(-1))
    loss.backward()
    model.focuser.memory.clear_memory()
    for n, p in model.named_parameters():
        if not n.startswith("classifier."):
            assert p.grad is None, n
    ref = _cpu_step(model.classifier, feature.cpu(), None, target)
    for n in PARAMS:
        got = dict(model.classifier.named_parameters())[n].grad.cpu()
        assert _rel(got, ref[2][n]) < 1e-4, n

    # one SGD step under autocast + GradScaler (ACT/main_dist.py:521-527), mirrored on a CPU copy of the classifier
    cpu_cls = _classifier(3328, 1024, 200, 0, p=0.0)
    cpu_cls.load_state_dict({k: v.cpu() for k, v in model.classifier.state_dict().items()})
    opt = torch.optim.SGD(model.classifier.parameters(), lr=0.5, momentum=0.9)
    scaler = torch.amp.GradScaler("cuda")
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda"):
        logits, _ = model(input=images, scan=images, training=False, backbone_pred=False, one_step=True)
        assert logits.dtype == torch.float32
        loss = torch.nn.functional.cross_entropy(logits, target.to(DEV).view(b, 1).expand(b, t).reshape(-1))
    scaler.scale(loss).backward()
    scaler.step(opt)
    scaler.update()
    model.focuser.memory.clear_memory()
    _, _, cpu_grads, _ = _cpu_step(cpu_cls, feature.cpu(), None, target)
    cpu_opt = torch.optim.SGD(cpu_cls.parameters(), lr=0.5, momentum=0.9)
    for n, p in cpu_cls.named_parameters():
        p.grad = cpu_grads[n]
    cpu_opt.step()
    model.eval()
    with torch.no_grad():
        new_logits, _ = model(input=images, scan=images, training=False, backbone_pred=False, one_step=True)
    assert (new_logits - eval_logits).abs().max().item() > 1e-3          # the step moved the classifier
    ref_gru = torch.nn.GRU(3328, 1024, batch_first=True)
    ref_fc = torch.nn.Linear(1024, 200)
    with torch.no_grad():
        for n, p in cpu_cls.named_parameters():
            mod, name = n.split(".")
            getattr(ref_gru if mod == "gru" else ref_fc, name).copy_(p)
        ref_new = ref_fc(ref_gru(feature.cpu())[0].reshape(b * t, -1))
    assert _rel(new_logits.cpu(), ref_new) < 1e-4
