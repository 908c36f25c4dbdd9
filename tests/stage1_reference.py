"""torch-CPU restatement of the stage-1 training step of the ActivityNet tree (ACT/main_dist.py:473-493 over ACT/models/gfv_net.py:135-150):
the frozen glancer (oracle.ref_model), one crop per frame at given origins, the local CNN in train mode (tests/stage0_reference.trunk),
[global, local], the GRU classifier with dropout multipliers (tests/heads_reference.gru_cls), the cross-entropy of every step against the
clip's label, SGD over the focuser's and the classifier's parameters.  What tests/test_stage1_host.py holds the G22 fixtures to; nothing
here touches the product code."""
import torch
import torch.nn.functional as F

from oracle import ref_model as O
from tests import heads_reference as H
from tests import stage0_reference as R0

LOCAL, CLS = "focuser.net.", "classifier."


def stage1_step(sd, images, target, origins, patch, glance, layers, lr, momentum, weight_decay, dtype, mask=None, with_glancer=True):
    """One stage-1 step on the CPU in `dtype`.  sd: the GFV's state dict, images (B, T*3, H, W), target (B,), origins (B*T, 2) integer
    (y, x), mask (B, T, hidden) dropout multipliers or None.  -> dict: logits (B*T, C), last (B, C), loss, {name: grad} of the local CNN's
    and the classifier's parameters (full names; focuser.net.fc.* has none), the local CNN's state after the step, the eval-mode
    stage-1-form logits after the SGD step on the same crops."""
    b, tc, hh, ww = images.shape
    t = tc // 3
    images = images.to(dtype)
    frames = images.view(b * t, 3, hh, ww)
    frozen = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.startswith("glancer.")}
    with torch.no_grad():
        fvec = O.glancer_act(frozen, "glancer.net.", O.glancer_input(images, glance).reshape(b * t, 3, glance, glance))[1]
        patches = torch.stack([frames[i, :, int(y):int(y) + patch, int(x):int(x) + patch] for i, (y, x) in enumerate(origins)])
    local = R0.cast({k[len(LOCAL):]: v for k, v in sd.items() if k.startswith(LOCAL)}, dtype)
    cls = [sd[CLS + k].to(dtype).clone().requires_grad_(True) for k in H.CLS_KEYS]

    def forward(training, m):
        feat = R0.trunk(local, patches, layers, training=training)
        feature = (torch.cat([fvec, feat], 1) if with_glancer else feat).view(b, t, -1)
        return H.gru_cls(feature, cls, m, dtype)

    logits = forward(True, mask)
    loss = F.cross_entropy(logits, target.repeat_interleave(t))
    names = [k for k, v in local.items() if v.requires_grad and not k.startswith("fc.")]
    leaves = [local[k] for k in names] + cls
    grads = dict(zip([LOCAL + k for k in names] + [CLS + k for k in H.CLS_KEYS], torch.autograd.grad(loss, leaves)))
    opt = torch.optim.SGD(leaves, lr=lr, momentum=momentum, weight_decay=weight_decay)
    for leaf, g in zip(leaves, grads.values()):
        leaf.grad = g.clone()
    opt.step()
    with torch.no_grad():
        after = forward(False, None)
    return dict(logits=logits.detach(), last=logits.detach().view(b, t, -1)[:, -1], loss=loss.detach().reshape(1), grads=grads,
                state={LOCAL + k: v.detach() for k, v in local.items()}, logits_after=after)


def fixture_rows(g, r, rnd):
    """Every stored quantity of a G22 archive `g` against the step `r` (logits, last, loss, logits_after, grads and state by full name, as
    stage1_step returns them): [(error relative to the quantity's largest entry, the stored fp32-vs-fp64 spread, tag)].  Gradients are
    compared as they are stored: in full, or as G17's two projections (rnd: the fixtures' generator)."""
    import numpy as np

    def row(tag, got, ref, spread):
        ref = np.asarray(ref, dtype=np.float64)
        got = got.detach().double().cpu().numpy().reshape(ref.shape)
        return np.abs(got - ref).max() / np.abs(ref).max(), float(spread), tag

    grads = r["grads"]
    rows = [row(k, r[k], g[k], g["spread_" + k][0]) for k in ("logits", "last", "loss", "logits_after")]
    for tag, name in (("fc_weight", "fc.weight"), ("fc_bias", "fc.bias"), ("gru_bias_ih", "gru.bias_ih_l0"), ("gru_bias_hh", "gru.bias_hh_l0")):
        rows.append(row(tag, grads[CLS + name], g[tag], g["spread_" + tag][0]))
    for tag in ("ih", "hh"):
        gv, ug = R0.project(grads[CLS + "gru.weight_%s_l0" % tag].double().cpu(), rnd)
        rows.append(row("gru_w_%s_Gv" % tag, gv, g["gru_w_%s_Gv" % tag], g["spread_gru_w_%s_Gv" % tag][0]))
        rows.append(row("gru_w_%s_uG" % tag, ug, g["gru_w_%s_uG" % tag], g["spread_gru_w_%s_uG" % tag][0]))
    off = 0
    for i, n in enumerate(g["names_bn"].tolist()):
        grad = grads[n]
        assert grad is not None and torch.isfinite(grad).all(), n
        rows.append(row(n, grad, g["bn"][off:off + grad.numel()], g["spread_bn"][i]))
        off += grad.numel()
    assert off == g["bn"].size
    off_v = off_u = 0
    for i, n in enumerate(g["names_conv"].tolist()):
        grad = grads[n]
        assert grad is not None and torch.isfinite(grad).all(), n
        gv, ug = R0.project(grad.double().cpu(), rnd)
        rows.append(row(n + "@v", gv, g["conv_Gv"][off_v:off_v + gv.numel()], g["spread_conv_Gv"][i]))
        rows.append(row("u@" + n, ug, g["conv_uG"][off_u:off_u + ug.numel()], g["spread_conv_uG"][i]))
        off_v, off_u = off_v + gv.numel(), off_u + ug.numel()
    assert off_v == g["conv_Gv"].size and off_u == g["conv_uG"].size
    off = 0
    for i, n in enumerate(g["names_stat"].tolist()):
        v = r["state"][n]
        rows.append(row(n, v, g["stat"][off:off + v.numel()], g["spread_stat"][i]))
        off += v.numel()
    assert off == g["stat"].size
    return rows
