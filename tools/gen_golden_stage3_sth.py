#!/usr/bin/env python3
"""Stage-3 fixture of the Something-Something tree: one training step of the REAL reference model (STH/models/gfv_net.py, STH/models/tsn.py)
that fine-tunes the local CNN as STH/stage3.py does, imported exactly like tools/gen_golden.py does (its shims; no reference source is
copied).  Writes tests/golden/g20_sth_stage3.npz (case p0, the names and the optimizer groups) and tests/golden/g20_sth_stage3_mask.npz
(case mask): two cases of 53 k BatchNorm gradients and 66 k projection entries are 950 KB of incompressible fp32, more than the largest
golden of the repository, so each case has its archive.  Runs on the CPU.

Configuration: gen_golden.sth_args() (B = 2, Tg = Tf = 8, P = 128, 'blockres' shift, 174 classes); weights of seed SEED_W by
gen_golden.load_synth, clips from synth.synth_frames (seeds 3 and 4): neither is stored.  The action is FORCED (stored), so the policy is
not part of the comparison.  One BatchNorm gamma of layer2.0 (bn2, channel 3) is set to exactly 0.  The model is in the mode of
STH/stage3.py:313-317 (train(), then glancer, focuser and both policies eval()); fc is stripped as STH/stage3.py:87 does.

Two cases:
  p0     dropout 0
  mask   dropout 0.5 with a FIXED mask: observed on the reference's own nn.Dropout call under torch.manual_seed(SEED_M) (the multipliers
         0 or 2, stored), and replayed as a product in the float64 run

Per case, the float64 run's results stored as float32 (a test compares against the fp64 result): logits, loss, classifier.bias' gradient
in full, classifier.weight's gradient (1.4 MB in full: more than a committed file may hold) and every conv weight gradient as the two fixed random projections  G v  (v of seed 174, length =
columns of G.flatten(1))  and  u^T G  (u of seed 184, length = rows), every BatchNorm weight / bias gradient in full, and the logits of a
second forward (eval mode) after one SGD step (lr, momentum, weight_decay recorded; group lr = lr * lr_mult, weight_decay * decay_mult).
Vectors of many parameters are concatenated in the order of `names_bn` / `names_conv` (the reference's state-dict names).
`spread_*`: the same step in float32, as a relative difference per quantity (per parameter for the concatenated ones).
`groups_pbn0_<i>` / `groups_pbn1_<i>`: the parameter names of group i of the reference's get_optim_policies() with partial BN off / on.

Usage:  python tools/gen_golden_stage3_sth.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_golden_depths import save_stable  # noqa: E402

from adafocus_amd import synth  # noqa: E402

SEED_W, SEED_M = 2020, 203
LR, MOMENTUM, WEIGHT_DECAY = 0.001, 0.9, 5e-4
FORCED = [[0.13, 0.92], [0.77, 0.31]]
TARGET = [5, 100]
ZERO_GAMMA = ("focuser.net.base_model.5.0.bn2.weight", 3)
PREFIX = "focuser.net."


def import_reference(md):
    GG._enter_tree(GG.STH)
    import models.resnet as R
    md.resnet50 = lambda pretrained=False, **k: R.resnet50(pretrained=False, **k)
    md.ResNet = R.ResNet
    import models.gfv_net as G
    _mb = G.mobilenet_v2
    G.mobilenet_v2 = lambda n_class, pretrained=True: _mb(n_class=n_class, pretrained=False)
    return G


def build(G, args, dtype):
    model = G.GFV(args)
    model.focuser.net.base_model = torch.nn.Sequential(*list(model.focuser.net.base_model.children())[:-1])
    GG.load_synth(model, SEED_W)
    pol_shapes = {k: tuple(v.shape) for k, v in model.focuser.policy.policy_old.state_dict().items()}
    pol_sd = synth.synth_state_dict({"policy." + k: s for k, s in pol_shapes.items()}, SEED_W)
    for pol in (model.focuser.policy.policy_old, model.focuser.policy.policy):
        pol.load_state_dict({k[len("policy."):]: torch.from_numpy(v) for k, v in pol_sd.items()})
    with torch.no_grad():
        dict(model.named_parameters())[ZERO_GAMMA[0]][ZERO_GAMMA[1]] = 0.0
    model = model.to(dtype)
    for pol in (model.focuser.policy.policy_old, model.focuser.policy.policy):
        pol.to(dtype)
        if hasattr(pol, "action_var"):
            pol.action_var = pol.action_var.to(dtype)
    forced = torch.tensor(FORCED, dtype=dtype)
    model.focuser.policy.select_action = lambda *a, **k: forced
    return model


def stage3_mode(model):
    model.train()                       # STH/stage3.py:313-317
    model.glancer.eval()
    model.focuser.eval()
    model.focuser.policy.policy.eval()
    model.focuser.policy.policy_old.eval()


class ObservedDropout(torch.nn.Dropout):
    """nn.Dropout that records the multipliers of its call: the same draw repeated on a tensor of ones from the saved generator state."""

    def forward(self, x):
        if not self.training:
            return super().forward(x)
        state = torch.get_rng_state()
        out = super().forward(x)
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        self.seen = torch.nn.functional.dropout(torch.ones_like(x), self.p, True)
        torch.set_rng_state(after)
        assert torch.equal(out, x * self.seen)
        return out


class FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype) if self.training else x


def group_names(model, policies):
    names = {id(p): n for n, p in model.named_parameters()}
    return [[names[id(p)] for p in g["params"]] for g in policies]


def step(G, args, dtype, case, mask):
    """One stage-3 step of the reference in `dtype`: ({quantity: float64 array}, the dropout mask, names)."""
    torch.set_default_dtype(dtype)
    try:
        model = build(G, args, dtype)
        if case == "p0":
            model.dropout = torch.nn.Dropout(0.0)
        elif mask is None:
            model.dropout = ObservedDropout(0.5)
        else:
            model.dropout = FixedMask(mask)
        stage3_mode(model)
        policies = model.focuser.net.get_optim_policies()
        groups = policies + [{"params": list(model.classifier.parameters())}]
        for g in groups:
            g["lr"] = LR * g.get("lr_mult", 1)
            g["weight_decay"] = WEIGHT_DECAY * g.get("decay_mult", 1)
        opt = torch.optim.SGD(groups, lr=0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
        gl = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=3)).to(dtype)
        fo = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=4)).view(2, 8, 3, 224, 224).to(dtype)
        target = torch.tensor(TARGET)
        opt.zero_grad()
        torch.manual_seed(SEED_M)
        with torch.no_grad():
            fm, glog = model.glance(gl)
        pred, _ = model.action_stage3(fo, fm, glog, 0, args, prev_local_patch=None)
        loss = torch.nn.functional.cross_entropy(pred, target)
        loss.backward()
        if isinstance(model.dropout, ObservedDropout):
            mask = model.dropout.seen.clone()
        params = dict(model.named_parameters())
        mods = dict(model.named_modules())
        names_bn = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.BatchNorm2d)]
        names_conv = [n for n in params if n.startswith(PREFIX) and isinstance(mods[n.rsplit(".", 1)[0]], torch.nn.Conv2d)]
        assert len(names_bn) + len(names_conv) == sum(1 for n in params if n.startswith(PREFIX))
        out = {"logits": pred.detach(), "loss": loss.detach().reshape(1), "cls_bias": params["classifier.bias"].grad}
        per = {"bn": [params[n].grad.reshape(-1) for n in names_bn], "conv_Gv": [], "conv_uG": []}

        def project(g):
            g = g.flatten(1)
            v = torch.from_numpy(GG.rnd((g.shape[1],), 174)).to(dtype)
            u = torch.from_numpy(GG.rnd((g.shape[0],), 184)).to(dtype)
            return g @ v, u @ g

        out["cls_w_Gv"], out["cls_w_uG"] = project(params["classifier.weight"].grad)
        for n in names_conv:
            gv, ug = project(params[n].grad)
            per["conv_Gv"].append(gv)
            per["conv_uG"].append(ug)
        for n, p in params.items():          # nothing outside the optimizer's groups is expected to move
            if not (n.startswith(PREFIX) or n.startswith("classifier.")):
                assert p.grad is None or not p.grad.any(), n
        opt.step()
        model.eval()
        with torch.no_grad():
            fm, glog = model.glance(gl)
            after, _ = model.action_stage3(fo, fm, glog, 0, args, prev_local_patch=None)
        out["logits_after"] = after
        out = {k: v.detach().double().numpy() for k, v in out.items()}
        per = {k: [t.detach().double().numpy() for t in v] for k, v in per.items()}
        return out, per, mask, names_bn, names_conv
    finally:
        torch.set_default_dtype(torch.float32)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    md = GG._install_shims()
    G = import_reference(md)
    args = GG.sth_args()
    arrays = {"seeds": np.array([SEED_W, SEED_M]), "forced_action": np.array(FORCED, dtype=np.float32), "target": np.array(TARGET),
              "sgd": np.array([LR, MOMENTUM, WEIGHT_DECAY]), "zero_gamma_channel": np.array([ZERO_GAMMA[1]]),
              "zero_gamma_name": np.array([ZERO_GAMMA[0]])}
    for pbn in (0, 1):
        model = build(G, GG.sth_args(partial_bn=bool(pbn)), torch.float32)
        policies = model.focuser.net.get_optim_policies()
        arrays["group_names"] = np.array([g["name"] for g in policies])
        arrays["group_mults"] = np.array([[g["lr_mult"], g["decay_mult"]] for g in policies])
        for i, names in enumerate(group_names(model, policies)):
            arrays["groups_pbn%d_%d" % (pbn, i)] = np.array(names, dtype=str)
            print("  partial_bn %d group %d (%s): %d parameters" % (pbn, i, policies[i]["name"], len(names)))
    shared, arrays = arrays, {}
    for case in ("p0", "mask"):
        r32, p32, mask, names_bn, names_conv = step(G, args, torch.float32, case, None)
        r64, p64, _, _, _ = step(G, args, torch.float64, case, mask)
        shared["names_bn"], shared["names_conv"] = np.array(names_bn), np.array(names_conv)
        if case == "mask":
            assert set(np.unique(mask.numpy())) == {0.0, 2.0}
            arrays["mask"] = (mask.numpy() != 0)
        for k in r64:
            arrays["%s_%s" % (case, k)] = r64[k].astype(np.float32)
            arrays["spread_%s_%s" % (case, k)] = np.array([rel(r32[k], r64[k])])
            print("  %-5s %-14s max %.3e  fp32-vs-fp64 %.2e" % (case, k, np.abs(r64[k]).max(), arrays["spread_%s_%s" % (case, k)][0]))
        for k in p64:
            arrays["%s_%s" % (case, k)] = np.concatenate(p64[k]).astype(np.float32)
            sp = np.array([rel(a, b) for a, b in zip(p32[k], p64[k])])
            arrays["spread_%s_%s" % (case, k)] = sp
            print("  %-5s %-14s %d parameters, fp32-vs-fp64 min %.2e median %.2e max %.2e" % (case, k, len(sp), sp.min(), np.median(sp), sp.max()))
            assert np.isfinite(sp).all() and (sp > 0).all(), (case, k)
    save_stable("g20_sth_stage3", **shared, **{k: v for k, v in arrays.items() if not k.startswith(("mask", "spread_mask"))})
    save_stable("g20_sth_stage3_mask", **{k: v for k, v in arrays.items() if k.startswith(("mask", "spread_mask"))})


if __name__ == "__main__":
    main()
