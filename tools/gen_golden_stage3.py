#!/usr/bin/env python3
"""Stage-3 fixture: one training step of the REAL reference RecurrentClassifier (ACT/models/gfv_net.py:409-435), imported exactly like
tools/gen_golden.py does (its shims; no reference source is copied).  Writes tests/golden/g17_act_stage3.npz.

Real dimensions (F = 3328, H = 1024, C = 200), B = 2, T = 8; weights of seed 1717 drawn by gen_golden.load_synth, features by seed 171
(scale 0.5), targets by seed 172; the loss is ACT/main_dist.py:530's cross-entropy over all B*T steps with the clip's target repeated.
Two cases:
  p0_*    dropout p = 0 (the module's nn.Dropout(0))
  mask_*  p = 0.5 with a FIXED mask: the instance's `dropout` module is swapped for one that multiplies by the recorded multipliers
          `mask` (0 or 2, seed 173)
Each case records logits, last_out, loss, the full gradients of bias_ih_l0, bias_hh_l0 and fc.bias, the feature gradient's projections,
and, for the weight gradients (40 MB at full size), fixed random projections  G v  (v of seed 174+i, length = columns)  and  u^T G  (u of
seed 184+i, length = rows)  instead of the matrices.

`spread_*` records the measured fp32-vs-fp64 difference of the same step (the reference module run in float64, relative to the largest
entry of each quantity): the tests' tolerances are a small multiple of it.  The .npz is written with fixed zip timestamps (two runs give
the same bytes).

Usage:  python tools/gen_golden_stage3.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_golden_depths import save_stable  # noqa: E402

SEED_W, SEED_X, SEED_Y, SEED_M = 1717, 171, 172, 173
B, T, F, H, C = 2, 8, 3328, 1024, 200
WEIGHTS = ("gru.weight_ih_l0", "gru.weight_hh_l0", "fc.weight")
BIASES = ("gru.bias_ih_l0", "gru.bias_hh_l0", "fc.bias")


def projections(name, i, shape):
    """(v, u) for weight gradient `name` (index i of WEIGHTS)."""
    v = GG.rnd((shape[1],), 174 + i)
    u = GG.rnd((shape[0],), 184 + i)
    return v, u


class FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype)


def step(G, p, mask, dtype):
    torch.set_default_dtype(dtype)             # (the reference's forward makes its zero state with torch.zeros)
    try:
        return _step(G, p, mask, dtype)
    finally:
        torch.set_default_dtype(torch.float32)


def _step(G, p, mask, dtype):
    cls = G.RecurrentClassifier(seq_len=T, input_dim=F, batch_size=B, hidden_dim=H, num_classes=C, dropout=p)
    GG.load_synth(cls, SEED_W)
    cls = cls.to(dtype)
    cls.train()
    if mask is not None:
        cls.dropout = FixedMask(torch.from_numpy(mask))
    x = torch.from_numpy(GG.rnd((B, T, F), SEED_X, 0.5)).to(dtype).requires_grad_(True)
    y = torch.from_numpy(np.random.Generator(np.random.PCG64(SEED_Y)).integers(0, C, size=B))
    logits, last = cls(x)
    loss = torch.nn.functional.cross_entropy(logits, y.view(B, -1).expand(B, T).reshape(-1))
    loss.backward()
    params = dict(cls.named_parameters())
    out = {"logits": logits.detach(), "last": last.detach(), "loss": loss.detach().reshape(1)}
    for n in BIASES:
        out[n] = params[n].grad
    for i, n in enumerate(WEIGHTS):
        g = params[n].grad
        v, u = projections(n, i, g.shape)
        out[n + "@v"] = g @ torch.from_numpy(v).to(dtype)
        out["u@" + n] = torch.from_numpy(u).to(dtype) @ g
    vx = torch.from_numpy(GG.rnd((F,), 194)).to(dtype)
    out["x@v"] = x.grad @ vx
    return {k: v.double().numpy() for k, v in out.items()}, y.numpy()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG._install_shims()
    GG._enter_tree(GG.ACT)
    import models.gfv_net as G
    mask = (np.random.Generator(np.random.PCG64(SEED_M)).random((B, T, H)) >= 0.5).astype(np.float32) * np.float32(2.0)
    arrays = {"seeds": np.array([SEED_W, SEED_X, SEED_Y, SEED_M]), "dims": np.array([B, T, F, H, C]), "mask": mask}
    for tag, p, m in (("p0", 0.0, None), ("mask", 0.5, mask)):
        r32, y = step(G, p, m, torch.float32)
        r64, _ = step(G, p, m, torch.float64)
        arrays["target"] = y
        for k in r32:
            arrays["%s_%s" % (tag, k)] = r32[k].astype(np.float32)
            spread = np.abs(r32[k] - r64[k]).max() / max(np.abs(r64[k]).max(), 1e-30)
            arrays["spread_%s_%s" % (tag, k)] = np.array([spread])
            print("  %-5s %-24s max %.3e  fp32-vs-fp64 %.2e" % (tag, k, np.abs(r64[k]).max(), spread))
    save_stable("g17_act_stage3", **arrays)


if __name__ == "__main__":
    main()
