#!/usr/bin/env python3
"""Randomised shapes through the conv engine (automatic tile choice and a few forced tiles) against the naive on-device
kernel of the same contract.  Maps are square or not (h and w drawn independently); about a third of the cases hand x, out and the
residual over as row-strided views (ldx / ldo / ldr > channels, out / residual possibly 4-byte but not 16-byte aligned).  Every operand
lives in a NaN-canary allocation with a guard band around it (tools/guard_bands.py): a write outside the output's payload or a read of a
gap is a MISMATCH.  usage: conv_fuzz.py [cases=150] [seed=0]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import guard_bands as S  # noqa: E402  (tools/guard_bands.py, next to this script)

dev = torch.device("cuda:0")
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
worst = 0.0
for i in range(cases):
    k = int(rng.choice([1, 1, 1, 3, 3, 5, 7]))
    stride = int(rng.choice([1, 1, 2])) if k > 1 or rng.random() < 0.3 else 1
    cin = int(rng.choice([4, 8, 16, 24, 32, 48, 64, 96, 128, 144, 160, 192, 256, 320, 384, 512]))
    cout = int(rng.choice([8, 16, 24, 32, 40, 64, 96, 128, 160, 200, 256, 320, 512, 1000]))
    if k >= 5:
        cin = min(cin, 32)
    hi = 29
    n = int(rng.integers(1, 40))
    if rng.random() < 0.25:
        n = int(rng.integers(200, 1200))
        hi = 9
    hh = int(rng.integers(max(k, 2), hi))
    ww = hh if rng.random() < 0.5 else int(rng.integers(max(k, 2), hi))      # square, or h and w on their own
    act = int(rng.choice([0, 1, 2, 3]))
    pad = k // 2 if rng.random() < 0.8 else 0
    oh, ow = (hh + 2 * pad - k) // stride + 1, (ww + 2 * pad - k) // stride + 1
    if oh <= 0 or ow <= 0:
        continue
    res = rng.random() < 0.4
    tsm = 0
    if k == 1 and stride == 1 and pad == 0 and cin % 32 == 0 and rng.random() < 0.3:
        tsm = int(rng.choice([2, 4, 8]))
        n = max(tsm, n - n % tsm)
    # strided, guarded operands: unrelated strides (ldx a multiple of 4, ldo / ldr any), out / residual 0..3 floats off 16-byte alignment
    ldx = ldo = ldr = oo = orr = 0
    if rng.random() < 0.35:
        ldx = cin + 4 * int(rng.integers(0, 8))
        ldo = cout + int(rng.integers(0, 24))
        ldr = cout + int(rng.integers(0, 24))
        oo, orr = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    x = torch.randn((n, hh, ww, cin), device=dev)
    w = torch.randn((cout, k, k, cin), device=dev) * float(1.0 / np.sqrt(k * k * cin))
    sc = torch.rand(cout, device=dev) + 0.5
    bi = torch.randn(cout, device=dev) * 0.1
    r = torch.randn((n, oh, ow, cout), device=dev) if res else None
    kw = dict(stride=stride, pad=pad, act=act, tsm_segments=tsm, tsm_div=8)

    def place(dense, ld, off):
        ld = ld or dense.shape[-1]
        buf, view = S.guarded(dense.shape[:-1], dense.shape[-1], ld, S.lead_for(ld, off), ld + 8, torch.float32, dev)
        return buf, S.fill(view, dense)

    def run(kind, tile):
        ld = ldo or cout
        ob, ov = S.guarded((n, oh, ow), cout, ld, S.lead_for(ld, oo), ld + 8, torch.float32, dev)
        S.conv_call(kind, xv, w, sc, bi, rv, ov, tile=tile, **kw)
        return S.payload(ov), S.find_guard_damage(ob, ov)

    xv = place(x, ldx, 0)[1]
    rv = place(r, ldr, orr)[1] if res else None
    desc = "n=%d h=%d w=%d cin=%d cout=%d k=%d s=%d pad=%d act=%d res=%s tsm=%d ldx=%d ldo=%d ldr=%d off=%d/%d" % (
        n, hh, ww, cin, cout, k, stride, pad, act, res, tsm, ldx, ldo, ldr, oo, orr)
    ref, hit = run("naive", 0)
    if hit is not None or not torch.isfinite(ref).all():
        print("MISMATCH case %d naive kernel: %s guard %r" % (i, desc, hit), flush=True)
    for tile in (0, 33, 38, 3, 41):
        got, hit = run("engine", tile)
        err = (got - ref).abs().max().item()
        scale = max(ref.abs().max().item(), 1.0)
        worst = max(worst, err / scale)
        if not torch.isfinite(got).all() or err / scale > 2e-4 or hit is not None:
            print("MISMATCH case %d tile %d: %s err=%.3e guard (offset, row, column, region)=%r" % (i, tile, desc, err, hit), flush=True)
print("%d cases x 5 tiles done; worst relative error %.2e" % (cases, worst))
