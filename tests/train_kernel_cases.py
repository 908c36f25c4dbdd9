"""The training kernels' outputs as bits (G21): one case per launch form of the split-K weight gradient (csrc/splitk_wgrad.h), of the
slice sum, the column sums and the strided GEMM (csrc/train_common.hip), with seeded CPU inputs copied to the device.  digests() runs
them and returns {case: {output: sha256 of its bytes}}; tools/train_kernel_digest.py prints that, tests/test_train_kernel_bits_gpu.py
holds the library to the recording of the build before the kernels were merged (tests/golden/g21_train_kernel_bits.json)."""
import hashlib

import torch
import torch.nn.functional as F

from adafocus_amd import _lib as L
from adafocus_amd import hip_ops
from tests.helpers import rnd
from tests.test_conv_backward_gpu import CASES as CONV_CASES
from tests.test_conv_backward_gpu import _case as conv_case


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv_operands(tag, dev):
    x, w, g, _, s, p = conv_case(tag)
    xd = _nhwc(x)
    if xd.shape[-1] % 4:
        xd = F.pad(xd, (0, 4 - xd.shape[-1]))                  # the stem's zero lane
    return xd.to(dev), _nhwc(g).to(dev), hip_ops.pack_conv_weight(w.to(dev)), w, s, p


def _conv_wgrad(tag):
    def run(dev):
        xd, gd, w_ohwi, _, s, p = _conv_operands(tag, dev)
        return {"dw": hip_ops.conv2d_wgrad(xd, gd, tuple(w_ohwi.shape), s, p)}
    return run


def _conv_bn_param_grad(tag):
    def run(dev):
        xd, gd, w_ohwi, w, s, p = _conv_operands(tag, dev)
        cout = w.shape[0]
        scale, mean = rnd((cout,), 3100).to(dev), rnd((cout,), 3101, 0.3).to(dev)
        var = (rnd((cout,), 3102).abs() + 0.5).to(dev)
        dw_raw = hip_ops.conv2d_wgrad(xd, gd, tuple(w_ohwi.shape), s, p)
        dw, dgamma, dbeta = hip_ops.conv_bn_param_grad(gd, dw_raw, w_ohwi, scale, mean, var, 1e-5, w.shape[1])
        return {"dw": dw, "dgamma": dgamma, "dbeta": dbeta}
    return run


def _wenc(npix, cin, cmid, gated, split_k, seed):
    def run(dev):
        states, de1 = rnd((npix, cin), seed).to(dev), rnd((npix, cmid), seed + 1).to(dev)
        e1 = rnd((npix, cmid), seed + 2).to(dev) if gated else None
        return {"dw": hip_ops.ppo_wenc_grad(states, de1, e1, split_k=split_k)}
    return run


def _encoder_backward(c, tg, hw, h, b, t, with_bn, seed):
    """The shapes of tests/test_stage2_sth_gpu.py::test_update_matches_float64_autograd: 64 conv outputs, C = c * tg channels."""
    def run(dev):
        cin, cmid, rows, px = c * tg, 64, t * b, hw * hw
        mid = px * cmid
        states = rnd((rows, hw, hw, cin), seed, 0.5).to(dev)
        e1, e_bt = rnd((rows, mid), seed + 1).to(dev), rnd((rows, h), seed + 2).to(dev)
        dx_bt, w_lin = rnd((b, t, h), seed + 3).to(dev), rnd((h, mid), seed + 4, mid ** -0.5).to(dev)
        bn = None
        if with_bn:
            c1, l1 = rnd((rows * px, cmid), seed + 5).to(dev), rnd((rows, h), seed + 6).to(dev)
            stats = [rnd((n,), seed + 7 + i, 0.3).to(dev) for i, n in enumerate((cmid, cmid, h, h))]         # gamma1, mean1, gamma2, mean2
            inv = [(rnd((n,), seed + 11 + i).abs() + 0.5).to(dev) for i, n in enumerate((cmid, h))]
            bn = (c1, stats[0], stats[1], inv[0], l1, stats[2], stats[3], inv[1])
        out = hip_ops.ppo_encoder_backward(states, e1, e_bt, dx_bt, t, b, w_lin, bn)
        names = ("dw_enc", "dw_lin", "db_lin", "dgamma1", "dbeta1", "dgamma2", "dbeta2")
        return dict(zip(names, out))
    return run


def _gru_backward(b, t, f, h, c, seed):
    def run(dev):
        x = rnd((b, t, f), seed, 0.5).to(dev)
        w_ih, w_hh = rnd((3 * h, f), seed + 1, f ** -0.5).to(dev), rnd((3 * h, h), seed + 2, h ** -0.5).to(dev)
        b_ih, b_hh = rnd((3 * h,), seed + 3, 0.1).to(dev), rnd((3 * h,), seed + 4, 0.1).to(dev)
        fc_w, fc_b = rnd((c, h), seed + 5, h ** -0.5).to(dev), rnd((c,), seed + 6, 0.1).to(dev)
        mask = ((rnd((b, t, h), seed + 7) >= 0).float() * 2.0).to(dev)
        logits, gi, hs = hip_ops.gru_cls_train_forward(x, w_ih, w_hh, b_ih, b_hh, fc_w, fc_b, mask)
        dlogits = rnd(tuple(logits.shape), seed + 8, 1e-3).to(dev)
        out = hip_ops.gru_cls_backward(x, w_ih, w_hh, b_hh, fc_w, gi, hs, mask, dlogits)
        return dict(zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh", "dw_fc", "db_fc"), out))
    return run


# name -> (runner, follows the device's CU count).  The PPO split-K launch plans its slices for min(device CUs, 256); the convolution's
# plans for 256 whatever the device, the strided GEMM and the column sums do not look at the device.
CASES = {}
for _tag in [c[0] for c in CONV_CASES]:
    CASES["conv2d_wgrad/" + _tag] = (_conv_wgrad(_tag), False)
for _tag in ("3x3_s1_9", "1x1_s1"):
    CASES["conv_bn_param_grad/" + _tag] = (_conv_bn_param_grad(_tag), False)
for _npix, _cin in ((7, 128), (1001, 384), (735, 1280)):               # <1,1> one partial group; <1,1> odd tail; <2,1>
    CASES["ppo_wenc_grad/32_gated_%dx%d" % (_npix, _cin)] = (_wenc(_npix, _cin, 32, True, True, 4000 + _npix), True)
for _npix, _cin in ((18, 128), (147, 384)):                            # <1,2>
    for _gated in (True, False):
        CASES["ppo_wenc_grad/64_%s_%dx%d" % ("gated" if _gated else "dense", _npix, _cin)] = (_wenc(_npix, _cin, 64, _gated, True, 4100 + _npix), True)
CASES["ppo_wenc_grad/chain_1001x384"] = (_wenc(1001, 384, 32, True, False, 4200), False)
CASES["ppo_encoder_backward/bn"] = (_encoder_backward(128, 3, 3, 64, 5, 1, True, 4300), True)
CASES["ppo_encoder_backward/plain"] = (_encoder_backward(128, 3, 3, 64, 5, 1, False, 4400), True)
CASES["gru_cls_backward/6x5x256"] = (_gru_backward(6, 5, 3328, 256, 200, 4500), False)


def device_cus(dev):
    return int(L.load_library().adaf_device_cus(L.handle(dev)))


ONE_CORE_SHAPES = ((128, 64), (384, 32))      # (cin, cout): the same tiles, slices and product order in both callers' plans on 256 CUs


def one_core_pair(cin, cout, dev):
    """A 1x1 stride-1 weight gradient over 1001 pixels through both callers of the split-K core: (conv2d_wgrad as (cout, cin),
    ppo_wenc_grad without a gate)."""
    x, g = rnd((1, 7, 143, cin), 4600 + cin).to(dev), rnd((1, 7, 143, cout), 4601 + cin).to(dev)
    conv = hip_ops.conv2d_wgrad(x, g, (cout, 1, 1, cin), 1, 0).reshape(cout, cin)
    return conv, hip_ops.ppo_wenc_grad(x.view(1001, cin), g.view(1001, cout), None)


def digest(name, dev):
    """{output: sha256 of the output's bytes} of one case."""
    res = CASES[name][0](dev)
    torch.cuda.synchronize()
    return {k: hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).hexdigest() for k, v in res.items()}


def digests(dev):
    """{case: {output: sha256 of the output's bytes}} over CASES."""
    return {name: digest(name, dev) for name in CASES}
