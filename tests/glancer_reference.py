"""torch-CPU restatement of MobileNetV2 in train mode (BatchNorm on BATCH statistics, ReLU6) over the ActivityNet key layout
(ACT/models/mobilenet.py), and of the stage-0 training step with pretrain_glancer=true built on it (ACT/main_dist.py:544-548): what
tests/test_glancer_train_gpu.py holds the HIP walk to, in float64 and fp32.  Functional over a state dict with the keys ``features.*`` /
``classifier.1.*``, modelled on tests/stage0_reference.py: nothing here touches the product code.

Every ReLU6 has TWO kinks.  ``pre`` receives each one's input under its neutral layer name ("stem", "b3.expand", "b3.dw", "head");
``masks`` replaces a ReLU6's own branches by given ones: name -> (passes, above), two bool maps -- the unit hands its input on, or it
is clipped to 6; neither: it is clipped to 0 -- so that a float64 run can follow the branches an fp32 device took."""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# (expand t, channels c, repeats n, stride s) -- mobilenet.py:88-97
SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def plan():
    """-> [(neutral name, conv key, bn key, depthwise?, stride, relu6?, block boundary)] in forward order; boundary: 'in' the layer
    reads the block's input, 'res' / 'out' it is the block's last layer with / without the identity joined."""
    out = [("stem", "features.0.0", "features.0.1", False, 2, True, None)]
    cin, i = 32, 0
    for t, c, n, s in SETTING:
        for r in range(n):
            i += 1
            stride, q, b, k = (s if r == 0 else 1), "features.%d.conv." % i, "b%d" % i, 0
            if t != 1:
                out.append((b + ".expand", q + "0.0", q + "0.1", False, 1, True, "in"))
                k = 1
            out.append((b + ".dw", q + "%d.0" % k, q + "%d.1" % k, True, stride, True, "in" if t == 1 else None))
            out.append((b + ".project", q + "%d" % (k + 1), q + "%d" % (k + 2), False, 1, False, "res" if stride == 1 and cin == c else "out"))
            cin = c
    out.append(("head", "features.18.0", "features.18.1", False, 1, True, None))
    return out


def relu6_names():
    return [name for name, _, _, _, _, r6, _ in plan() if r6]


def features(p, x, training=True, pre=None, masks=None):
    """(N, 3, S, S) -> (N, 1280).  p: name -> tensor; training: BatchNorm on the statistics of the batch, the running statistics of p
    updated in place (momentum 0.1, unbiased variance) and num_batches_tracked += 1; else on the running statistics."""
    y = x
    xin = None
    for name, conv, bn, dw, stride, r6, edge in plan():
        if edge == "in":
            xin = y
        w = p[conv + ".weight"]
        k = w.shape[-1]
        z = F.conv2d(y, w, None, stride, (k - 1) // 2, 1, w.shape[0] if dw else 1)
        if training and bn + ".num_batches_tracked" in p:
            p[bn + ".num_batches_tracked"] += 1
        z = F.batch_norm(z, p[bn + ".running_mean"], p[bn + ".running_var"], p[bn + ".weight"], p[bn + ".bias"], training, BN_MOMENTUM, BN_EPS)
        if edge == "res":
            z = z + xin
        if r6:
            if pre is not None:
                pre[name] = z.detach()
            if masks is None:
                z = F.hardtanh(z, 0.0, 6.0)
            else:
                passes, above = masks[name]
                z = z * passes.to(z.dtype) + 6.0 * above.to(z.dtype)
        y = z
    return y.mean((2, 3))


def cast(sd, dtype):
    """A working copy of a state dict in `dtype`: parameters as leaves that require grad, buffers as clones."""
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            out[k] = v.clone()
        elif k.endswith((".weight", ".bias")):
            out[k] = v.to(dtype).clone().requires_grad_(True)
        else:
            out[k] = v.to(dtype).clone()
    return out


ZERO_SHARE = 1e-6


def grad_scale(g64, name):
    """What a gradient's error is measured against: its largest float64 entry -- except for the bias of a project BatchNorm, whose gradient
    is exactly zero in exact arithmetic (everything that reads a block's output is a 1x1 convolution followed by a BatchNorm on batch
    statistics, which removes a per-channel constant; what any run computes is the residue of a sum that cancels).  Such a gradient,
    below ZERO_SHARE of the same BatchNorm's weight gradient (a sum of the same upstream gradient), takes that gradient's scale."""
    own = g64[name].abs().max().item()
    if name.endswith(".bias"):
        w = g64[name[:-len("bias")] + "weight"].abs().max().item()
        if own < ZERO_SHARE * w:
            return w
    return own


def is_feature_param(k):
    return k.startswith("features.") and k.endswith((".weight", ".bias"))


def walk(sd, x, dfeat, dtype, masks=None, pre=None):
    """Features, the gradient of <features, dfeat> for every parameter of ``features`` and the moved buffers, in `dtype`."""
    p = cast(sd, dtype)
    feat = features(p, x.to(dtype), True, pre, masks)
    names = [k for k in p if is_feature_param(k)]
    grads = dict(zip(names, torch.autograd.grad(feat, [p[k] for k in names], dfeat.to(dtype))))
    return feat.detach(), grads, {k: v.detach() for k, v in p.items() if k.startswith("features.") and not is_feature_param(k)}
