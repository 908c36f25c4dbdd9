"""torch-CPU restatement of the Bottleneck ResNet with BatchNorm on BATCH statistics (train mode), and of the stage-0 training step of the
ActivityNet tree (ACT/main_dist.py:544-548) built on it: what tests/test_stage0_gpu.py holds the HIP walk to, in float64, and what
tests/test_stage0_host.py holds the G21 fixture to.  Functional over a state dict (tests/test_trunk_backward_gpu._cpu_trunk with
F.batch_norm(training=True) in place of the folded affine): nothing here touches the product code."""
import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def shift(x, t, div):
    """TemporalShift.shift on (NT, C, H, W) clips of t frames."""
    nt, c, hh, ww = x.shape
    v = x.view(nt // t, t, c, hh, ww)
    fold = c // div
    out = torch.zeros_like(v)
    out[:, :-1, :fold] = v[:, 1:, :fold]
    out[:, 1:, fold:2 * fold] = v[:, :-1, fold:2 * fold]
    out[:, :, 2 * fold:] = v[:, :, 2 * fold:]
    return out.view(nt, c, hh, ww)


def is_trunk_param(k):
    return k.endswith((".weight", ".bias")) and not k.startswith("fc.")


def trunk(p, x, layers, tsm=0, div=8, place="blockres", training=True, pre=None, masks=None):
    """(N, 3, S, S) -> (N, 2048).  p: name -> tensor with the torchvision keys; training: BatchNorm on the statistics of the batch, the
    running statistics of p updated in place (momentum 0.1, unbiased variance) and num_batches_tracked += 1; else on the running
    statistics.  pre: a dict that receives every ReLU's input by name ("stem", "<block>.z1", ".z2", ".y"); masks: name -> bool map that
    replaces the ReLU's own branch."""
    def cbn(conv, bn, z, stride=1, pad=0):
        z = F.conv2d(z, p[conv + ".weight"], stride=stride, padding=pad)
        if training and bn + ".num_batches_tracked" in p:
            p[bn + ".num_batches_tracked"] += 1
        return F.batch_norm(z, p[bn + ".running_mean"], p[bn + ".running_var"], p[bn + ".weight"], p[bn + ".bias"], training, BN_MOMENTUM, BN_EPS)

    def act(name, z):
        if pre is not None:
            pre[name] = z.detach()
        return F.relu(z) if masks is None else z * masks[name].to(z.dtype)

    n_round = 2 if layers[2] >= 23 else 1
    y = F.max_pool2d(act("stem", cbn("conv1", "bn1", x, 2, 3)), 3, 2, 1)
    for li, (nblk, stride) in enumerate(zip(layers, (1, 2, 2, 2)), start=1):
        for b in range(nblk):
            q = "layer%d.%d" % (li, b)
            s = stride if b == 0 else 1
            if tsm and place == "block":
                y = shift(y, tsm, div)
            z = shift(y, tsm, div) if tsm and place != "block" and b % n_round == 0 else y
            z = act(q + ".z1", cbn(q + ".conv1", q + ".bn1", z))
            z = act(q + ".z2", cbn(q + ".conv2", q + ".bn2", z, s, 1))
            z = cbn(q + ".conv3", q + ".bn3", z)
            idn = cbn(q + ".downsample.0", q + ".downsample.1", y, s) if b == 0 else y
            y = act(q + ".y", z + idn)
    return y.mean((2, 3))


def cast(sd, dtype, grad=True):
    """A working copy of a state dict in `dtype`: parameters as leaves that require grad, buffers as clones."""
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            out[k] = v.clone()
        elif grad and k.endswith((".weight", ".bias")):
            out[k] = v.to(dtype).clone().requires_grad_(True)
        else:
            out[k] = v.to(dtype).clone()
    return out


def project(g, rnd):
    """G17's two projections of a weight gradient: (G v, u^T G) with v of seed 174 and u of seed 184 (rnd: the fixtures' generator)."""
    g = g.flatten(1)
    v = torch.as_tensor(rnd((g.shape[1],), 174)).to(g.dtype)
    u = torch.as_tensor(rnd((g.shape[0],), 184)).to(g.dtype)
    return g @ v, u @ g


def stage0_step(sd, images, target, layers, lr, momentum, weight_decay, dtype):
    """One stage-0 step on the CPU in `dtype`: sd the ResNet's state dict (fc included), images (B, T*3, H, W), target (B,).
    -> dict: logits (B*T, C), pred (B, C), loss, {name: grad} of every parameter, the state dict after the step (running statistics
    moved, parameters stepped by SGD), the eval-mode per-frame logits after the step."""
    p = cast(sd, dtype)
    b, tc, hh, ww = images.shape
    t = tc // 3
    x = images.to(dtype).view(b * t, 3, hh, ww)
    logits = F.linear(trunk(p, x, layers, training=True), p["fc.weight"], p["fc.bias"])
    pred = logits.view(b, t, -1).mean(1, keepdim=True).squeeze(1)
    loss = F.cross_entropy(pred, target)
    names = [k for k, v in p.items() if v.requires_grad]
    grads = dict(zip(names, torch.autograd.grad(loss, [p[k] for k in names])))
    opt = torch.optim.SGD([p[k] for k in names], lr=lr, momentum=momentum, weight_decay=weight_decay)
    for k in names:
        p[k].grad = grads[k].clone()
    opt.step()
    with torch.no_grad():
        after = F.linear(trunk(p, x, layers, training=False), p["fc.weight"], p["fc.bias"])
    return dict(logits=logits.detach(), pred=pred.detach(), loss=loss.detach(), grads=grads, state={k: v.detach() for k, v in p.items()},
                logits_after=after)
