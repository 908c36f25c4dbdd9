"""Training of the glancer's MobileNetV2 (stage 0 of the ActivityNet tree with pretrain_glancer=true: ACT/main_dist.py:534-548,
ACT/models/gfv_net.py:65-66, 90-91): one differentiable walk of the network over its NEUTRAL layer names -- ``stem``,
``b1`` .. ``b17`` with ``expand`` / ``dw`` / ``project``, and ``head``, the names of ``glancer_hip.neutral_params`` -- with a HIP backward.
``glancer_layers`` maps the ActivityNet key layout onto those names; the Something-Something layout can map onto the same walk.

THE WALK, in the batch-statistics form only (stage 0 has the whole model in train mode; a frozen-statistics form has no consumer):
  forward   per layer the RAW convolution -- the engine's ``conv2d_bn_act`` without affine and activation for the stem and the 1x1s,
            ``dwconv3x3_bn_act`` with unit scale and zero bias for the depthwise --, then ``bn_map_train_forward_act``: BatchNorm on the
            statistics of the map with ReLU6, or without activation and with the block's input as the residual for a ``project`` of a
            block with use_res_connect.  Running statistics move once, num_batches_tracked += 1.  Kept per layer: the layer's input, the
            raw map, mean, invstd and the output.  Then the mean over pixels.
  backward  the reverse walk: ``bn_map_train_backward_act`` with the ReLU6 mask (0 < y < 6 on the stored output) inside gives the gradient
            at the convolution's output, dgamma and dbeta; dW comes from ``conv2d_wgrad_rows`` (cout 16, 24 and 144 do not fill a block of
            32 filter rows) or ``dwconv3x3_wgrad``; the data gradient from ``conv2d_dgrad`` or ``dwconv3x3_dgrad``.  At a residual block
            the identity's gradient joins the main path's (``hip_ops.add``).  Launches for parameters that do not require grad are
            skipped; the data-gradient chain stops at the earliest layer with a trainable parameter; the stem takes no data gradient.

Math is fp32.  Orchestration in Python over ``hip_ops`` and one ``torch.autograd.Function``, as ``trunk_train.py``."""
import torch

from . import hip_ops
from .glancer_hip import _expand_ratios
from .trunk_train import _check_bn

__all__ = ["glancer_features", "GlancerFn", "glancer_layers", "walk_forward"]


class _Layer:
    """One conv + BatchNorm of the walk under its neutral name.  kind: 'conv' (the engine) or 'dw' (depthwise 3x3, pad 1); act: the
    activation behind the BatchNorm; res: the block's input joins in front of it (a project of a block with use_res_connect)."""

    def __init__(self, name, conv, bn, kind, stride, pad, act, res=False):
        self.name, self.conv, self.bn, self.kind, self.stride, self.pad, self.act, self.res = name, conv, bn, kind, stride, pad, act, res

    def params(self):
        return (self.conv.weight, self.bn.weight, self.bn.bias)


def glancer_layers(net, variant="act"):
    """-> (stem, [(layers of the block in forward order, use_res_connect)] for b1 .. b17, head) of a mobilenet.MobileNetV2 (the
    ActivityNet key layout: features.i.conv = [expand CBR,] depthwise CBR, project conv, project BN)."""
    if variant != "act":
        raise NotImplementedError("glancer_layers: the %r key layout is not mapped onto the walk (the ActivityNet layout is)" % (variant,))
    f, r6, none = net.features, hip_ops.ACT_RELU6, hip_ops.ACT_NONE
    stem = _Layer("stem", f[0][0], f[0][1], "conv", 2, 1, r6)
    blocks = []
    for i, t in enumerate(_expand_ratios(), start=1):
        seq, b, layers, k = f[i].conv, "b%d" % i, [], 0
        if t != 1:
            layers.append(_Layer(b + ".expand", seq[0][0], seq[0][1], "conv", 1, 0, r6))
            k = 1
        dw = seq[k][0]
        layers.append(_Layer(b + ".dw", dw, seq[k][1], "dw", dw.stride[0], 1, r6))
        layers.append(_Layer(b + ".project", seq[k + 1], seq[k + 2], "conv", 1, 0, none, res=f[i].use_res_connect))
        blocks.append((layers, f[i].use_res_connect))
    head = _Layer("head", f[18][0], f[18][1], "conv", 1, 0, r6)
    return stem, blocks, head


def _flat(stem, blocks, head):
    return [stem] + [l for layers, _ in blocks for l in layers] + [head]


class _Kept:
    """What a layer's forward leaves for its backward: x the convolution's input, w its packed filter (OHWI, or [3][3][c]), raw the
    convolution's output, mean / invstd of the batch, y the layer's output."""

    def __init__(self, x, w, raw, mean, invstd, y):
        self.x, self.w, self.raw, self.mean, self.invstd, self.y = x, w, raw, mean, invstd, y


def _layer_forward(layer, x, residual=None):
    bn = layer.bn
    _check_bn(bn)
    if layer.kind == "dw":
        c = x.shape[-1]
        w = hip_ops.pack_dw_weight(layer.conv.weight.detach())
        raw = hip_ops.dwconv3x3_bn_act(x, w, torch.ones(c, device=x.device), torch.zeros(c, device=x.device), layer.stride, hip_ops.ACT_NONE)
    else:
        w = hip_ops.pack_conv_weight(layer.conv.weight.detach())
        raw = hip_ops.conv2d_bn_act(x, w, None, None, None, layer.stride, layer.pad, hip_ops.ACT_NONE)
    y, mean, invstd = hip_ops.bn_map_train_forward_act(raw, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                                       bn.momentum, residual=residual, act=layer.act)
    bn.num_batches_tracked += 1
    return _Kept(x, w, raw, mean, invstd, y)


class Walk:
    """What the forward leaves for the backward (and for the tests that read the device's ReLU6 branches): feat (N, 1280); stem, blocks,
    head of glancer_layers; kept: id(layer) -> _Kept."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def walk_forward(net, x4):
    """The training walk's forward over (N,H,W,4) pixel-major frames -> Walk.  Every running statistic moves once."""
    stem, blocks, head = glancer_layers(net)
    kept = {}
    k = kept[id(stem)] = _layer_forward(stem, x4)
    y = k.y
    for layers, use_res in blocks:
        xin = y
        for layer in layers:
            k = kept[id(layer)] = _layer_forward(layer, y, xin if layer.res else None)
            y = k.y
    k = kept[id(head)] = _layer_forward(head, y)
    net._note_stats_written()
    return Walk(feat=hip_ops.global_avgpool(k.y), stem=stem, blocks=blocks, head=head, kept=kept)


class GlancerFn(torch.autograd.Function):
    """apply(frames_nhwc4, net, *params) -> (N, 1280); params = (conv.weight, bn.weight, bn.bias) of every layer in walk order, so the
    gradients land in their .grad.  The frames take no gradient."""

    @staticmethod
    def forward(ctx, x4, net, *params):
        wk = ctx.walk = walk_forward(net, x4)
        feat, wk.feat = wk.feat, None           # (not kept on ctx: the output owns the node that owns ctx)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        wk = ctx.walk
        flat = _flat(wk.stem, wk.blocks, wk.head)
        index = {id(l): i for i, l in enumerate(flat)}
        need = [ctx.needs_input_grad[2 + 3 * i: 5 + 3 * i] for i in range(len(flat))]
        live = [i for i, n in enumerate(need) if any(n)]
        grads = [(None, None, None)] * len(flat)
        if not live:
            return (None, None) + (None,) * (3 * len(flat))
        earliest = live[0]          # nothing in front of it wants a gradient: the data-gradient chain stops here

        def through(layer, g):
            """The layer's backward for the gradient g at its output -> the gradient at its input (None: nobody in front wants one)."""
            i, k = index[id(layer)], wk.kept[id(layer)]
            gc, dgamma, dbeta = hip_ops.bn_map_train_backward_act(k.raw, k.y, g, layer.bn.weight.detach(), k.mean, k.invstd, act=layer.act)
            dw = None
            if need[i][0]:
                if layer.kind == "dw":
                    dw = hip_ops.dwconv3x3_wgrad(k.x, gc, layer.stride)
                else:
                    cin = layer.conv.weight.shape[1]
                    dw = hip_ops.conv2d_wgrad_rows(k.x, gc, tuple(k.w.shape), layer.stride, layer.pad)[..., :cin].permute(0, 3, 1, 2).contiguous()
            grads[i] = (dw, dgamma, dbeta)
            if i <= earliest:
                return None
            if layer.kind == "dw":
                return hip_ops.dwconv3x3_dgrad(gc, k.w, tuple(k.x.shape), layer.stride)
            return hip_ops.conv2d_dgrad(gc, hip_ops.pack_conv_dgrad_weight(k.w), tuple(k.x.shape), layer.stride, layer.pad)

        head_y = wk.kept[id(wk.head)].y
        g = through(wk.head, hip_ops.global_avgpool_backward(dfeat.contiguous().float(), tuple(head_y.shape)))
        for layers, use_res in reversed(wk.blocks):
            if g is None:
                break
            g_idn = g if use_res and index[id(layers[0])] > earliest else None      # the identity's path to the layers in front of the block
            for layer in reversed(layers):
                g = through(layer, g)
                if g is None:
                    break
            if g is not None and g_idn is not None:
                g = hip_ops.add(g, g_idn)
        else:
            if g is not None:
                through(wk.stem, g)

        out = []
        for (dw, dgamma, dbeta), (nw, ng, nb) in zip(grads, need):
            out += [dw if nw else None, dgamma if ng else None, dbeta if nb else None]
        return (None, None) + tuple(out)


def glancer_features(net, frames_nhwc4):
    """(N, S, S, 4) pixel-major frames -> (N, 1280), the mean over pixels of the head's map, with an autograd graph into every conv weight
    and BatchNorm weight / bias of `net` (a mobilenet.MobileNetV2) that requires grad; BatchNorm on the statistics of the batch."""
    stem, blocks, head = glancer_layers(net)
    params = [p for layer in _flat(stem, blocks, head) for p in layer.params()]
    return GlancerFn.apply(frames_nhwc4.contiguous(), net, *params)
