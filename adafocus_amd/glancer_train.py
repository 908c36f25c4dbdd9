"""Training of the glancer's MobileNetV2 (stage 0 of the ActivityNet tree with pretrain_glancer=true: ACT/main_dist.py:534-548,
ACT/models/gfv_net.py:65-66, 90-91): one differentiable walk of the network over its NEUTRAL layer names -- ``stem``,
``b1`` .. ``b17`` with ``expand`` / ``dw`` / ``project``, and ``head``, the names of ``glancer_hip.neutral_params`` -- with a HIP backward.
``glancer_layers`` maps the ActivityNet key layout onto those names; the Something-Something layout can map onto the same walk.

This file is the TOPOLOGY: a chain of blocks, and what the backward may skip.  How one conv + BatchNorm layer runs on the statistics of its
batch is ``layer_train.BatchForm``, shared with the trunk's walk (stage 0 has the whole model in train mode; a frozen-statistics form has no
consumer); the glancer's form calls the ``_act`` entry points (``bn_map_train_forward_act`` / ``_backward_act`` -- ReLU6, 0 < y < 6 on the
stored output in the backward, and no activation on a ``project`` -- and ``conv2d_wgrad_rows``: cout 16, 24 and 144 do not fill a block of
32 filter rows).

THE WALK
  forward   the stem, per block expand / depthwise / project with the block's input as the project's residual in a block with
            use_res_connect, the head, then the mean over pixels.  Kept per layer: its input and its output.
  backward  the reverse walk through the layers' form.  At a residual block the identity's gradient joins the main path's
            (``hip_ops.add``).  Launches for parameters that do not require grad are skipped; the data-gradient chain stops at the earliest
            layer with a trainable parameter; the stem takes no data gradient.

Math is fp32.  Orchestration in Python over ``hip_ops`` and one ``torch.autograd.Function``, as ``trunk_train.py``."""
import torch

from . import hip_ops
from .glancer_hip import _expand_ratios
from .layer_train import BatchForm, Layer, Walk, take_feat, walk_grads, walk_needs, walk_params

__all__ = ["glancer_features", "GlancerFn", "glancer_layers", "walk_forward"]


def glancer_layers(net, variant="act"):
    """-> (stem, [(layers of the block in forward order, use_res_connect)] for b1 .. b17, head) of a mobilenet.MobileNetV2 (the
    ActivityNet key layout: features.i.conv = [expand CBR,] depthwise CBR, project conv, project BN)."""
    if variant != "act":
        raise NotImplementedError("glancer_layers: the %r key layout is not mapped onto the walk (the ActivityNet layout is)" % (variant,))
    f, r6, none = net.features, hip_ops.ACT_RELU6, hip_ops.ACT_NONE
    stem = Layer("stem", f[0][0], f[0][1], "conv", 2, 1, r6)
    blocks = []
    for i, t in enumerate(_expand_ratios(), start=1):
        seq, b, layers, k = f[i].conv, "b%d" % i, [], 0
        if t != 1:
            layers.append(Layer(b + ".expand", seq[0][0], seq[0][1], "conv", 1, 0, r6))
            k = 1
        dw = seq[k][0]
        layers.append(Layer(b + ".dw", dw, seq[k][1], "dw", dw.stride[0], 1, r6))
        layers.append(Layer(b + ".project", seq[k + 1], seq[k + 2], "conv", 1, 0, none))
        blocks.append((layers, f[i].use_res_connect))
    head = Layer("head", f[18][0], f[18][1], "conv", 1, 0, r6)
    return stem, blocks, head


def _flat(stem, blocks, head):
    return [stem] + [l for layers, _ in blocks for l in layers] + [head]


class _Kept:
    """What the walk keeps of a layer beside the form's own state: x the convolution's input, y the layer's output."""

    def __init__(self, x, y):
        self.x, self.y = x, y


def walk_forward(net, x4):
    """The training walk's forward over (N,H,W,4) pixel-major frames -> Walk: feat (N, 1280); stem, blocks, head of glancer_layers; kept:
    id(layer) -> the layer's input x and output y (the tests read the device's ReLU6 branches from y); form, with its per-layer state
    (the raw map, mean and invstd).  Every running statistic moves once."""
    stem, blocks, head = glancer_layers(net)
    form = BatchForm("act")                  # (the one place that says which entry points the glancer calls)
    kept = {}

    def run(layer, x, residual=None):
        form.pack(layer)
        k = kept[id(layer)] = _Kept(x, form.forward(layer, x, residual))
        return k.y

    y = run(stem, x4)
    for layers, use_res in blocks:
        xin = y
        for layer in layers:
            y = run(layer, y, xin if use_res and layer is layers[-1] else None)      # the block's input joins behind its project
    y = run(head, y)
    form.after_forward(net)
    return Walk(feat=hip_ops.global_avgpool(y), stem=stem, blocks=blocks, head=head, kept=kept, form=form)


class GlancerFn(torch.autograd.Function):
    """apply(frames_nhwc4, net, *walk_params(layers in walk order)) -> (N, 1280).  The frames take no gradient."""

    @staticmethod
    def forward(ctx, x4, net, *params):
        ctx.walk = walk_forward(net, x4)
        return take_feat(ctx.walk)

    @staticmethod
    def backward(ctx, dfeat):
        wk = ctx.walk
        flat = _flat(wk.stem, wk.blocks, wk.head)
        index = {id(l): i for i, l in enumerate(flat)}
        need = walk_needs(ctx, flat)
        live = [i for i, l in enumerate(flat) if any(need[id(l)])]
        grads = {}
        if not live:
            return walk_grads(flat, need, grads)
        earliest = live[0]          # nothing in front of it wants a gradient: the data-gradient chain stops here

        def through(layer, g):
            """The layer's backward for the gradient g at its output -> the gradient at its input (None: nobody in front wants one)."""
            k = wk.kept[id(layer)]
            gc, grads[id(layer)] = wk.form.backward(layer, g, k.x, k.y, need[id(layer)])
            return wk.form.dgrad(layer, gc, k.x.shape) if index[id(layer)] > earliest else None

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
        return walk_grads(flat, need, grads)


def glancer_features(net, frames_nhwc4):
    """(N, S, S, 4) pixel-major frames -> (N, 1280), the mean over pixels of the head's map, with an autograd graph into every conv weight
    and BatchNorm weight / bias of `net` (a mobilenet.MobileNetV2) that requires grad; BatchNorm on the statistics of the batch."""
    return GlancerFn.apply(frames_nhwc4.contiguous(), net, *walk_params(_flat(*glancer_layers(net))))
