"""The conv + BatchNorm layer of the training walks, stated once: what ``trunk_train.py`` (the ResNet local CNN) and
``glancer_train.py`` (the glancer's MobileNetV2) share.  A walk is a topology -- which layer reads what, what is skipped in the
backward -- over a list of ``Layer``s; how ONE layer runs forward and backward is a LAYER FORM, and the forms live here.  A new network to
train is a new list of layers and a walk, not another copy of the layer treatment; a new treatment of a layer is a new form, not a new walk.

  Layer       name, the conv and BatchNorm modules that hold the parameters, kind ('conv' on the engine, 'dw' depthwise 3x3 pad 1), stride,
              pad and the activation behind the BatchNorm.  A residual is no property of the layer: it is an operand of the forward call.
  FrozenForm  BatchNorm on its running statistics (stage 3 of the Something-Something tree: STH/stage3.py:189-193 hands
              ``get_optim_policies()`` to the optimizer and :313-317 keeps the focuser in eval mode).  Forward: one ``conv2d_bn_act`` with the
              folded affine, the activation, the residual and the fused shift, the stem on the trunk's stem kernel -- the fma chains of the
              engine do not depend on the launch form, so the features are the eval engine's, bit for bit.  Backward: the ReLU
              mask, the split-K weight gradient (unscaled), from it dW = s * G, dbeta and dgamma without a pre-BN map
              (``hip_ops.conv_bn_param_grad``); the data gradient's filter is scaled.  Running statistics are never touched.  Engine layers
              only: a depthwise layer has no consumer in this form.
  BatchForm   BatchNorm on the statistics of the batch, as the module in train mode (stage 0 and 1 of the ActivityNet tree,
              ACT/main_dist.py:534-548).  Forward: the RAW convolution -- the engine's ``conv2d_bn_act`` without affine and activation (the
              trunk's stem too: its own kernel has the folded affine and the ReLU built in and hands out no raw map), ``dwconv3x3_bn_act``
              with unit scale and zero bias for the depthwise --, then BatchNorm on the statistics of the map with the layer's activation
              and the call's residual.  Kept per layer: the raw map, mean and invstd -- twice the activation memory of the frozen form.
              Running statistics move once per forward; num_batches_tracked += 1.  Backward: the BatchNorm backward with the activation's
              mask inside gives the gradient at the convolution's output, dgamma and dbeta; the weight gradient of that gradient IS dW
              (split-K on the engine, ``dwconv3x3_wgrad`` for the depthwise), and the data gradient's filter is packed with scale 1.
              The library has two sets of entry points of equal bits for this -- the relu flag with ``conv2d_wgrad``, and the ``_act`` pair
              with ``conv2d_wgrad_rows`` (any cout % 4 == 0) -- and WHICH a walk calls is the walk's, named once where it builds its form.

Also here: the autograd plumbing every walk's ``torch.autograd.Function`` has (``walk_params``, ``walk_needs``, ``walk_grads``, ``take_feat``,
the ``Walk`` bag).  Math is fp32; orchestration in Python over ``hip_ops``."""
import torch

from . import hip_ops

__all__ = ["Layer", "FrozenForm", "BatchForm", "Walk", "walk_params", "walk_needs", "walk_grads", "take_feat"]

BN_EPS = 1e-5      # the eps the engine folds with (csrc/resnet_trunk.hip)


class Layer:
    """One conv + BatchNorm of a walk: the modules that hold its parameters, its geometry and the activation behind the BatchNorm
    (hip_ops.ACT_NONE, ACT_RELU or ACT_RELU6).  kind: 'conv' (the engine) or 'dw' (depthwise 3x3, pad 1)."""

    def __init__(self, name, conv, bn, kind, stride, pad, act):
        self.name, self.conv, self.bn, self.kind, self.stride, self.pad, self.act = name, conv, bn, kind, stride, pad, act

    def params(self):
        return (self.conv.weight, self.bn.weight, self.bn.bias)


_RELU_FLAG = {hip_ops.ACT_NONE: False, hip_ops.ACT_RELU: True}        # (the relu-flag entry points have no ReLU6: a KeyError)


def _check_bn(bn):
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise NotImplementedError("BatchNorm with momentum=None, without running statistics or without affine parameters")


# ---- the layer forms ------------------------------------------------------------------------------------------------------------------------
class _Form:
    def dgrad(self, layer, g, x_shape):
        """The gradient at the convolution's input from the gradient g at its output."""
        if layer.kind == "dw":
            return hip_ops.dwconv3x3_dgrad(g, self.dgrad_weight(layer), tuple(x_shape), layer.stride)
        return hip_ops.conv2d_dgrad(g, self.dgrad_weight(layer), tuple(x_shape), layer.stride, layer.pad)


class FrozenForm(_Form):
    """conv + BatchNorm on its running statistics, folded into one launch.  pk: per layer (OHWI filter, folded scale, folded bias)."""

    def __init__(self):
        self.pk = {}

    def pack(self, layer):
        if layer.kind != "conv":
            raise NotImplementedError("FrozenForm: a %r layer (%s) on frozen statistics is not built" % (layer.kind, layer.name))
        bn = layer.bn
        self.pk[id(layer)] = (hip_ops.pack_conv_weight(layer.conv.weight.detach()),) + hip_ops.fold_bn(
            bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, BN_EPS)

    def stem(self, layer, x4):
        # (the stem on the trunk's own kernel: the generic engine adds its 147 products in another order)
        _, scale, bias = self.pk[id(layer)]
        return hip_ops.stem7x7_bn_relu(x4, layer.conv.weight.detach(), scale, bias)

    def forward(self, layer, x, residual=None, tsm=0, div=8):
        w, scale, bias = self.pk[id(layer)]
        return hip_ops.conv2d_bn_act(x, w, scale, bias, residual, layer.stride, layer.pad, layer.act, tsm_segments=tsm, tsm_div=div)

    def after_forward(self, net):
        pass

    def wants_input(self, need):
        return any(need)            # dgamma and dbeta come from the weight gradient too

    def relu_mask(self, g, y):
        return hip_ops.relu_backward(g, y)

    def backward(self, layer, g, x, y, need):
        if not any(need):
            return g, None
        (w, scale, _), bn = self.pk[id(layer)], layer.bn
        raw = hip_ops.conv2d_wgrad(x, g, tuple(w.shape), layer.stride, layer.pad)
        return g, hip_ops.conv_bn_param_grad(g, raw, w, scale, bn.running_mean, bn.running_var, BN_EPS, layer.conv.weight.shape[1],
                                             want_dw=need[0], want_affine=need[1] or need[2])

    def dgrad_weight(self, layer):
        w, scale, _ = self.pk[id(layer)]
        return hip_ops.pack_conv_dgrad_weight(w, scale)


class BatchForm(_Form):
    """The raw convolution, then BatchNorm on the statistics of its map, as the module in train mode.  entry: which of the library's two
    sets of entry points the walk calls, 'relu_flag' (bn_map_train_forward / _backward, conv2d_wgrad; no ReLU6) or 'act'
    (bn_map_train_forward_act / _backward_act, conv2d_wgrad_rows).  w: per layer the packed filter (OHWI, or [3][3][c]); kept: per layer
    what the backward needs, (the raw conv map, mean, invstd)."""

    def __init__(self, entry):
        self.act_entry = {"relu_flag": False, "act": True}[entry]
        self.w, self.kept = {}, {}

    def pack(self, layer):
        _check_bn(layer.bn)
        w = layer.conv.weight.detach()
        self.w[id(layer)] = hip_ops.pack_dw_weight(w) if layer.kind == "dw" else hip_ops.pack_conv_weight(w)

    def stem(self, layer, x4):
        # (the stem on the generic engine: the trunk's stem kernel folds the affine and the ReLU in and has no raw form)
        return self.forward(layer, x4)

    def forward(self, layer, x, residual=None, tsm=0, div=8):
        bn, w = layer.bn, self.w[id(layer)]
        if layer.kind == "dw":
            c = x.shape[-1]
            raw = hip_ops.dwconv3x3_bn_act(x, w, torch.ones(c, device=x.device), torch.zeros(c, device=x.device), layer.stride, hip_ops.ACT_NONE)
        else:
            raw = hip_ops.conv2d_bn_act(x, w, None, None, None, layer.stride, layer.pad, hip_ops.ACT_NONE, tsm_segments=tsm, tsm_div=div)
        args = (raw, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps, bn.momentum)
        if self.act_entry:
            y, mean, invstd = hip_ops.bn_map_train_forward_act(*args, residual=residual, act=layer.act)
        else:
            y, mean, invstd = hip_ops.bn_map_train_forward(*args, residual=residual, relu=_RELU_FLAG[layer.act])
        bn.num_batches_tracked += 1
        self.kept[id(layer)] = (raw, mean, invstd)
        return y

    def after_forward(self, net):
        net._note_stats_written()

    def wants_input(self, need):
        return need[0]

    def relu_mask(self, g, y):
        return g                             # (the BatchNorm backward applies it)

    def backward(self, layer, g, x, y, need):
        """g: the gradient at the layer's output; x: the convolution's input; y: the output whose activation mask is still to be applied
        (None: none, or g has it) -> (the gradient at the convolution's output, (dW in PyTorch's layout | None, dgamma, dbeta))."""
        raw, mean, invstd = self.kept[id(layer)]
        if self.act_entry:
            gc, dgamma, dbeta = hip_ops.bn_map_train_backward_act(raw, y, g, layer.bn.weight.detach(), mean, invstd, act=layer.act)
        else:
            gc, dgamma, dbeta = hip_ops.bn_map_train_backward(raw, y, g, layer.bn.weight.detach(), mean, invstd)
        dw = None
        if need[0] and layer.kind == "dw":
            dw = hip_ops.dwconv3x3_wgrad(x, gc, layer.stride)
        elif need[0]:                        # the weight gradient of the raw convolution is dW itself
            wgrad = hip_ops.conv2d_wgrad_rows if self.act_entry else hip_ops.conv2d_wgrad
            cin = layer.conv.weight.shape[1]
            dw = wgrad(x, gc, tuple(self.w[id(layer)].shape), layer.stride, layer.pad)[..., :cin].permute(0, 3, 1, 2).contiguous()
        return gc, (dw, dgamma, dbeta)

    def dgrad_weight(self, layer):
        w = self.w[id(layer)]
        return w if layer.kind == "dw" else hip_ops.pack_conv_dgrad_weight(w)


# ---- what every walk's autograd Function does: apply(x4, net, *walk_params(layers)) ---------------------------------------------------------
class Walk:
    """What a walk's forward leaves for its backward (and for the tests that read the device's activation branches): feat, the layers
    and the kept outputs as the walk names them, form with its per-layer state."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def walk_params(layers):
    """(conv.weight, bn.weight, bn.bias) of every layer in walk order: handed to the Function so that the gradients land in their .grad."""
    return [p for layer in layers for p in layer.params()]


def walk_needs(ctx, layers):
    """id(layer) -> which of (dW, dgamma, dbeta) autograd wants, from the Function's inputs (x4, net, *walk_params(layers))."""
    return {id(l): ctx.needs_input_grad[2 + 3 * i: 5 + 3 * i] for i, l in enumerate(layers)}


def walk_grads(layers, need, grads):
    """What the Function's backward returns: nothing for x4 and net, then per layer the wanted ones of grads[id(layer)] (absent or None: the layer's
    backward did not run)."""
    out = []
    for layer in layers:
        got = grads.get(id(layer)) or (None, None, None)
        out += [g if n else None for g, n in zip(got, need[id(layer)])]
    return (None, None) + tuple(out)


def take_feat(wk):
    """The features out of the saved walk (not kept on ctx: the output owns the node that owns ctx)."""
    feat, wk.feat = wk.feat, None
    return feat
