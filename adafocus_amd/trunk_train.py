"""Training of the ResNet local CNN: the differentiable walk of the trunk, stated once, and the two treatments of a conv + BatchNorm layer
that run through it.  ``trunk_features`` is the network of ``adaf_resnet50_forward``, one launch per layer, with a HIP
backward (csrc/conv_bwd.hip, csrc/bn_map.hip).

THE WALK
  forward   the stem, the max-pool, the Bottlenecks (conv1, conv2, the downsample branch, conv3 with the residual join) and the pool, with
            the temporal shift where ``ResNet.shifted_blocks`` puts it: 'blockres' fused into conv1, 'block' in front of the whole block.
            Every layer output is kept; the ReLU mask of the backward is ``y > 0`` of the stored output.
  backward  the reverse walk: per layer the gradient goes through the layer's form, which hands back the gradient at the convolution's
            output and the parameter gradients the layer wants; the data gradient runs on the forward engine with the filter transposed and
            rotated (``hip_ops.conv2d_dgrad``).  Launches are skipped for parameters that do not require grad, and the data-gradient chain
            stops at the earliest layer that has a trainable parameter.

A LAYER FORM answers what differs between the treatments and nothing else: what is packed per layer, a layer's forward, the gradient
through a layer, whether that needs the convolution's input, the filter of the data gradient, and what happens after the forward.  A new
treatment of a layer is a new form, not a new walk.

  FrozenForm  BatchNorm on its running statistics (stage 3 of the Something-Something tree: STH/stage3.py:189-193 hands
              ``get_optim_policies()`` to the optimizer and :313-317 keeps the focuser in eval mode).  Forward: one ``conv2d_bn_act`` with the
              folded affine, the activation, the residual and the fused shift, the stem on the trunk's stem kernel -- the fma chains of the
              engine do not depend on the launch form, so the features are the eval engine's, bit for bit.  Backward: the ReLU
              mask, the split-K weight gradient (unscaled), from it dW = s * G, dbeta and dgamma without a pre-BN map
              (``hip_ops.conv_bn_param_grad``); the data gradient's filter is scaled.  Running statistics are never touched.
  BatchForm   BatchNorm on the statistics of the batch (stage 0 and 1 of the ActivityNet tree, ACT/main_dist.py:534-548, where the
              focuser's ResNet is in train mode; ``ResNet.set_bn_batch_stats(True)`` and the module in train mode select it).  Forward: the
              convolution with the identity affine (the raw map), then ``hip_ops.bn_map_train_forward`` with the ReLU and, for conv3, the
              residual; the stem runs on the generic engine too (its own kernel has the folded affine and the ReLU built in and hands out
              no raw map).  Kept per layer: the raw map, mean and invstd -- twice the activation memory of the frozen form.  Running
              statistics move once per forward; num_batches_tracked += 1.  Backward: ``hip_ops.bn_map_train_backward`` with the ReLU mask
              inside gives the gradient at the convolution's output, dgamma and dbeta; ``conv2d_wgrad`` of that gradient IS dW, and the data
              gradient's filter is packed with scale 1.

Math is fp32 only; generic over ``resnet.DEPTHS``.  Orchestration in Python over ``hip_ops`` and one ``torch.autograd.Function``, as
``policy_train.py``."""
import torch

from . import hip_ops

__all__ = ["trunk_features", "TrunkFn", "trunk_layers", "walk_forward", "FrozenForm", "BatchForm"]

BN_EPS = 1e-5      # the eps the engine folds with (csrc/resnet_trunk.hip)


class _Layer:
    """One conv + BatchNorm of the walk: the modules that hold its parameters and its geometry."""

    def __init__(self, name, conv, bn, stride, pad):
        self.name, self.conv, self.bn, self.stride, self.pad = name, conv, bn, stride, pad

    def params(self):
        return (self.conv.weight, self.bn.weight, self.bn.bias)


def trunk_layers(net):
    """-> (stem layer, [(conv1, conv2, conv3, downsample | None, shifted)] per block in forward order) of an adafocus_amd ResNet."""
    stem = _Layer("conv1", net.conv1, net.bn1, 2, 3)
    blocks = []
    for stage in range(1, 5):
        shifted = set(net.shifted_blocks(stage))
        for i, blk in enumerate(getattr(net, "layer%d" % stage)):
            p = "layer%d.%d." % (stage, i)
            ds = None if blk.downsample is None else _Layer(p + "downsample", blk.downsample[0], blk.downsample[1], blk.stride, 0)
            blocks.append((_Layer(p + "conv1", blk.conv1, blk.bn1, 1, 0), _Layer(p + "conv2", blk.conv2, blk.bn2, blk.stride, 1),
                           _Layer(p + "conv3", blk.conv3, blk.bn3, 1, 0), ds, i in shifted))
    return stem, blocks


def _flat(stem, blocks):
    out = [stem]
    for c1, c2, c3, ds, _ in blocks:
        out += [c1, c2, c3] + ([ds] if ds is not None else [])
    return out


# ---- the two layer forms --------------------------------------------------------------------------------------------------------------------
class FrozenForm:
    """conv + BatchNorm on its running statistics, folded into one launch.  pk: per layer (OHWI filter, folded scale, folded bias)."""

    def __init__(self):
        self.pk = {}

    def pack(self, layer):
        bn = layer.bn
        self.pk[id(layer)] = (hip_ops.pack_conv_weight(layer.conv.weight.detach()),) + hip_ops.fold_bn(
            bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, BN_EPS)

    def stem(self, layer, x4):
        # (the stem on the trunk's own kernel: the generic engine adds its 147 products in another order)
        _, scale, bias = self.pk[id(layer)]
        return hip_ops.stem7x7_bn_relu(x4, layer.conv.weight.detach(), scale, bias)

    def forward(self, layer, x, relu, residual=None, tsm=0, div=8):
        w, scale, bias = self.pk[id(layer)]
        return hip_ops.conv2d_bn_act(x, w, scale, bias, residual, layer.stride, layer.pad, hip_ops.ACT_RELU if relu else hip_ops.ACT_NONE,
                                     tsm_segments=tsm, tsm_div=div)

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


def _check_bn(bn):
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise NotImplementedError("BatchNorm with momentum=None, without running statistics or without affine parameters")


class BatchForm:
    """The raw convolution, then BatchNorm on the statistics of its map, as the module in train mode.  w: per layer the OHWI filter; kept:
    per layer what the backward needs, (the raw conv map, mean, invstd)."""

    def __init__(self):
        self.w, self.kept = {}, {}

    def pack(self, layer):
        _check_bn(layer.bn)
        self.w[id(layer)] = hip_ops.pack_conv_weight(layer.conv.weight.detach())

    def stem(self, layer, x4):
        # (the stem on the generic engine: the trunk's stem kernel folds the affine and the ReLU in and has no raw form)
        return self.forward(layer, x4, True)

    def forward(self, layer, x, relu, residual=None, tsm=0, div=8):
        bn = layer.bn
        raw = hip_ops.conv2d_bn_act(x, self.w[id(layer)], None, None, None, layer.stride, layer.pad, hip_ops.ACT_NONE, tsm_segments=tsm, tsm_div=div)
        y, mean, invstd = hip_ops.bn_map_train_forward(raw, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                                       bn.momentum, residual=residual, relu=relu)
        bn.num_batches_tracked += 1
        self.kept[id(layer)] = (raw, mean, invstd)
        return y

    def after_forward(self, net):
        net._note_stats_written()

    def wants_input(self, need):
        return need[0]

    def relu_mask(self, g, y):
        return g                             # (bn_map_train_backward applies it)

    def backward(self, layer, g, x, y, need):
        raw, mean, invstd = self.kept[id(layer)]
        gc, dgamma, dbeta = hip_ops.bn_map_train_backward(raw, y, g, layer.bn.weight.detach(), mean, invstd)
        dw = None
        if need[0]:                          # the weight gradient of the raw convolution is dW itself
            cin = layer.conv.weight.shape[1]
            dw = hip_ops.conv2d_wgrad(x, gc, tuple(self.w[id(layer)].shape), layer.stride, layer.pad)[..., :cin].permute(0, 3, 1, 2).contiguous()
        return gc, (dw, dgamma, dbeta)

    def dgrad_weight(self, layer):
        return hip_ops.pack_conv_dgrad_weight(self.w[id(layer)])


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------
class Walk:
    """What the forward leaves for the backward (and for the tests that read the device's ReLU branches): feat (N, 2048); stem_out; acts,
    per block (block input as the identity sees it, conv1's output, conv2's output, block output) -- all after ReLU; stem and blocks of
    trunk_layers; the shift (tsm segments, div, place); form, with its per-layer state."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def walk_forward(net, x4, form=None):
    """The training walk's forward -> Walk.  form: FrozenForm() or BatchForm(); None: as the net's mode says.  The batch-statistics form
    moves every running statistic once."""
    if form is None:
        form = BatchForm() if (net.training and net.bn_batch_stats) else FrozenForm()
    stem, blocks = trunk_layers(net)
    tsm, div, place = int(net.tsm_segments), int(net.tsm_div), net.tsm_place
    for layer in _flat(stem, blocks):
        form.pack(layer)
    s = form.stem(stem, x4)
    y = hip_ops.maxpool3x3s2(s)
    acts = []
    for c1, c2, c3, ds, shifted in blocks:
        xin = y
        if tsm and place == "block":
            xin = hip_ops.temporal_shift(y, tsm, div, hip_ops.LAYOUT_NHWC)
        fused = tsm if (tsm and place != "block" and shifted) else 0
        z1 = form.forward(c1, xin, True, tsm=fused, div=div)
        z2 = form.forward(c2, z1, True)
        idn = xin if ds is None else form.forward(ds, xin, False)
        y = form.forward(c3, z2, True, residual=idn)
        acts.append((xin, z1, z2, y))
    form.after_forward(net)
    return Walk(feat=hip_ops.global_avgpool(y), stem_out=s, acts=acts, stem=stem, blocks=blocks, tsm=tsm, div=div, place=place, form=form)


class TrunkFn(torch.autograd.Function):
    """apply(patches_nhwc4, net, *params) -> (N, 2048), in the form the net's mode selects (walk_forward); params = (conv.weight,
    bn.weight, bn.bias) of every layer in walk order, so the gradients land in their .grad.  The patches take no gradient (the crop has
    integer origins)."""

    @staticmethod
    def forward(ctx, x4, net, *params):
        wk = ctx.walk = walk_forward(net, x4)
        ctx.x4 = x4
        feat, wk.feat = wk.feat, None           # (not kept on ctx: the output owns the node that owns ctx)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        wk = ctx.walk
        stem, blocks, acts, form, tsm, div = wk.stem, wk.blocks, wk.acts, wk.form, wk.tsm, wk.div
        flat = _flat(stem, blocks)
        need = {id(l): ctx.needs_input_grad[2 + 3 * i: 5 + 3 * i] for i, l in enumerate(flat)}
        grads = {}

        def live(layer):
            return any(need[id(layer)])

        def through(layer, g, x, y=None):
            """The layer's backward for the gradient g at its output, after the form's relu_mask (x: the convolution's input; y: the
            output whose ReLU mask a form that masks in its own backward still applies) -> the gradient at the convolution's output; keeps
            the parameter gradients the layer wants.  Gradients and shifted inputs come in as temporaries and die with the call."""
            gc, got = form.backward(layer, g, x, y, need[id(layer)])
            if got is not None:
                grads[id(layer)] = got
            return gc

        def dgrad(layer, g, x_shape):
            return hip_ops.conv2d_dgrad(g, form.dgrad_weight(layer), tuple(x_shape), layer.stride, layer.pad)

        # upstream[b]: some layer in front of block b (the stem or an earlier block) has a trainable parameter
        upstream, seen = [], live(stem)
        for c1, c2, c3, ds, _ in blocks:
            upstream.append(seen)
            seen = seen or any(live(l) for l in (c1, c2, c3, ds) if l is not None)

        dfeat = dfeat.contiguous().float()
        g_out = g_idn = None           # the two gradients that meet at a block's output (main path, identity path)
        for b in range(len(blocks) - 1, -1, -1):
            c1, c2, c3, ds, shifted = blocks[b]
            xin, z1, z2, y = acts[b]
            if not (upstream[b] or any(live(l) for l in (c1, c2, c3, ds) if l is not None)):
                break                                   # nothing trainable here or in front of it
            if b == len(blocks) - 1:                    # the pool's broadcast with the last ReLU folded in
                g3 = hip_ops.global_avgpool_backward(dfeat, tuple(y.shape), y)
            else:
                g3 = hip_ops.relu_backward(g_out, y, g_idn)
            deeper = upstream[b] or live(c1) or live(c2)
            gc3 = through(c3, g3, z2) if (deeper or live(c3)) else None
            gcd = through(ds, g3, xin) if ds is not None and (upstream[b] or live(ds)) else None
            g_out = g_idn = None
            if deeper:
                gc2 = through(c2, form.relu_mask(dgrad(c3, gc3, z2.shape), z2), z1, z2)
                if upstream[b] or live(c1):
                    fused = tsm and wk.place != "block" and shifted
                    shift_x = fused and form.wants_input(need[id(c1)])      # conv1 read the shifted map: materialised only for a weight gradient
                    gc1 = through(c1, form.relu_mask(dgrad(c2, gc2, z1.shape), z1),
                                  hip_ops.temporal_shift(xin, tsm, div, hip_ops.LAYOUT_NHWC) if shift_x else xin, z1)
                    if upstream[b]:
                        g_out = dgrad(c1, gc1, xin.shape)
                        if fused:
                            g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
            if upstream[b]:
                g_idn = g3 if ds is None else dgrad(ds, gcd, xin.shape)
                if tsm and wk.place == "block":         # the whole block read the shifted map
                    g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
                    g_idn = hip_ops.temporal_shift_backward(g_idn, tsm, div, hip_ops.LAYOUT_NHWC)
        else:
            if live(stem):
                # the pooled map is a maximum of ReLU outputs: where it is 0 its arg-max is a stem output of 0, which the stem's own ReLU
                # mask zeroes anyway, so joining the two gradients under the mask `pooled > 0` changes nothing downstream
                pooled = hip_ops.maxpool3x3s2(wk.stem_out)
                gp = hip_ops.relu_backward(g_out, pooled, g_idn)
                through(stem, form.relu_mask(hip_ops.maxpool3x3s2_backward(wk.stem_out, gp), wk.stem_out), ctx.x4, wk.stem_out)

        out = []
        for layer in flat:
            got = grads.get(id(layer), (None, None, None))
            nw, ng, nb = need[id(layer)]
            out += [got[0] if nw else None, got[1] if ng else None, got[2] if nb else None]
        return (None, None) + tuple(out)


def trunk_features(net, patches_nhwc4):
    """(N, P, P, 4) pixel-major patches -> (N, 2048) with an autograd graph into every conv weight and BatchNorm weight / bias of `net`
    (an adafocus_amd ResNet) that requires grad.  BatchNorm uses its running statistics (the focuser is in eval mode in stage 3), or, with
    the module in train mode and ``set_bn_batch_stats(True)``, the statistics of the batch (stage 0)."""
    if net.math != "f32":
        raise NotImplementedError("training the local CNN runs in fp32 only: set_math(%r) and set_trainable(True) do not combine "
                                  "(the %s arithmetic has no backward)" % (net.math, net.math))
    stem, blocks = trunk_layers(net)
    params = [p for layer in _flat(stem, blocks) for p in layer.params()]
    return TrunkFn.apply(patches_nhwc4.contiguous(), net, *params)
