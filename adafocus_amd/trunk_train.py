"""Stage-3 training of the Something-Something local CNN: the differentiable walk of the ResNet trunk.

STH/stage3.py:189-193 hands ``focuser.net.get_optim_policies()`` to the optimizer and :313-317 keeps the focuser in eval mode, so the
shipped recipe fine-tunes every convolution and every BatchNorm affine parameter of the TSM-ResNet with FROZEN BatchNorm statistics.
``trunk_features`` is that network, one launch per layer, with a HIP backward (csrc/conv_bwd.hip):

  forward   the stem on the trunk's stem kernel, the max-pool, the Bottlenecks through ``hip_ops.conv2d_bn_act`` and the pool, with the
            folded BN affine, the residual and the temporal shift where ``ResNet.shifted_blocks`` puts it ('block': in front of the whole block) -- the fma chains of the
            engine do not depend on the launch form, so the features are the eval engine's, bit for bit.  Every layer
            output is kept; the ReLU mask of the backward is ``y > 0`` of the stored output.
  backward  the reverse walk: per convolution the split-K weight gradient (unscaled), from it dW = s * G, dbeta and dgamma without a
            pre-BN map (``hip_ops.conv_bn_param_grad``), and the data gradient on the forward engine with the filter transposed,
            rotated and scaled.  Launches are skipped for parameters that do not require grad, and the data-gradient chain stops at the
            earliest layer that has a trainable parameter.  BatchNorm running statistics are never touched.

THE BATCH-STATISTICS FORM (stage 0 of the ActivityNet tree, ACT/main_dist.py:534-548, where the focuser's ResNet is in
train mode): ``ResNet.set_bn_batch_stats(True)`` and the module in train mode select ``walk_forward_batch`` / ``TrunkBatchFn``.

  forward   per layer the convolution on the engine with the identity affine (no scale, no bias, no activation: the raw map), then
            ``hip_ops.bn_map_train_forward`` with the ReLU and, for conv3, the residual; the stem runs on the generic engine too (its own
            kernel has the folded affine and the ReLU built in and hands out no raw map).  The max-pool, the shift in both placements
            and the pool are the frozen walk's.  Kept per layer: the raw map, the output after ReLU, mean and invstd -- twice the
            activation memory of the frozen walk.  Running statistics move once per forward; num_batches_tracked += 1.
  backward  the masked gradient goes through ``hip_ops.bn_map_train_backward`` (the ReLU mask of conv1 / conv2 / the stem inside it; the
            residual join's two gradients are added by ``relu_backward`` first), which gives the gradient at the convolution's output,
            dgamma and dbeta; ``conv2d_wgrad`` of that gradient IS dW, and ``conv2d_dgrad`` takes the filter packed with scale 1.  The
            skipping rules are the frozen walk's.

Math is fp32 only; generic over ``resnet.DEPTHS``.  Orchestration in Python over ``hip_ops`` and one ``torch.autograd.Function`` per form,
as ``policy_train.py``."""
import torch

from . import hip_ops

__all__ = ["trunk_features", "TrunkFn", "TrunkBatchFn", "trunk_layers", "walk_forward", "walk_forward_batch"]

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


class _Packed:
    """The engine-layout operands of one layer, packed from the parameters as they are now."""

    def __init__(self, layer):
        bn = layer.bn
        self.w = hip_ops.pack_conv_weight(layer.conv.weight.detach())
        self.scale, self.bias = hip_ops.fold_bn(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, BN_EPS)


def _conv(layer, pk, x, act, residual=None, tsm=0, div=8):
    return hip_ops.conv2d_bn_act(x, pk.w, pk.scale, pk.bias, residual, layer.stride, layer.pad, act, tsm_segments=tsm, tsm_div=div)


def walk_forward(net, x4):
    """The training walk's forward: -> (features (N, 2048), the packed operands per layer, the stem's output, per block (block input as
    the identity sees it, conv1's output, conv2's output, block output) -- all after ReLU --, the walk's description)."""
    stem, blocks = trunk_layers(net)
    tsm, div, place = int(net.tsm_segments), int(net.tsm_div), net.tsm_place
    pk = {id(l): _Packed(l) for l in _flat(stem, blocks)}
    # (the stem on the trunk's own kernel: the generic engine adds its 147 products in another order)
    s = hip_ops.stem7x7_bn_relu(x4, stem.conv.weight.detach(), pk[id(stem)].scale, pk[id(stem)].bias)
    y = hip_ops.maxpool3x3s2(s)
    acts = []
    for c1, c2, c3, ds, shifted in blocks:
        xin = y
        if tsm and place == "block":
            xin = hip_ops.temporal_shift(y, tsm, div, hip_ops.LAYOUT_NHWC)
        fused = tsm if (tsm and place != "block" and shifted) else 0
        z1 = _conv(c1, pk[id(c1)], xin, hip_ops.ACT_RELU, tsm=fused, div=div)
        z2 = _conv(c2, pk[id(c2)], z1, hip_ops.ACT_RELU)
        idn = xin if ds is None else _conv(ds, pk[id(ds)], xin, hip_ops.ACT_NONE)
        y = _conv(c3, pk[id(c3)], z2, hip_ops.ACT_RELU, residual=idn)
        acts.append((xin, z1, z2, y))
    return hip_ops.global_avgpool(y), pk, s, acts, (stem, blocks, tsm, div, place)


class TrunkFn(torch.autograd.Function):
    """apply(patches_nhwc4, net, *params) -> (N, 2048); params = (conv.weight, bn.weight, bn.bias) of every layer in walk order, so the
    gradients land in their .grad.  The patches take no gradient (the crop has integer origins)."""

    @staticmethod
    def forward(ctx, x4, net, *params):
        feat, ctx.pk, ctx.s, ctx.acts, ctx.walk = walk_forward(net, x4)
        ctx.x4 = x4
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        stem, blocks, tsm, div, place = ctx.walk
        pk, acts = ctx.pk, ctx.acts
        flat = _flat(stem, blocks)
        need = {id(l): ctx.needs_input_grad[2 + 3 * i: 5 + 3 * i] for i, l in enumerate(flat)}
        grads = {}

        def live(layer):
            return any(need[id(layer)])

        def param_grads(layer, x, g):
            if not live(layer):
                return
            nw, ng, nb = need[id(layer)]
            p, bn = pk[id(layer)], layer.bn
            raw = hip_ops.conv2d_wgrad(x, g, tuple(p.w.shape), layer.stride, layer.pad)
            grads[id(layer)] = hip_ops.conv_bn_param_grad(g, raw, p.w, p.scale, bn.running_mean, bn.running_var, BN_EPS,
                                                          layer.conv.weight.shape[1], want_dw=nw, want_affine=ng or nb)

        def dgrad(layer, g, x_shape):
            p = pk[id(layer)]
            return hip_ops.conv2d_dgrad(g, hip_ops.pack_conv_dgrad_weight(p.w, p.scale), tuple(x_shape), layer.stride, layer.pad)

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
            param_grads(c3, z2, g3)
            if ds is not None:
                param_grads(ds, xin, g3)
            g_out = g_idn = None
            if upstream[b] or live(c1) or live(c2):
                g2 = hip_ops.relu_backward(dgrad(c3, g3, z2.shape), z2)
                param_grads(c2, z1, g2)
                if upstream[b] or live(c1):
                    g1 = hip_ops.relu_backward(dgrad(c2, g2, z1.shape), z1)
                    fused = tsm and place != "block" and shifted
                    if live(c1):
                        param_grads(c1, hip_ops.temporal_shift(xin, tsm, div, hip_ops.LAYOUT_NHWC) if fused else xin, g1)
                    if upstream[b]:
                        g_out = dgrad(c1, g1, xin.shape)
                        if fused:
                            g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
            if upstream[b]:
                g_idn = g3 if ds is None else dgrad(ds, g3, xin.shape)
                if tsm and place == "block":            # the whole block read the shifted map
                    g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
                    g_idn = hip_ops.temporal_shift_backward(g_idn, tsm, div, hip_ops.LAYOUT_NHWC)
        else:
            if live(stem):
                # the pooled map is a maximum of ReLU outputs: where it is 0 its arg-max is a stem output of 0, which the stem's own ReLU
                # mask zeroes anyway, so joining the two gradients under the mask `pooled > 0` changes nothing downstream
                pooled = hip_ops.maxpool3x3s2(ctx.s)
                gp = hip_ops.relu_backward(g_out, pooled, g_idn)
                gs = hip_ops.relu_backward(hip_ops.maxpool3x3s2_backward(ctx.s, gp), ctx.s)
                param_grads(stem, ctx.x4, gs)

        out = []
        for layer in flat:
            got = grads.get(id(layer), (None, None, None))
            nw, ng, nb = need[id(layer)]
            out += [got[0] if nw else None, got[1] if ng else None, got[2] if nb else None]
        return (None, None) + tuple(out)


# ---- the batch-statistics form ------------------------------------------------------------------------------------------------------------
class _Kept:
    """What the backward needs of one conv + BatchNorm(batch statistics): the raw conv map and the statistics it was normalised with."""

    def __init__(self, raw, mean, invstd):
        self.raw, self.mean, self.invstd = raw, mean, invstd


def _check_bn(bn):
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise NotImplementedError("BatchNorm with momentum=None, without running statistics or without affine parameters")


def _conv_raw(layer, w, x, tsm=0, div=8):
    return hip_ops.conv2d_bn_act(x, w, None, None, None, layer.stride, layer.pad, hip_ops.ACT_NONE, tsm_segments=tsm, tsm_div=div)


def _bn_batch(layer, raw, relu, residual=None):
    """BatchNorm of `layer` on the statistics of `raw` [+ residual] [+ ReLU], as the module in train mode: -> (output, _Kept)."""
    bn = layer.bn
    y, mean, invstd = hip_ops.bn_map_train_forward(raw, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                                                   bn.momentum, residual=residual, relu=relu)
    bn.num_batches_tracked += 1
    return y, _Kept(raw, mean, invstd)


def walk_forward_batch(net, x4):
    """walk_forward with BatchNorm on batch statistics: -> (features (N, 2048), the packed filter per layer, the stem's output, per block
    (block input as the identity sees it, conv1's output, conv2's output, block output) -- all after ReLU --, the _Kept of every layer,
    the walk's description).  Moves every running statistic once."""
    stem, blocks = trunk_layers(net)
    tsm, div, place = int(net.tsm_segments), int(net.tsm_div), net.tsm_place
    flat = _flat(stem, blocks)
    for l in flat:
        _check_bn(l.bn)
    w = {id(l): hip_ops.pack_conv_weight(l.conv.weight.detach()) for l in flat}
    kept = {}
    # (the stem on the generic engine: the trunk's stem kernel folds the affine and the ReLU in and has no raw form)
    s, kept[id(stem)] = _bn_batch(stem, _conv_raw(stem, w[id(stem)], x4), True)
    y = hip_ops.maxpool3x3s2(s)
    acts = []
    for c1, c2, c3, ds, shifted in blocks:
        xin = y
        if tsm and place == "block":
            xin = hip_ops.temporal_shift(y, tsm, div, hip_ops.LAYOUT_NHWC)
        fused = tsm if (tsm and place != "block" and shifted) else 0
        z1, kept[id(c1)] = _bn_batch(c1, _conv_raw(c1, w[id(c1)], xin, fused, div), True)
        z2, kept[id(c2)] = _bn_batch(c2, _conv_raw(c2, w[id(c2)], z1), True)
        idn = xin
        if ds is not None:
            idn, kept[id(ds)] = _bn_batch(ds, _conv_raw(ds, w[id(ds)], xin), False)
        y, kept[id(c3)] = _bn_batch(c3, _conv_raw(c3, w[id(c3)], z2), True, residual=idn)
        acts.append((xin, z1, z2, y))
    net._note_stats_written()
    return hip_ops.global_avgpool(y), w, s, acts, kept, (stem, blocks, tsm, div, place)


class TrunkBatchFn(torch.autograd.Function):
    """TrunkFn for the batch-statistics form: the same operands and the same skipping rules."""

    @staticmethod
    def forward(ctx, x4, net, *params):
        feat, ctx.w, ctx.s, ctx.acts, ctx.kept, ctx.walk = walk_forward_batch(net, x4)
        ctx.x4 = x4
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        stem, blocks, tsm, div, place = ctx.walk
        w, acts, kept = ctx.w, ctx.acts, ctx.kept
        flat = _flat(stem, blocks)
        need = {id(l): ctx.needs_input_grad[2 + 3 * i: 5 + 3 * i] for i, l in enumerate(flat)}
        grads = {}

        def live(layer):
            return any(need[id(layer)])

        def through_bn(layer, x, g, y=None):
            """BatchNorm backward of `layer` for the gradient g at its output (y: the output after ReLU whose mask g still needs), the
            parameter gradients the layer wants (x: the convolution's input) -> the gradient at the convolution's output."""
            k = kept[id(layer)]
            gc, dgamma, dbeta = hip_ops.bn_map_train_backward(k.raw, y, g, layer.bn.weight.detach(), k.mean, k.invstd)
            dw = None
            if need[id(layer)][0]:           # the weight gradient of the raw convolution is dW itself
                cin = layer.conv.weight.shape[1]
                dw = hip_ops.conv2d_wgrad(x, gc, tuple(w[id(layer)].shape), layer.stride, layer.pad)[..., :cin].permute(0, 3, 1, 2).contiguous()
            grads[id(layer)] = (dw, dgamma, dbeta)
            return gc

        def dgrad(layer, g, x_shape):
            return hip_ops.conv2d_dgrad(g, hip_ops.pack_conv_dgrad_weight(w[id(layer)]), tuple(x_shape), layer.stride, layer.pad)

        upstream, seen = [], live(stem)
        for c1, c2, c3, ds, _ in blocks:
            upstream.append(seen)
            seen = seen or any(live(l) for l in (c1, c2, c3, ds) if l is not None)

        dfeat = dfeat.contiguous().float()
        g_out = g_idn = None
        for b in range(len(blocks) - 1, -1, -1):
            c1, c2, c3, ds, shifted = blocks[b]
            xin, z1, z2, y = acts[b]
            if not (upstream[b] or any(live(l) for l in (c1, c2, c3, ds) if l is not None)):
                break
            if b == len(blocks) - 1:
                g3 = hip_ops.global_avgpool_backward(dfeat, tuple(y.shape), y)
            else:
                g3 = hip_ops.relu_backward(g_out, y, g_idn)
            g_out = g_idn = None
            deeper = upstream[b] or live(c1) or live(c2)
            gc3 = through_bn(c3, z2, g3) if (deeper or live(c3)) else None
            gcd = through_bn(ds, xin, g3) if ds is not None and (upstream[b] or live(ds)) else None
            if deeper:
                gc2 = through_bn(c2, z1, dgrad(c3, gc3, z2.shape), z2)
                if upstream[b] or live(c1):
                    fused = tsm and place != "block" and shifted
                    x1 = hip_ops.temporal_shift(xin, tsm, div, hip_ops.LAYOUT_NHWC) if (fused and need[id(c1)][0]) else xin
                    gc1 = through_bn(c1, x1, dgrad(c2, gc2, z1.shape), z1)
                    if upstream[b]:
                        g_out = dgrad(c1, gc1, xin.shape)
                        if fused:
                            g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
            if upstream[b]:
                g_idn = g3 if ds is None else dgrad(ds, gcd, xin.shape)
                if tsm and place == "block":
                    g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
                    g_idn = hip_ops.temporal_shift_backward(g_idn, tsm, div, hip_ops.LAYOUT_NHWC)
        else:
            if live(stem):
                # (the join under the mask `pooled > 0`: TrunkFn.backward says why that changes nothing downstream)
                pooled = hip_ops.maxpool3x3s2(ctx.s)
                gp = hip_ops.relu_backward(g_out, pooled, g_idn)
                through_bn(stem, ctx.x4, hip_ops.maxpool3x3s2_backward(ctx.s, gp), ctx.s)

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
    fn = TrunkBatchFn if (net.training and net.bn_batch_stats) else TrunkFn
    return fn.apply(patches_nhwc4.contiguous(), net, *params)
