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

Math is fp32 only; generic over ``resnet.DEPTHS``.  Orchestration in Python over ``hip_ops`` and one ``torch.autograd.Function``, as
``policy_train.py``."""
import torch

from . import hip_ops

__all__ = ["trunk_features", "TrunkFn", "trunk_layers", "walk_forward"]

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


def trunk_features(net, patches_nhwc4):
    """(N, P, P, 4) pixel-major patches -> (N, 2048) with an autograd graph into every conv weight and BatchNorm weight / bias of `net`
    (an adafocus_amd ResNet) that requires grad.  BatchNorm uses its running statistics (the focuser is in eval mode in stage 3)."""
    if net.math != "f32":
        raise NotImplementedError("training the local CNN runs in fp32 only: set_math(%r) and set_trainable(True) do not combine "
                                  "(the %s arithmetic has no backward)" % (net.math, net.math))
    stem, blocks = trunk_layers(net)
    params = [p for layer in _flat(stem, blocks) for p in layer.params()]
    return TrunkFn.apply(patches_nhwc4.contiguous(), net, *params)
