"""Training of the ResNet local CNN: the differentiable walk of the trunk, stated once.  ``trunk_features`` is the
network of ``adaf_resnet50_forward``, one launch per layer, with a HIP backward (csrc/conv_bwd.hip, csrc/bn_map.hip).  This file is the
TOPOLOGY: which layer reads what, and what the backward may skip.  How one conv + BatchNorm layer runs -- on frozen statistics (FrozenForm,
the module in eval mode: stage 3 of the Something-Something tree) or on the statistics of the batch (BatchForm, the module in train mode
with ``ResNet.set_bn_batch_stats(True)``: stage 0 and 1 of the ActivityNet tree) -- is a layer form of ``layer_train.py``, shared with the
glancer's walk; the trunk's batch-statistics form calls the relu-flag entry points (``bn_map_train_forward`` / ``_backward``, ``conv2d_wgrad``).

THE WALK
  forward   the stem, the max-pool, the Bottlenecks (conv1, conv2, the downsample branch, conv3 with the residual join) and the pool, with
            the temporal shift where ``ResNet.shifted_blocks`` puts it: 'blockres' fused into conv1, 'block' in front of the whole block.
            Every layer output is kept; the ReLU mask of the backward is ``y > 0`` of the stored output.
  backward  the reverse walk: per layer the gradient goes through the layer's form, which hands back the gradient at the convolution's
            output and the parameter gradients the layer wants; the data gradient runs on the forward engine with the filter transposed and
            rotated (``hip_ops.conv2d_dgrad``).  Launches are skipped for parameters that do not require grad, and the data-gradient chain
            stops at the earliest layer that has a trainable parameter.

Math is fp32 only; generic over ``resnet.DEPTHS``.  Orchestration in Python over ``hip_ops`` and one ``torch.autograd.Function``, as
``policy_train.py``."""
import torch

from . import hip_ops
from .layer_train import BatchForm, FrozenForm, Layer, Walk, take_feat, walk_grads, walk_needs, walk_params

__all__ = ["trunk_features", "TrunkFn", "trunk_layers", "walk_forward", "FrozenForm", "BatchForm"]


def trunk_layers(net):
    """-> (stem layer, [(conv1, conv2, conv3, downsample | None, shifted)] per block in forward order) of an adafocus_amd ResNet."""
    relu, none = hip_ops.ACT_RELU, hip_ops.ACT_NONE          # ReLU behind every BatchNorm (conv3: behind the join), none on the downsample branch
    stem = Layer("conv1", net.conv1, net.bn1, "conv", 2, 3, relu)
    blocks = []
    for stage in range(1, 5):
        shifted = set(net.shifted_blocks(stage))
        for i, blk in enumerate(getattr(net, "layer%d" % stage)):
            p = "layer%d.%d." % (stage, i)
            ds = None if blk.downsample is None else Layer(p + "downsample", blk.downsample[0], blk.downsample[1], "conv", blk.stride, 0, none)
            blocks.append((Layer(p + "conv1", blk.conv1, blk.bn1, "conv", 1, 0, relu), Layer(p + "conv2", blk.conv2, blk.bn2, "conv", blk.stride, 1, relu),
                           Layer(p + "conv3", blk.conv3, blk.bn3, "conv", 1, 0, relu), ds, i in shifted))
    return stem, blocks


def _flat(stem, blocks):
    out = [stem]
    for c1, c2, c3, ds, _ in blocks:
        out += [c1, c2, c3] + ([ds] if ds is not None else [])
    return out


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------
def walk_forward(net, x4, form=None):
    """The training walk's forward -> Walk: feat (N, 2048); stem_out; acts, per block (block input as the identity sees it, conv1's output,
    conv2's output, block output) -- all after ReLU; stem and blocks of trunk_layers; the shift (tsm segments, div, place); form, with its
    per-layer state.  form: a layer_train form; None: as the net's mode says, the batch-statistics form on the relu-flag entry points (the
    one place that says which the trunk calls).  The batch-statistics form moves every running statistic once."""
    if form is None:
        form = BatchForm("relu_flag") if (net.training and net.bn_batch_stats) else FrozenForm()
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
        z1 = form.forward(c1, xin, tsm=fused, div=div)
        z2 = form.forward(c2, z1)
        idn = xin if ds is None else form.forward(ds, xin)
        y = form.forward(c3, z2, residual=idn)
        acts.append((xin, z1, z2, y))
    form.after_forward(net)
    return Walk(feat=hip_ops.global_avgpool(y), stem_out=s, acts=acts, stem=stem, blocks=blocks, tsm=tsm, div=div, place=place, form=form)


class TrunkFn(torch.autograd.Function):
    """apply(patches_nhwc4, net, *walk_params(layers in walk order)) -> (N, 2048), in the form the net's mode selects (walk_forward).  The
    patches take no gradient (the crop has integer origins)."""

    @staticmethod
    def forward(ctx, x4, net, *params):
        wk = ctx.walk = walk_forward(net, x4)
        ctx.x4 = x4
        return take_feat(wk)

    @staticmethod
    def backward(ctx, dfeat):
        wk = ctx.walk
        stem, blocks, acts, form, tsm, div = wk.stem, wk.blocks, wk.acts, wk.form, wk.tsm, wk.div
        flat = _flat(stem, blocks)
        need = walk_needs(ctx, flat)
        grads = {}

        def live(layer):
            return any(need[id(layer)])

        def through(layer, g, x, y=None):
            """The layer's backward for the gradient g at its output, after the form's relu_mask (x: the convolution's input; y: the
            output whose ReLU mask a form that masks in its own backward still applies) -> the gradient at the convolution's output; keeps
            the parameter gradients the layer wants.  Gradients and shifted inputs come in as temporaries and die with the call."""
            gc, grads[id(layer)] = form.backward(layer, g, x, y, need[id(layer)])
            return gc

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
                gc2 = through(c2, form.relu_mask(form.dgrad(c3, gc3, z2.shape), z2), z1, z2)
                if upstream[b] or live(c1):
                    fused = tsm and wk.place != "block" and shifted
                    shift_x = fused and form.wants_input(need[id(c1)])      # conv1 read the shifted map: materialised only for a weight gradient
                    gc1 = through(c1, form.relu_mask(form.dgrad(c2, gc2, z1.shape), z1),
                                  hip_ops.temporal_shift(xin, tsm, div, hip_ops.LAYOUT_NHWC) if shift_x else xin, z1)
                    if upstream[b]:
                        g_out = form.dgrad(c1, gc1, xin.shape)
                        if fused:
                            g_out = hip_ops.temporal_shift_backward(g_out, tsm, div, hip_ops.LAYOUT_NHWC)
            if upstream[b]:
                g_idn = g3 if ds is None else form.dgrad(ds, gcd, xin.shape)
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

        return walk_grads(flat, need, grads)


def trunk_features(net, patches_nhwc4):
    """(N, P, P, 4) pixel-major patches -> (N, 2048) with an autograd graph into every conv weight and BatchNorm weight / bias of `net`
    (an adafocus_amd ResNet) that requires grad.  BatchNorm uses its running statistics (the focuser is in eval mode in stage 3), or, with
    the module in train mode and ``set_bn_batch_stats(True)``, the statistics of the batch (stage 0)."""
    if net.math != "f32":
        raise NotImplementedError("training the local CNN runs in fp32 only: set_math(%r) and set_trainable(True) do not combine "
                                  "(the %s arithmetic has no backward)" % (net.math, net.math))
    return TrunkFn.apply(patches_nhwc4.contiguous(), net, *walk_params(_flat(*trunk_layers(net))))
