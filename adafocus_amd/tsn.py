"""TSN wrapper of the local CNN -- host mirror of STH/models/tsn.py for the configurations the
Something-Something drivers use (base_model resnet50 / resnet101 / resnet152, RGB, TSM, no temporal pooling).

``forward(input, no_reshape=True)`` (tsn.py:215-241) = TSM-ResNet trunk -> (N, 2048), executed by
``adaf_resnet50_forward`` with the shift fused into conv1.  State-dict compatibility: the reference
wraps the shifted Bottleneck conv1s in ``TemporalShift`` (key ``...conv1.net.weight``; an unshifted block of a ResNet-101 / -152,
n_round = 2, keeps ``...conv1.weight``; with shift_place='block' every whole Bottleneck: ``layer1.0.net.conv1.weight``) and
STH/evaluate.py:83 re-wraps the children in a Sequential to drop fc (keys ``base_model.4.0.conv1.net.
weight``); both spellings load and save here.
"""
import re

import torch
from torch import nn

from .resnet import DEPTHS, ResNet
from .temporal_shift import make_temporal_shift

__all__ = ["TSN"]

_SEQ = {"conv1": "0", "bn1": "1", "layer1": "4", "layer2": "5", "layer3": "6", "layer4": "7"}
_SEQ_INV = {v: k for k, v in _SEQ.items()}


class TSN(nn.Module):
    def __init__(self, num_segments, modality="RGB", base_model="resnet50", new_length=None, crop_num=1,
                 partial_bn=True, print_spec=False, pretrain="imagenet", is_shift=False, shift_div=8,
                 shift_place="blockres", fc_lr5=False, temporal_pool=False, non_local=False):
        super().__init__()
        if base_model not in DEPTHS:
            raise NotImplementedError("adafocus_amd.TSN: base_model %r is not supported; supported: %s" % (base_model, ", ".join(DEPTHS)))
        if modality != "RGB" or non_local or temporal_pool:
            raise NotImplementedError("adafocus_amd.TSN: RGB without non-local / temporal pooling only")
        self.modality, self.num_segments, self.reshape = modality, num_segments, False
        self.is_shift, self.shift_div, self.shift_place = is_shift, shift_div, shift_place
        self.new_length = 1
        self._enable_pbn = bool(partial_bn)      # STH/models/tsn.py:86-88
        self._stripped = False
        object.__setattr__(self, "_in_init", True)
        self.base_model = ResNet(num_classes=1000, layers=DEPTHS[base_model])
        object.__setattr__(self, "_in_init", False)
        if is_shift:
            make_temporal_shift(self.base_model, num_segments, n_div=shift_div, place=shift_place)
        self._register_load_state_dict_pre_hook(self._canonicalise_keys)
        self._register_state_dict_hook(self._reference_keys)

    # ---- STH/evaluate.py:83 compatibility ------------------------------------------------
    def strip_fc(self):
        """Equivalent of `base_model = Sequential(*children[:-1])`: fc disappears from the state dict and
        the remaining keys take Sequential indices; the HIP trunk is untouched (it never used fc)."""
        self._stripped = True
        return self

    def __setattr__(self, name, value):
        if name == "base_model" and isinstance(value, nn.Sequential) and not getattr(self, "_in_init", True) \
                and "base_model" in self._modules:
            self.strip_fc()          # the unmodified driver line lands here
            return
        super().__setattr__(name, value)

    # ---- key translation -----------------------------------------------------------------
    def _canonicalise_keys(self, state_dict, prefix, *args):
        p = prefix + "base_model."
        for k in [k for k in state_dict if k.startswith(p)]:
            rest = k[len(p):].replace(".conv1.net.", ".conv1.")                      # shift_place = 'blockres': TemporalShift(conv1)
            rest = re.sub(r"^((?:layer)?\d\.\d+)\.net\.", r"\1.", rest)                 # shift_place = 'block': TemporalShift(Bottleneck)
            head, _, tail = rest.partition(".")
            if head in _SEQ_INV:
                rest = _SEQ_INV[head] + "." + tail
            if rest != k[len(p):]:
                state_dict[p + rest] = state_dict.pop(k)
        if self._stripped:           # a stripped checkpoint has no fc; keep ours
            for leaf in ("fc.weight", "fc.bias"):
                state_dict.setdefault(p + leaf, getattr(self.base_model.fc, leaf.split(".")[1]).detach())

    def _reference_keys(self, module, state_dict, prefix, local_metadata):
        p = prefix + "base_model."
        shifted = {s: set(self.base_model.shifted_blocks(s)) for s in range(1, 5)}
        for k in [k for k in state_dict if k.startswith(p)]:
            rest = k[len(p):]
            if self.is_shift and self.shift_place == "block":
                rest = re.sub(r"^(layer\d\.\d+)\.", r"\1.net.", rest)
            elif self.is_shift:       # only the blocks make_temporal_shift wrapped (n_round)
                rest = re.sub(r"^layer(\d)\.(\d+)\.conv1\.", lambda m: m.group(0) + "net." if int(m.group(2)) in shifted[int(m.group(1))]
                              else m.group(0), rest)
            if self._stripped:
                head, _, tail = rest.partition(".")
                if head == "fc":
                    del state_dict[k]
                    continue
                rest = _SEQ[head] + "." + tail
            if rest != k[len(p):]:
                state_dict[p + rest] = state_dict.pop(k)
        return state_dict

    # ---- reference surface ---------------------------------------------------------------
    def forward(self, input, no_reshape=False):
        if not no_reshape:
            input = input.view((-1, 3) + input.size()[-2:])
        return self.base_model.get_featvec(input).squeeze()

    def features_nhwc4(self, patches_nhwc4, out=None):
        return self.base_model.features_nhwc4(patches_nhwc4, out=out)

    def features_from_frames(self, frames, actions, patch_size, frames_per_action=1, out=None):
        return self.base_model.features_from_frames(frames, actions, patch_size, frames_per_action, out=out)

    def features_train_nhwc4(self, patches_nhwc4):
        return self.base_model.features_train_nhwc4(patches_nhwc4)

    def train(self, mode=True):
        """STH/models/tsn.py:146-162: with partial BN, train mode freezes the affine parameters of every BatchNorm2d of the base model
        but the first (requires_grad = False; they stay frozen afterwards, as in the reference).  BatchNorm statistics are frozen in
        every mode here: the trunk runs BatchNorm on its running statistics only."""
        super().train(mode)
        if getattr(self, "_enable_pbn", False) and mode:
            bns = [m for m in self.base_model.modules() if isinstance(m, nn.BatchNorm2d)]
            for m in bns[1:]:
                m.eval()
                m.weight.requires_grad = False
                m.bias.requires_grad = False
        return self

    def partialBN(self, enable):
        self._enable_pbn = enable

    def get_optim_policies(self):
        """STH/models/tsn.py:167-213: the five parameter groups stage 3 hands to SGD, with the reference's names, lr_mult and decay_mult.
        The first convolution's weight; (no convolution has a bias: both bias groups are empty); every other convolution's weight;
        the BatchNorm weights and biases -- all of them, or with partial BN only the first BatchNorm's."""
        convs = [m for m in self.modules() if isinstance(m, nn.Conv2d)]
        bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        for m in self.modules():
            if not m._modules and not isinstance(m, (nn.Conv2d, nn.BatchNorm2d)) and list(m.parameters()) and m is not self.base_model.fc:
                raise ValueError("New atomic module type: %s. Need to give it a learning policy" % type(m))
        first_w, normal_w = [convs[0].weight], [m.weight for m in convs[1:]]
        first_b = [convs[0].bias] if convs[0].bias is not None else []
        normal_b = [m.bias for m in convs[1:] if m.bias is not None]
        bn = [p for m in (bns[:1] if getattr(self, "_enable_pbn", False) else bns) for p in m.parameters()]
        flow = self.modality == "Flow"
        return [{"params": first_w, "lr_mult": 5 if flow else 1, "decay_mult": 1, "name": "first_conv_weight"},
                {"params": first_b, "lr_mult": 10 if flow else 2, "decay_mult": 0, "name": "first_conv_bias"},
                {"params": normal_w, "lr_mult": 1, "decay_mult": 1, "name": "normal_weight"},
                {"params": normal_b, "lr_mult": 2, "decay_mult": 0, "name": "normal_bias"},
                {"params": bn, "lr_mult": 1, "decay_mult": 0, "name": "BN scale/shift"}]

    @property
    def feature_dim(self):
        return 2048
