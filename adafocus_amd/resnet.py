"""Local CNN: a Bottleneck ResNet (50, 101 or 152 layers) with the reference's parameter names, executed by the HIP trunk.

Mirrors the surface of ACT/models/resnet.py that the hot path uses -- ``resnet50()``, ``resnet101()``, ``resnet152()`` (:280-315),
``ResNet.get_featmap(x, pooled)`` (:211-225), ``get_featvec`` (:227-239), ``forward`` (:196-209),
``feature_dim`` (:241-243) and the torchvision state-dict keys -- while the nn.Conv2d / BatchNorm2d
children only hold parameters: their ``forward`` is never called.  All arithmetic runs in
``adaf_resnet50_forward`` (implicit-GEMM MFMA convs with the BN affine, residual add and ReLU in
the epilogue).  The Bottleneck depths are built (the reference's Something-Something TSN takes any torchvision
``resnet*`` by name, STH/models/tsn.py:109-145); the BasicBlock ResNet-18 / -34 are not (TSN.feature_dim is 2048).
"""
import torch
from torch import nn

from . import hip_ops
from .utils import TrainOptIn, nchw_to_nhwc4

__all__ = ["ResNet", "resnet50", "resnet101", "resnet152", "Bottleneck", "DEPTHS"]

DEPTHS = {"resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3), "resnet152": (3, 8, 36, 3)}   # Bottlenecks per stage
_PLANES = ((64, 1), (128, 2), (256, 2), (512, 2))          # (planes, stride of the stage's first block)
DEFAULT_MATH = "f32"      # arithmetic of newly built trunks ("f32" | "split_bf16" | "f16"); ResNet.set_math overrides per model
MATH_MODES = ("f32", "split_bf16", "f16")


def check_local_math(mode, local_arch="resnet50"):
    """Validates the build-specific ``args.local_math`` of the GFV models: the ResNet local CNN's arithmetic ("f32" default,
    "split_bf16", "f16"), at every depth of DEPTHS.  An EfficientNet local CNN keeps its own ``local_dtype``: any value but "f32" is
    refused there."""
    if mode not in MATH_MODES:
        raise ValueError("local_math must be one of %s, got %r" % (", ".join(MATH_MODES), mode))
    if local_arch not in DEPTHS and mode != "f32":
        raise ValueError("local_math=%r applies to the ResNet local CNN only (local_arch=%r: use local_dtype)" % (mode, local_arch))
    return mode


class Bottleneck(nn.Module):
    """Parameter container for one residual block (ACT/models/resnet.py:74-114)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride, with_downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = None
        if with_downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes * 4))
        self.stride = stride

    def forward(self, x):
        raise RuntimeError("Bottleneck is a parameter container; the block runs inside adaf_resnet50_forward")


class ResNet(TrainOptIn, nn.Module):
    def __init__(self, num_classes=1000, layers=DEPTHS["resnet50"]):
        super().__init__()
        if tuple(layers) not in DEPTHS.values():
            raise NotImplementedError("adafocus_amd.ResNet: Bottleneck layers %s; the trunk runs %s" % (
                list(layers), ", ".join("%s %s" % (k, list(v)) for k, v in DEPTHS.items())))
        self.layers = tuple(int(b) for b in layers)
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, ((planes, stride), blocks) in enumerate(zip(_PLANES, self.layers), start=1):
            seq = [Bottleneck(inplanes, planes, stride, True)]
            inplanes = planes * 4
            seq += [Bottleneck(inplanes, planes, 1, False) for _ in range(blocks - 1)]
            setattr(self, "layer%d" % i, nn.Sequential(*seq))
        self.fc = nn.Linear(2048, num_classes)
        for m in self.modules():  # same initialisation family as the reference (resnet.py:152-157)
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self.tsm_segments = 0     # > 0: temporal shift before the Bottleneck conv1s (TSM, STH; which ones: shifted_blocks)
        self.tsm_div = 8
        self.tsm_place = "blockres"   # 'blockres': shift inside the Bottleneck conv1s; 'block': in front of every whole Bottleneck
        self._trunk = None
        self._sig = None

    @property
    def n_round(self):
        """make_temporal_shift's stride over the blocks of a stage under 'blockres' (STH/ops/temporal_shift.py:123-127): 2 when layer3
        has 23 or more blocks (ResNet-101 / -152), else 1."""
        return 2 if self.layers[2] >= 23 else 1

    def shifted_blocks(self, stage):
        """Indices of the blocks of layer<stage> whose conv1 the 'blockres' shift wraps (the library derives the same set itself)."""
        return [i for i in range(self.layers[stage - 1]) if i % self.n_round == 0]

    # ---- weight hand-off to the library -------------------------------------------------
    def _trunk_params(self):
        out = {}
        for k, v in self.state_dict().items():
            if not (k.startswith("fc.") or k.endswith("num_batches_tracked")):
                out[k] = v
        return out

    def _sync(self):
        params = self._trunk_params()
        dev = next(iter(params.values())).device
        if dev.type != "cuda":
            raise RuntimeError("adafocus_amd.ResNet runs on MI355X only; move the module to the GPU (.cuda())")
        # (the batch-statistics walk writes the running statistics from its kernels, which no tensor version sees: its own count)
        sig = tuple((v.data_ptr(), v._version) for v in params.values()) + (getattr(self, "_stats_written", 0),)
        if self._trunk is None or self._trunk.device != dev or sig != self._sig:
            if self._trunk is None or self._trunk.device != dev:
                self._trunk = hip_ops.ResNet50Trunk(dev)
                self._trunk.set_math(getattr(self, "_math", None) or DEFAULT_MATH)
                self._trunk.set_fusion(getattr(self, "_fusion", True))
            self._trunk.load(params)
            self._sig = sig
        if getattr(self._trunk, "_place", "blockres") != self.tsm_place:
            self._trunk.set_shift_place(self.tsm_place)
            self._trunk._place = self.tsm_place
        return self._trunk

    def set_fusion(self, on):
        """Trunk layer fusion (stage-1 bottleneck tails, stem + max-pool) on / off; bit-identical either way."""
        self._fusion = int(on)
        if self._trunk is not None:
            self._trunk.set_fusion(on)

    def set_math(self, mode):
        """Opt-in arithmetic of the convolutions: "f32" (default, fp32 matrix pipe), "split_bf16" (fp32 operands
        as three exact bf16 parts on the bf16 matrix pipe, fp32 accumulate) or "f16" (fp16 activations and filters on
        the f16 matrix pipe with fp32 accumulation; fp32 stem and pooled features -- include/adafocus.h ADAF_MATH_F16);
        no reference counterpart."""
        if mode not in MATH_MODES:
            raise ValueError("math must be one of %s, got %r" % (", ".join(MATH_MODES), mode))
        self._math = mode
        if self._trunk is not None:
            self._trunk.set_math(mode)

    @property
    def math(self):
        """The arithmetic the trunk runs with ("f32" | "split_bf16" | "f16")."""
        return getattr(self, "_math", None) or DEFAULT_MATH

    # (the opt-ins set_trainable / set_bn_batch_stats: utils.TrainOptIn.  Stage-3 fine-tuning of the Something-Something tree,
    #  STH/stage3.py:189-193, walks on frozen statistics in eval mode; stage 0 of the ActivityNet tree, ACT/main_dist.py:534-548, DESIGN 3.14,
    #  on batch statistics in train mode; in eval mode the walk runs in the frozen form either way)
    def _note_stats_written(self):
        """The running statistics were written by a kernel: the next _sync folds them anew."""
        self._stats_written = getattr(self, "_stats_written", 0) + 1

    def features_train_nhwc4(self, patches_nhwc4):
        """features_nhwc4 with an autograd graph into the trunk's parameters: BatchNorm on its running statistics (the module is in eval
        mode, as STH/stage3.py:313-317 puts the focuser), the same bits as the eval engine's features.  After optimizer.step() the
        parameter versions change and the next features_nhwc4 re-packs the engine's weights (_sync).  In train mode with
        set_bn_batch_stats(True): BatchNorm on the statistics of the batch (the same walk, trunk_train.walk_forward, in its
        batch-statistics form, trunk_train.BatchForm)."""
        if not self.trainable:
            raise RuntimeError("adafocus_amd.ResNet: the training walk is off; call set_trainable(True) first")
        if self.training and not self.bn_batch_stats:
            raise RuntimeError("adafocus_amd.ResNet trains with frozen BatchNorm statistics only (stage 3: the focuser is in eval mode); "
                               "BatchNorm in batch-statistics mode is not implemented")
        from . import trunk_train
        return trunk_train.trunk_features(self, patches_nhwc4)

    # ---- reference surface --------------------------------------------------------------
    def features_nhwc4(self, patches_nhwc4, out=None):
        """Fast path used by the Focuser: (N,P,P,4) pixel-major patches -> (N,2048)."""
        if self.training:
            raise RuntimeError("adafocus_amd.ResNet implements the eval-mode (offline inference) path only")
        return self._sync().forward(patches_nhwc4, self.tsm_segments, self.tsm_div, out=out)

    def features_from_frames(self, frames, actions, patch_size, frames_per_action=1, out=None):
        """PatchSampler.sample + get_featmap(pooled=True) in one call (ACT/models/gfv_net.py:325-331): frames (N,3,H,W) or pixel-major
        (N,H,W,4), actions (k * N / frames_per_action, 2) -> (k * N, 2048); the stem gathers its own windows (no patch tensor)."""
        if self.training:
            raise RuntimeError("adafocus_amd.ResNet implements the eval-mode (offline inference) path only")
        return self._sync().forward_frames(frames, actions.to(device=frames.device, dtype=torch.float32), patch_size, frames_per_action, self.tsm_segments,
                                           self.tsm_div, out=out)

    def get_featmap(self, x, pooled=True):
        """ACT/models/resnet.py:211-225: the trunk up to layer4, then the global average pool (pooled=True: (N,2048,1,1), the call the
        Focuser makes) or the map itself (pooled=False: (N,2048,s,s), NCHW like the reference's return value)."""
        if self.training:
            raise RuntimeError("adafocus_amd.ResNet implements the eval-mode (offline inference) path only")
        if not pooled:
            fmap, _ = self._sync().forward_map(nchw_to_nhwc4(x), self.tsm_segments, self.tsm_div)
            return fmap.permute(0, 3, 1, 2)
        feat = self.features_nhwc4(nchw_to_nhwc4(x))
        return feat.view(feat.shape[0], 2048, 1, 1)

    def get_featvec(self, x):
        return self.features_nhwc4(nchw_to_nhwc4(x))

    def forward(self, x):
        return hip_ops.linear(self.get_featvec(x), self.fc.weight.detach(), self.fc.bias.detach())

    def forward_train(self, x_nchw):
        """forward with an autograd graph: (N, 3, H, W) frames -> (N, num_classes) logits through the training walk and ``fc`` (the Linear
        and its backward of the Something-Something stage-3 head).  Needs set_trainable(True); which BatchNorm statistics the walk uses
        follows the module's mode (features_train_nhwc4)."""
        from .gfv_net_sth import _FcMeanPool
        feat = self.features_train_nhwc4(nchw_to_nhwc4(x_nchw))
        return _FcMeanPool.apply(feat, self.fc.weight, self.fc.bias, None, feat.shape[0])

    @property
    def feature_dim(self):
        return self.fc.weight.shape[-1]


def resnet50(pretrained=False, progress=True, **kwargs):
    """ACT/models/resnet.py:280.  There is no network here: `pretrained` weights must be supplied
    through load_state_dict (the reference's checkpoints load unchanged)."""
    return ResNet(layers=DEPTHS["resnet50"], **kwargs)


def resnet101(pretrained=False, progress=True, **kwargs):
    """ACT/models/resnet.py:292 (Bottleneck, [3, 4, 23, 3]); weights through load_state_dict, as resnet50."""
    return ResNet(layers=DEPTHS["resnet101"], **kwargs)


def resnet152(pretrained=False, progress=True, **kwargs):
    """ACT/models/resnet.py:304 (Bottleneck, [3, 8, 36, 3]); weights through load_state_dict, as resnet50."""
    return ResNet(layers=DEPTHS["resnet152"], **kwargs)
