"""The numerics contract of EfficientNet in fp16 storage (adaf_effnet_set_dtype(ADAF_DTYPE_F16)) as a CPU model -- a test helper.

The contract itself is written down once, in include/adafocus.h ("EfficientNet, fp16 storage: numerics contract", next to
adaf_effnet_set_dtype); DESIGN.md 3.7.4 points there.  This module restates it on the CPU with the structure of
oracle/ref_effnet.py (block_list, same_pad, out_size, BN_EPS, PARAMS; `_mbconv` mirrors ref_effnet.mbconv line by line): the same
code runs its convolutions in fp32 or in fp64 (`dtype`) and rounds to fp16 (`.half().to(dtype)`) ONLY at the contract's rounding
points, so nothing but the order of the fp32 sums separates it from the kernels.  Every launch plan of the fp16 network is held to
it (tests/test_effnet_contract_gpu.py); tests/test_effnet_contract_host.py pins its structure to the oracle and shows that it
tells five wrong placements of a rounding, a padding or the identity apart -- or says where it cannot.

Rounding points, each read off the kernels (csrc = adafocus_amd/csrc):

  filters    The 1x1 filters (expand, project, head) are rounded to fp16 at finalize: effnet_net.hip:302-305
             (adaf_launch_pack_weight_f16 for every conv with k == 1 that is not depthwise) and, for the whole-block kernel,
             effnet_net.hip:337-338 (adaf_launch_pack_bfrag_f16, mbconv_whole.hip:637-639: the same rounding of the same fp32
             values into fragment order).  Depthwise taps, every folded BN affine, the SE matrices and biases stay fp32
             (effnet_net.hip:323-329, 339-341).  The STEM filter stays fp32 as well: k == 3, so effnet_net.hip:302 skips it, and the stem
             kernels multiply fp32 frames by fp32 taps on the fp32 matrix pipe (effnet_kernels.hip:1396-1409).
  stem       fp32 products, BN affine as one fma, swish, ONE rounding at the store: effnet_kernels.hip:1419 / 1441 (Chunk<T>::pack).
  expand     fp16 operands, fp32 accumulate, fma(acc, scale, bias), swish, one rounding -- in every plan: the conv engine's epilogue
             (conv_gemm.hip:243-249), the strip kernel of the narrow blocks, the expand inside the depthwise launch
             (effnet_kernels.hip:293-299) and the whole-block kernel (mbconv_whole.hip:265-268: the accumulators are rounded before the taps
             read them).
  depthwise  fp32 taps on the (exactly widened) fp16 inputs in (ky, kx) order, fma(acc, scale, bias), swish; the STORED map is
             rounded once (effnet_kernels.hip:438-441, 547-552; mbconv_whole.hip:320-324, 355-359).  The squeeze sums the UNROUNDED fp32
             values in every plan: effnet_kernels.hip:439 (`psum += v` before pack), effnet_kernels.hip:551, mbconv_whole.hip:321 / 356; the mean is
             sum * (1 / hw) (effnet_kernels.hip:876, mbconv_whole.hip:405-414).
  SE gate    fp32 throughout: effnet_kernels.hip:879-929, mbconv_whole.hip:419-494.
  gated A    fp16(float(D16) * gate): effnet_kernels.hip:1023-1030 (gated_project_kernel's staging), the narrow-project strips
             (effnet_kernels.hip:708-709) and mbconv_whole.hip:540-546.
  project    fp16 operands, fp32 accumulate, fma(acc, scale, bias) + float(identity16), one rounding: effnet_kernels.hip:1107-1118 / 1132-1134,
             mbconv_whole.hip:628.  The identity is added AFTER the affine.
  head       fp16 operands (the stored block output, the fp16 head filter), fp32 accumulate, affine, swish; the fp32 map is NOT
             rounded (effnet_net.hip:460: run_dense with an fp32 output) and the pooled vector is the mean of the fp32 map in pixel
             order (effnet_net.hip:463; the pool-in-epilogue form conv_gemm.hip:301, 350 without RND: the same bits).

Not part of the contract (order-dependent fp32 sums, which differ between plans and between this model and the kernels): the k order
of the 1x1 convs' accumulation, the order of the squeeze's pixel sum, the SE dot products, the head pool; and the logistic function
(the kernels use the exp2 / reciprocal units, 1 ulp each).  After a rounding these show up as isolated one-ulp flips; `ulp_error`
measures exactly that.
"""
import torch
import torch.nn.functional as F

from oracle import ref_effnet as R

from tests.test_f16_trunk import SPREAD_FACTOR      # the project's one constant for "how far two implementations of a contract may be apart"

NAME = "efficientnet-b3"
ULP = 2.0 ** -10         # one fp16 ulp relative to the lower end of its binade


class Contract:
    """What the model rounds.  Contract() is the contract; rounding=False turns every rounding off (the oracle's arithmetic); the
    other switches are the WRONG variants the host test must tell apart from the contract:
      squeeze_rounded   (a) the squeeze sums the rounded depthwise map
      gate_unrounded    (b) the gated operand is not rounded before the project conv
      expand_unrounded  (c) the expanded map is not rounded
      swap_pad          (d) pad_before and pad_after of the depthwise conv trade places
      identity_first    (e) the identity is added before the BN affine of the project conv"""

    def __init__(self, rounding=True, squeeze_rounded=False, gate_unrounded=False, expand_unrounded=False, swap_pad=False,
                 identity_first=False):
        self.rounding, self.squeeze_rounded, self.gate_unrounded = rounding, squeeze_rounded, gate_unrounded
        self.expand_unrounded, self.swap_pad, self.identity_first = expand_unrounded, swap_pad, identity_first

    def h(self, t):
        return t.half().to(t.dtype) if self.rounding else t


ROUNDED, UNROUNDED = Contract(), Contract(rounding=False)


def cast_sd(sd, dtype):
    """The state dict's floating tensors in the model's dtype (exact widening of the fp32 parameters)."""
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _affine(sd, p, x):
    """The folded BN affine the kernels apply: scale = w / sqrt(var + eps), bias = b - mean * scale."""
    scale = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + R.BN_EPS)
    bias = sd[p + ".bias"] - sd[p + ".running_mean"] * scale
    return x * scale.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)


def _tap(taps, key, t):
    if taps is not None:
        taps[key] = t
    return t


def _mbconv(sd, p, x, b, pad_size, c, taps=None):
    """ref_effnet.mbconv with the contract's roundings.  x: the block's stored input (fp16 values in `dtype`)."""
    inp = x
    if b["expand"] != 1:
        e = R.swish(_affine(sd, p + "_bn0", F.conv2d(x, c.h(sd[p + "_expand_conv.weight"]))))
        x = e if c.expand_unrounded else _tap(taps, "expand", c.h(e))
    pb, pa = R.same_pad(pad_size, b["k"], b["stride"])
    if c.swap_pad:
        pb, pa = pa, pb
    if pb or pa:
        x = F.pad(x, (pb, pa, pb, pa))
    d = R.swish(_affine(sd, p + "_bn1", F.conv2d(x, sd[p + "_depthwise_conv.weight"], None, b["stride"], 0, 1, b["hid"])))
    d16 = _tap(taps, "dw", c.h(d))
    s = (d16 if c.squeeze_rounded else d).mean((2, 3), keepdim=True)
    s = R.swish(F.conv2d(s, sd[p + "_se_reduce.weight"], sd[p + "_se_reduce.bias"]))
    s = F.conv2d(s, sd[p + "_se_expand.weight"], sd[p + "_se_expand.bias"])
    g = torch.sigmoid(s) * d16
    g = g if c.gate_unrounded else _tap(taps, "gated", c.h(g))
    y = F.conv2d(g, c.h(sd[p + "_project_conv.weight"]))
    skip = b["stride"] == 1 and b["cin"] == b["cout"]
    if skip and c.identity_first:
        y = _affine(sd, p + "_bn2", y + inp)
    else:
        y = _affine(sd, p + "_bn2", y)
        if skip:
            y = y + inp
    return _tap(taps, "out", c.h(y))


def _size(image_size):
    return R.PARAMS[NAME][2] if image_size == "native" else image_size


def contract_stem(sd, x, image_size="native", dtype=torch.float64, c=ROUNDED):
    """Frames (N,3,S,S) -> the stored stem output.  image_size as ref_effnet.extract_features ("native" | int | None)."""
    sd = cast_sd(sd, dtype)
    x = x.to(dtype)
    size = int(_size(image_size) or x.shape[-1])
    return c.h(R.swish(_affine(sd, "_bn0", R._conv_same(x, sd["_conv_stem.weight"], 2, size))))


def contract_block(sd, x, bi, image_size="native", dtype=torch.float64, c=ROUNDED, taps=None):
    """Block bi applied to ITS OWN stored input x (N, cin, h, w), as ref_effnet.mbconv_block."""
    width, depth = R.PARAMS[NAME][:2]
    image_size = _size(image_size)
    blocks = R.block_list(width, depth)
    size = None
    if image_size:
        size = R.out_size(int(image_size), 2)
        for b in blocks[:bi]:
            size = R.out_size(size, b["stride"])
    return _mbconv(cast_sd(sd, dtype), "_blocks.%d." % bi, x.to(dtype), blocks[bi], size if size is not None else x.shape[-1], c, taps)


def contract_head_pooled(sd, x, dtype=torch.float64, c=ROUNDED):
    """The stored output of the last block -> (fp32-contract head map, its pooled vector): nothing is rounded behind the head filter."""
    sd = cast_sd(sd, dtype)
    fmap = R.swish(_affine(sd, "_bn1", F.conv2d(x.to(dtype), c.h(sd["_conv_head.weight"]))))
    return fmap, fmap.mean((2, 3))


def contract_features(sd, x, image_size="native", dtype=torch.float64, c=ROUNDED, upto=None, pooled=True, taps=None):
    """The free-running network, as ref_effnet.extract_features / features_pooled.  upto: the stored output after that many blocks.
    taps: a dict that receives every stored tensor ("stem", "b<i>.expand" / ".dw" / ".gated" / ".out")."""
    width, depth = R.PARAMS[NAME][:2]
    image_size = _size(image_size)
    size = int(image_size or x.shape[-1])
    y = contract_stem(sd, x, image_size, dtype, c)
    _tap(taps, "stem", y)
    sdd = cast_sd(sd, dtype)
    size = R.out_size(size, 2)
    for bi, b in enumerate(R.block_list(width, depth)):
        if upto is not None and bi >= upto:
            return y
        bt = {} if taps is not None else None
        y = _mbconv(sdd, "_blocks.%d." % bi, y, b, size, c, bt)
        if taps is not None:
            taps.update({"b%d.%s" % (bi, k): v for k, v in bt.items()})
        size = R.out_size(size, b["stride"])
    if upto is not None:
        return y
    fmap, vec = contract_head_pooled(sd, y, dtype, c)
    return vec if pooled else fmap


# ---------------------------------------------------------------------------------------------------- the metric and its bound
def ulp_error(got, ref):
    """Element by element, in fp16 ulps of the value itself: |got - ref| / (2^-10 max(|ref|, rms of ref over that image)); the rms floor
    keeps cancelled outputs near zero from dominating.  ref = the fp64 contract model; first axis = images.  Returns the tensor."""
    got, ref = got.double(), ref.double()
    n = ref.shape[0]
    rms = ref.reshape(n, -1).pow(2).mean(1).sqrt().view([n] + [1] * (ref.dim() - 1))
    return (got - ref).abs() / (ULP * torch.maximum(ref.abs(), rms.expand_as(ref)).clamp(min=1e-30))


def ulp_bound(ref32, ref64):
    """(bound, spread): max(1 ulp, SPREAD_FACTOR x the distance between the contract model accumulated in fp32 and in fp64).  One ulp is
    derived, not measured: a sum that lands within fp32 noise of a rounding boundary rounds either way, and that flip is 2^(k-10) on
    a value of at least 2^k."""
    spread = float(ulp_error(ref32, ref64).max())
    return max(1.0, SPREAD_FACTOR * spread), spread


def flip_share(got, ref32):
    """Share of elements that differ at all from the fp32 contract model."""
    return float((got.double() != ref32.double()).double().mean())
