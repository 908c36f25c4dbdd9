"""The float64 statement of the ResNet trunk's front (csrc/stem.hip, the max-pools of csrc/misc_ops.hip), its inputs, and the case tables
of tests/test_stem_forms_gpu.py (tests/test_stem_reference_host.py checks the reference and the tables themselves, without a GPU).  Not
a test module.

    pooled = max_pool2d(relu(conv2d(x[..., :3], w, stride 2, pad 3) * scale + bias), 3, 2, 1)

evaluated by torch on the CPU in float64 (the reference) and in fp32 (the same expression in ATen's order) through heads_reference.measure.
THE TOLERANCE is heads_reference's rule for single products and reductions, imported and not restated: err <= bound_single(spread), both
relative to the output's largest float64 entry.  The fp16 stores have no tolerance: one round-to-nearest-even of the fp32 pooled value,
so torch.equal to .half() of the same form's fp32 output.

INPUTS.  Seeded `rnd` patches, every image its own content (a wrong image index or a conv row carried from one image into the next shows);
w scaled by 147^-0.5; scale uniform in [0.5, 1.5) with scale[1] = 0 and bias[1] < 0 (channel 1 is all zeros after the ReLU) and
scale[2] < 0 (an inverted channel); bias 0.1 x normal.  About 2 % of the pooled map is exactly zero from P = 7 upwards: live windows next
to dead ones, which is where padding the pooling windows with 0 instead of -inf would show if the ReLU did not make it harmless."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from tests import heads_reference as R
from tests.helpers import rnd

bound_single, rel_err = R.bound_single, R.rel_err


# ---- the operation ---------------------------------------------------------------------------------------------------------------------------
def conv_size(p):
    return (p + 6 - 7) // 2 + 1


def pool_size(oh):
    return (oh + 2 - 3) // 2 + 1


def stem(x4, w, scale, bias, dtype=torch.float64):
    """x4 (n, P, P, 4) NHWC4 (lane 3 is not read), w (64, 3, 7, 7), scale, bias (64,) -> {"conv": (n, OH, OH, 64), "pool": (n, PH, PH, 64)}."""
    x = x4[..., :3].permute(0, 3, 1, 2).to(dtype)
    y = F.conv2d(x, w.to(dtype), stride=2, padding=3) * scale.to(dtype).view(1, -1, 1, 1) + bias.to(dtype).view(1, -1, 1, 1)
    y = F.relu(y)
    return {"conv": y.permute(0, 2, 3, 1).contiguous(), "pool": F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).contiguous()}


def measure(x4, params):
    """-> heads_reference.Ref with the outputs 'conv' and 'pool' of these images."""
    return R.measure(lambda dt: stem(x4, *params, dtype=dt))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def params(seed=8100):
    """-> (w (64, 3, 7, 7), scale (64,), bias (64,))."""
    w = rnd((64, 3, 7, 7), seed, 147 ** -0.5)
    g = np.random.Generator(np.random.PCG64([seed, 1]))
    scale = torch.from_numpy((g.random(64, dtype=np.float32) + np.float32(0.5)))
    bias = rnd((64,), seed + 1, 0.1)
    scale[1] = 0.0
    bias[1] = -bias[1].abs() - 0.05
    scale[2] = -scale[2]
    return w, scale, bias


def patches(n, p, seed=8200, lane3=0.0):
    """(n, P, P, 4) patches: three seeded normal lanes, lane 3 = `lane3`."""
    x4 = torch.full((n, p, p, 4), float(lane3))
    x4[..., :3] = rnd((n, p, p, 3), seed + p)
    return x4


def frames(nf, h, w, seed=8300):
    """Planar (nf, 3, H, W) frames."""
    return rnd((nf, 3, h, w), seed + h + w)


def held_images(n, per_round=0):
    """The images of a case that are held to float64: all of them up to 8; else image 0, image n - 1, the first two and the last image
    of every later round of a persistent grid that takes `per_round` images per round, then the lowest indices up to 8 at least."""
    if n <= 8:
        return list(range(n))
    want = [0, n - 1]
    if 0 < per_round < n:
        for first in range(per_round, n, per_round):
            want += [first, min(first + 1, n - 1), min(first + per_round - 1, n - 1)]
    i = 1
    while len(set(want)) < 8:
        want.append(i)
        i += 1
    return sorted(set(want))


_REFS = {}


def reference(key, x4, idx, prm):
    """The Ref of images `idx` of x4, computed once per `key` and never changed."""
    k = (key, tuple(idx))
    if k not in _REFS:
        _REFS[k] = measure(x4[list(idx)].contiguous(), prm)
    return _REFS[k]


# ---- the kernels' geometry, restated from csrc/stem.hip -------------------------------------------------------------------------------------------
N = collections.namedtuple("N", "cus bpc_cus plus", defaults=(0, 0, 0))        # n = cus x CUs + bpc_cus x CUs x BPC + plus


def images(spec, cus, bpc=1):
    return spec.cus * cus + spec.bpc_cus * cus * bpc + spec.plus


def tile_waves(tph):
    """PoolCfg<TPH>::NWV: (2 TPH + 1) x 17 conv pixels in waves of 32."""
    return ((2 * tph + 1) * 17 + 31) // 32


def tile_rows(p):
    """The tile height the cost rule picks (adaf_stem7x7_pool_pays: 6 where the 6-row cover takes fewer waves, else 4)."""
    ph = pool_size(conv_size(p))
    return 6 if -(-ph // 6) * tile_waves(6) < -(-ph // 4) * tile_waves(4) else 4


STRIP = {64: (32, 4), 96: (48, 8), 128: (64, 2), 144: (72, 4)}                 # P -> (OW, R) of launch_rows_for
MAXO = 32                                                                      # window origins a strip block keeps in LDS


def strip_bpc(p):
    """RowsCfg<OW, R>::BPC: strip blocks per CU by their LDS footprint (filter bank + window + 36-float staging pixels) against 160 KB."""
    ow, r = STRIP[p]
    win = ((2 * r + 5) * (2 * ow + 5) * 3 + 3) & ~3
    ldsf = 2 * 74 * 64 + win + r * ow * 36
    return 2 if (ldsf * 4 + 1023) // 1024 * 1024 * 2 <= 160 * 1024 else 1


def walk_form(p, n, cus):
    """adaf_stem7x7_plan with fusion on and the default options: what the trunk's walk launches."""
    if p in STRIP and n >= cus:
        return "strip"
    return "tile6" if tile_rows(p) == 6 else "unfused"


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------------
# conv only: 8 x 16 output tiles on a persistent grid of 3 x CUs blocks
CONV_CASES = [(1, N(plus=3)), (2, N(plus=3)), (7, N(plus=3)), (30, N(plus=3)), (33, N(plus=3)), (64, N(plus=3)), (96, N(plus=3)),
              (16, N(cus=3, plus=5))]            # one tile per image, more tiles than blocks: the persistent loop and its prefetch
# pooled tile kernels, both heights forced at every size (persistent grid of 2 x CUs blocks)
TILE_CASES = [(p, N(plus=3)) for p in (1, 2, 7, 18, 37, 50, 98, 100, 96, 128, 144)] + [(37, N(plus=1)), (96, N(plus=1)),
              (32, N(cus=2, plus=9))]            # two tiles per image: the tile loop goes round
TILE_PICKS = {37: 6, 96: 6, 144: 6, 50: 4, 98: 4, 100: 4, 128: 4}
# strip kernel: one image; some blocks with a second image (BPC = 1) or none (BPC = 2); blocks with two and blocks with three images
STRIP_CASES = [(p, spec) for p in sorted(STRIP) for spec in (N(plus=1), N(cus=1, plus=3), N(bpc_cus=2, plus=5))]
AUTO_SIZES = (96, 128, 144, 160, 176, 192, 224)
AUTO_N = (N(plus=8), N(cus=1, plus=3))

Gather = collections.namedtuple("Gather", "p h w nf fpa k actions lane3", defaults=("edges", 0.0))
GATHER_CASES = [
    Gather(64, 101, 101, 8, 1, 1),               # H - P = 37: not a multiple of 4; the corners, products on and beside an integer, clamped values
    Gather(64, 101, 101, 1, 1, 1),               # a single patch
    Gather(96, 96, 96, 8, 8, 2),                 # H = P: every origin is 0; one action per clip of 8 frames, two action sets
    Gather(64, 80, 100, 8, 1, 2),                # a wide frame: the span is H - P on both axes, x clamped to W - P
    Gather(128, 171, 171, 8, 8, 2),              # H - P = 43
    Gather(144, 224, 224, 8, 1, 1),
    Gather(96, 224, 224, 8, 1, 2, "edges", 1e30),  # lane 3 of the pixel-major frames and of the NHWC4 patches is not read
]


def edge_actions(span, count, seed):
    """(count, 2) fp32 (y, x) actions: the corners {0, 1}^2, values whose fp32 product with `span` lands on an integer and one ulp to
    either side of it, -0.25 and 1.5 (clamped like crop_kernel), then uniform draws."""
    one = np.float32(1.0)
    vals = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)]
    if span > 1:
        for j in (1, span // 2, span - 1):
            a = np.float32(j) / np.float32(span)
            vals += [(a, np.nextafter(a, one)), (np.nextafter(a, -one), a)]
    vals += [(-0.25, 1.5), (1.5, -0.25)]
    g = np.random.Generator(np.random.PCG64([seed, span]))
    out = g.random((count, 2), dtype=np.float32)
    m = min(count, len(vals))
    # the last two rows of a short table are the clamped pair, whatever else fits
    pick = vals[:m] if m == len(vals) or m < 3 else vals[:m - 2] + vals[-2:]
    out[:m] = np.asarray(pick, dtype=np.float32)
    return torch.from_numpy(out)


def gather_actions(c, seed=8400):
    return edge_actions(c.h - c.p, c.k * c.nf // c.fpa, seed + c.p + c.h)


def origins(actions, h, w, p):
    """floor(action x (H - P)) in fp32 on both axes, y clamped to [0, H - P], x to [0, W - P] (window_origin, csrc/crop.hip) -> int64 (M, 2)."""
    span = np.float32(h - p)
    a = actions.numpy().astype(np.float32)
    o = np.floor(a * span).astype(np.int64)
    o[:, 0] = np.clip(o[:, 0], 0, h - p)
    o[:, 1] = np.clip(o[:, 1], 0, w - p)
    return o


def gather(frames_nchw, actions, p, fpa, k):
    """get_patch on the CPU: patch j * nf + f is the window of frame f at the origin of action j * nf / fpa + f / fpa -> (k nf, P, P, 4),
    lane 3 zero."""
    nf, _, h, w = frames_nchw.shape
    o = origins(actions, h, w, p)
    out = torch.zeros((k * nf, p, p, 4))
    for j in range(k):
        for f in range(nf):
            y0, x0 = o[j * (nf // fpa) + f // fpa]
            out[j * nf + f, :, :, :3] = frames_nchw[f, :, y0:y0 + p, x0:x0 + p].permute(1, 2, 0)
    return out


# stand-alone max-pools
MAXPOOL_SHAPES = [(h, w, c) for h, w in ((1, 1), (1, 5), (2, 2), (7, 10), (8, 8), (15, 15), (48, 48)) for c in (4, 64, 68)]
MAXPOOL_KINDS = ("normal", "negative", "neginf")


def maxpool_input(h, w, c, kind, n=3, seed=8500):
    """(n, h, w, c) NHWC: normal values; all-negative values (the padding must not win: the result is negative); normal values with one
    whole map, and scattered entries of the others, at -inf."""
    x = rnd((n, h, w, c), seed + 100 * h + w + c)
    if kind == "negative":
        x = -x.abs() - 0.5
    elif kind == "neginf":
        x[n - 1] = -float("inf")
        g = np.random.Generator(np.random.PCG64([seed, h, w, c]))
        x[torch.from_numpy(g.random((n, h, w, c)) < 0.3)] = -float("inf")
    return x


def maxpool(x_nhwc):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
