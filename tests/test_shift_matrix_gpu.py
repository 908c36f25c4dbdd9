"""GPU tests of the temporal shift (TSM, STH/ops/temporal_shift.py:28-46) over `shift_div` and the clip length, in every kernel form it
is fused into: the move itself, the conv engine's operand load (general form, lean K loop, split and fp16-operand tiles), the ResNet-50
trunk (fused stage-1 tail with one, two and four passes per fold, tile groups of 120 / 125 / 126 images, both placements, the three
arithmetics) and the MobileNetV2 glancer (materialised copy, expand conv's operand load, strip kernel's pixel loads).

Which form a layer takes is selected by fold = channels / shift_div, and `shift_div` is a user setting (args.shift_div), so each form is
run here at the folds that select it and at their boundaries -- DESIGN.md 3.2.1 has the table.

References: index arithmetic for the move (torch.equal); for everything numeric a plain PyTorch-CPU restatement evaluated in FLOAT64
(oracle.ref_model.temporal_shift in front of F.conv2d, resnet50_trunk, glancer_sth, sth_forward with a .double() state dict and input).

Tolerances.  Moves and plan comparisons (fusion on / off, strips / tiles, lean / select K loop, chunking, clip independence): none,
torch.equal.  Single convs: the suite's CONV_TOL (2e-4, same input and weight scaling as the cases it was set for) and the bounds of
test_conv_f16_operands_vs_fp32_reference for the fp16-operand tiles.  End to end the float32 oracle is itself 8e-4 .. 9.5e-4 (feature
map) away from the float64 oracle at 224^2, so a fixed 1e-3 would measure the reference; instead

    err(kernel, oracle64) <= F_BOUND * err(oracle32, oracle64)        (max abs, same input, per case)

F_BOUND is calibrated on the shift_div = 8 cells of this module (the configuration pinned by goldens from the real reference, G7-STH /
G12 / G13): twice the largest ratio err(kernel, oracle64) / err(oracle32, oracle64) seen there, and not below 2 (two float32
evaluations that differ in summation order; a factor under 2 would flag order noise).  Measured on an MI355X: largest ratio 2.238,
F_BOUND = 4.476 (figures at the constant below).  Every case prints its ratio (pytest -s).  The fp16 trunk is held to
test_f16_trunk.py's contract model and its own calibrated bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib as L
from tests.helpers import rnd, synth_sd
from tests.test_hip_parity import CONV_TOL

pytestmark = pytest.mark.gpu

# Ratios measured on the shift_div = 8 cells (MI355X, 19 figures): ResNet-50 trunk 1.59 .. 2.23 (f32; 360 patches of 48^2, T = 12) and
# 1.97 .. 2.24 (split_bf16; 256 patches of 32^2, T = 8), glancer map 0.74 .. 1.19, glancer logits 0.85 .. 1.10.  Largest: 2.238.
# Over the other shift_div cells the ratio reached 2.54 (trunk), 1.66 (glancer) -- the seeded strip-shift error is 6 000 x / 25 000 x.
F_BOUND = 2 * 2.238

E_BADARG, E_LAYOUT = r"failed \(-1\)", r"failed \(-2\)"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def O():
    from oracle import ref_model
    return ref_model


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def _maxerr(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


def _ratio(tag, got, ref32, ref64):
    """Prints err(kernel, oracle64), err(oracle32, oracle64) and their ratio; returns a message when the bound is missed, else None."""
    err, noise = _maxerr(got, ref64), _maxerr(ref32, ref64)
    print("RATIO %s: kernel-vs-f64 %.3e  oracle32-vs-f64 %.3e  ratio %.3f  (max |ref| %.2f)" % (tag, err, noise, err / noise, ref64.abs().max().item()))
    assert noise > 0.0 and torch.isfinite(got).all()
    return None if err <= F_BOUND * noise else "%s: |kernel - oracle64| = %.3e > %.3f x %.3e (ratio %.1f)" % (tag, err, F_BOUND, noise, err / noise)


def _bounded(tag, got, ref32, ref64):
    """err(kernel, oracle64) <= F_BOUND * err(oracle32, oracle64)."""
    miss = _ratio(tag, got, ref32, ref64)
    assert miss is None, miss


# ------------------------------------------------------------------------------------------------ 1. the move itself
def shift_by_index(x, n_segment, fold_div):
    """TemporalShift.shift by index arithmetic on (NT, C, H, W): channel ch of frame f comes from frame f + 1 (ch < fold), from frame
    f - 1 (fold <= ch < 2 fold) or from f itself; a neighbour outside the clip is zeros.  fold = C // fold_div; fold_div = 1 leaves no
    second or third group (the reference's slices are empty there)."""
    nt, c = x.shape[0], x.shape[1]
    fold = c // fold_div
    out = torch.zeros_like(x)
    for f in range(nt):
        t = f % n_segment
        for ch in range(c):
            src = f + 1 if ch < fold else f - 1 if ch < 2 * fold else f
            if 0 <= t + (src - f) < n_segment:          # else: the neighbour lies outside the clip
                out[f, ch] = x[src, ch]
    return out


MOVE_T = (1, 2, 3, 8, 12)
MOVE_C = (4, 24, 32, 64, 96, 256)


@pytest.mark.parametrize("div", [1, 2, 3, 4, 8, 16])
def test_move_exact(dev, ops, div):
    """adaf_temporal_shift_f32 in both layouts: fold 0 (4 / 8, 4 / 16), odd folds, 2 fold == c, fold == c; clips of one frame (both
    shifted groups all zeros); two clips; a 3 x 3 and a 1 x 1 map."""
    for t in MOVE_T:
        for c in MOVE_C:
            for hw in (3, 1):
                x = rnd((2 * t, c, hw, hw), 1000 + 16 * t + c + hw)
                ref = shift_by_index(x, t, div)
                got = ops.temporal_shift(x.to(dev), t, div).cpu()
                assert torch.equal(got, ref), ("nchw", div, t, c, hw)
                got = ops.temporal_shift(x.permute(0, 2, 3, 1).contiguous().to(dev), t, div, ops.LAYOUT_NHWC).cpu()
                assert torch.equal(got.permute(0, 3, 1, 2), ref), ("nhwc", div, t, c, hw)


def test_move_refusals(dev, ops):
    x = torch.zeros((6, 8, 2, 2), device=dev)
    with pytest.raises(L.AdafError, match=E_BADARG):
        ops.temporal_shift(x, 4, 8)                   # 6 frames are not whole clips of 4
    with pytest.raises(L.AdafError, match=E_BADARG):
        ops.temporal_shift(x, 3, 0)
    with pytest.raises(L.AdafError, match=E_BADARG):
        ops.temporal_shift(x, 0, 8)


# ------------------------------------------------------------------------------------------------ 2. the conv engine's fused shift
GENERAL = [(64, 4), (64, 8), (64, 16), (256, 16), (96, 8)]                                      # fold 16, 8, 4, 16, 12: per-4-channel select
LEAN = [(64, 2), (256, 8), (256, 4), (256, 2), (512, 8), (1024, 4), (2048, 8)]                  # fold 32, 32, 64, 128, 64, 256, 256: whole slices
F32_TILES = (0, 1, 2, 3, 4, 5, 21, 22, 23, 24, 25, 26, 31, 32, 33, 34, 38, 39, 71, 72, 73, 74)
LEAN_TILES = (0, 31, 32, 34, 38, 39)          # DMA tiles larger than 64 x 64 on the fp32 pipe: the ones the lean K loop exists for
SPLIT6, SPLIT9 = (41, 42, 43, 44, 45, 46), (51, 52, 53, 54)
F16_TILES = (0, 81, 82, 83, 84, 88)
COUT, MAP = 96, 3                            # 96 columns: a ragged column tile under 64- and 128-wide tiles


def _images(t):
    """Whole clips giving 270 .. 324 rows of a 3 x 3 map: two full 128-row tiles and a ragged third (256-row tiles: one and a ragged
    second), the last valid row being the last frame of a clip."""
    return {1: 30, 2: 30, 3: 30, 8: 32, 12: 36}[t]


def _conv_inputs(cin, t, seed, f16=False):
    """Same distributions as test_hip_parity._conv_case (fp32) / test_conv_f16_operands_vs_fp32_reference (fp16-valued operands)."""
    g = np.random.Generator(np.random.PCG64([seed, 171]))
    n = _images(t)
    x = torch.from_numpy(g.standard_normal((n, cin, MAP, MAP), dtype=np.float32))
    wscale = 1.0 / np.sqrt(cin) if f16 else np.sqrt(2.0 / cin)
    w = torch.from_numpy(g.standard_normal((COUT, cin, 1, 1), dtype=np.float32) * np.float32(wscale))
    scale = torch.from_numpy(g.uniform(0.5, 1.5, COUT).astype(np.float32))
    bias = torch.from_numpy(g.normal(0, 0.1, COUT).astype(np.float32))
    res = torch.from_numpy(g.standard_normal((n, COUT, MAP, MAP), dtype=np.float32))
    if f16:
        x, w, res = x.half().float(), w.half().float(), res.half().float()
    return x, w, scale, bias, res


def _conv_ref64(O, x, w, scale, bias, res, t, div):
    xin = O.temporal_shift(x.double(), t, div) if t else x.double()
    ref = F.conv2d(xin, w.double()) * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
    if res is not None:
        ref = ref + res.double()
    return F.relu(ref).permute(0, 2, 3, 1)


@pytest.mark.parametrize("t", MOVE_T)
@pytest.mark.parametrize("cin,div", GENERAL + LEAN)
def test_conv_fused_shift_fp32_and_split_tiles(dev, ops, O, cin, div, t):
    """(a) every tile against the float64 conv of the shifted input, (b) lean K loop == per-lane select, (c) all fp32 tiles equal bit for
    bit (one k order), the split tiles among themselves, (d) shifted != unshifted."""
    lean_form = (cin // div) % 32 == 0 and cin % 32 == 0
    assert lean_form == ((cin, div) in LEAN)
    x, w, scale, bias, res = _conv_inputs(cin, t, 7 * cin + div + t)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, sd_, bd = ops.pack_conv_weight(w.to(dev), cin), scale.to(dev), bias.to(dev)
    for with_res in (False, True):
        rd = res.permute(0, 2, 3, 1).contiguous().to(dev) if with_res else None
        ref = _conv_ref64(O, x, w, scale, bias, res if with_res else None, t, div)

        def run(tile, seg=t):
            return ops.conv2d_bn_act(xd, wd, sd_, bd, rd, act=ops.ACT_RELU, tsm_segments=seg, tsm_div=div, tile=tile).cpu()
        worst = 0.0
        outs = {}
        for tile in F32_TILES + SPLIT6 + SPLIT9:
            outs[tile] = run(tile)
            err = _maxerr(outs[tile], ref)
            worst = max(worst, err)
            assert err < CONV_TOL, (cin, div, t, with_res, tile, err)
        print("conv cin=%d div=%d T=%d res=%d: worst |err| vs float64 %.2e over %d tiles" % (cin, div, t, with_res, worst, len(outs)))
        for tile in F32_TILES[1:]:
            assert torch.equal(outs[tile], outs[0]), (cin, div, t, with_res, tile)
        for group in (SPLIT6, SPLIT9):
            for tile in group[1:]:
                assert torch.equal(outs[tile], outs[group[0]]), (cin, div, t, with_res, tile)
        with L.option("tsm_lean", 0):
            for tile in LEAN_TILES:
                assert torch.equal(run(tile), outs[tile]), ("tsm_lean 0", cin, div, t, with_res, tile)
        naive = ops.conv2d_bn_act(xd, wd, sd_, bd, rd, act=ops.ACT_RELU, tsm_segments=t, tsm_div=div, naive=True).cpu()
        assert _maxerr(naive, ref) < CONV_TOL
        assert not torch.equal(run(0, seg=0), outs[0])


@pytest.mark.parametrize("t", MOVE_T)
@pytest.mark.parametrize("cin,div", [(c, d) for c, d in GENERAL + LEAN if (c // d) % 8 == 0])
def test_conv_fused_shift_fp16_operand_tiles(dev, ops, O, cin, div, t):
    """Tiles 81 .. 84, 88: fp16 operands move whole 16-byte chunks (folds that are multiples of 8).  Operands that are fp16 values: the
    products are exact, only the summation order (fp32 store) or one rounding (fp16 store) separates the tiles from the float64 conv."""
    x, w, scale, bias, res = _conv_inputs(cin, t, 9 * cin + div + t, f16=True)
    xd = x.permute(0, 2, 3, 1).contiguous().half().to(dev)
    wd = ops.pack_conv_weight_f16(w.to(dev))
    for with_res in (False, True):
        rd = res.permute(0, 2, 3, 1).contiguous().half().to(dev) if with_res else None
        ref = _conv_ref64(O, x, w, scale, bias, res if with_res else None, t, div)
        for odt in (torch.float32, torch.float16):
            tol = 2e-4 if odt == torch.float32 else 2e-3 * max(1.0, ref.abs().max().item())
            for tile in F16_TILES:
                got = ops.conv2d_bn_act_f16(xd, wd, scale.to(dev), bias.to(dev), rd, act=ops.ACT_RELU, out_dtype=odt, tile=tile,
                                            tsm_segments=t, tsm_div=div)
                assert got.dtype == odt
                err = _maxerr(got, ref)
                assert err < tol, (cin, div, t, with_res, odt, tile, err)
            plain = ops.conv2d_bn_act_f16(xd, wd, scale.to(dev), bias.to(dev), rd, act=ops.ACT_RELU, out_dtype=odt)
            assert not torch.equal(plain, got)


def test_conv_fused_shift_refusals(dev, ops):
    """What the engine cannot do is refused with the documented code, not computed."""
    def call(n, cin, seg, div, half=False):
        x = torch.zeros((n, 2, 2, cin), device=dev)
        w = torch.zeros((8, 1, 1, cin), device=dev)
        if half:
            return ops.conv2d_bn_act_f16(x.half(), w.half(), tsm_segments=seg, tsm_div=div)
        return ops.conv2d_bn_act(x, w, tsm_segments=seg, tsm_div=div)
    for cin, div in ((64, 3), (24, 8), (96, 16), (64, 32)):           # fold 21, 3, 6, 2
        with pytest.raises(L.AdafError, match=E_LAYOUT):
            call(8, cin, 4, div)
    with pytest.raises(L.AdafError, match=E_BADARG):
        call(9, 64, 4, 8)                                             # n % T != 0
    for div in (0, -1):
        with pytest.raises(L.AdafError, match=E_BADARG):
            call(8, 64, 4, div)
    for cin, div in ((64, 16), (96, 8)):                              # fp16 operands: fold 4, 12 are not whole 16-byte chunks
        with pytest.raises(L.AdafError, match=E_LAYOUT):
            call(8, cin, 4, div, half=True)
    assert call(8, 64, 4, 16).shape == (8, 2, 2, 8) and call(8, 64, 4, 8, half=True).shape == (8, 2, 2, 8)


# ------------------------------------------------------------------------------------------------ 3. ResNet-50 trunk
_NETS = {}


def _trunk(dev, math="f32"):
    if math not in _NETS:
        from adafocus_amd.resnet import resnet50
        net = resnet50(num_classes=200).eval()
        sd = synth_sd("ACT", 1007, "focuser.net.", keep_prefix=False)
        net.load_state_dict(sd, strict=True)
        net.set_math(math)
        _NETS[math] = (net.to(dev), sd)
    net, sd = _NETS[math]
    net.tsm_segments, net.tsm_div, net.tsm_place = 0, 8, "blockres"
    net.set_fusion(True)
    return net, sd


def _patches(n, p, seed):
    x = rnd((n, 3, p, p), seed)
    x4 = torch.zeros((n, p, p, 4))
    x4[..., :3] = x.permute(0, 2, 3, 1)
    return x, x4


def _oracle_trunk(O, sd, x, t, div, place="blockres"):
    with torch.no_grad():
        r32 = O.resnet50_trunk(sd, "", x, t, div, shift_place=place).flatten(1)
        r64 = O.resnet50_trunk(_f64(sd), "", x.double(), t, div, shift_place=place).flatten(1)
    return r32, r64


# (shift_div, T): 8 is the calibration column
TRUNK_CELLS = [(d, t) for d in (2, 4, 16) for t in (3, 8, 12)] + [(4, 5), (4, 7)] + [(8, 8), (8, 12)]
# >= 128 images at 32^2 / 48^2 (an 8 x 8 / 12 x 12 stage-1 map): position-major tile groups of 128 (T = 8), 126 (T = 3, 7), 125 (T = 5), 120 (T = 12)
LARGE = {3: [(32, 252)], 5: [(32, 250)], 7: [(48, 252)], 8: [(32, 256)], 12: [(32, 240), (48, 360)]}


def _trunk_plans(net, x4d, t, div, clip_rows):
    """Features under every plan (torch.equal among them) + the profile of the fused plan; returns (features, tile ids)."""
    net.tsm_segments, net.tsm_div = t, div
    with torch.no_grad():
        net.set_fusion(False)
        ref = net.features_nhwc4(x4d).clone()
        net.set_fusion(2)
        got2 = net.features_nhwc4(x4d).clone()
        prof = net._sync().profile(x4d, tsm_segments=t, tsm_div=div)
        with L.option("tsm_lean", 0):
            sel2 = net.features_nhwc4(x4d).clone()
        net.set_fusion(True)
        got1 = net.features_nhwc4(x4d).clone()
        with L.option("tsm_lean", 0):
            sel1 = net.features_nhwc4(x4d).clone()
        # a clip's features do not depend on the other clips of its batch
        alone = net.features_nhwc4(x4d[clip_rows:].contiguous()).clone()
        net.tsm_segments = 0
        plain = net.features_nhwc4(x4d).clone()
    assert torch.isfinite(ref).all()
    assert torch.equal(got2, ref), "set_fusion(2) != set_fusion(False)"
    assert torch.equal(got1, ref), "set_fusion(True) != set_fusion(False)"
    assert torch.equal(sel2, ref) and torch.equal(sel1, ref), "tsm_lean 0 != 1"
    assert torch.equal(alone, ref[clip_rows:]), "clip independence"
    assert not torch.equal(plain, ref)
    return ref, [e["tile"] for e in prof]


@pytest.mark.parametrize("div,t", TRUNK_CELLS)
def test_trunk_few_images(dev, O, div, t):
    """Two clips at 64^2 (T = 12: 72^2): row-major tiles everywhere, no fused tail with a shifted conv1."""
    net, sd = _trunk(dev)
    p = 72 if t == 12 else 64
    x, x4 = _patches(2 * t, p, 3000 + 16 * div + t)
    got, tiles = _trunk_plans(net, x4.to(dev), t, div, t)
    assert 92 not in tiles
    r32, r64 = _oracle_trunk(O, sd, x, t, div)
    _bounded("sec3 few-images div=%d T=%d n=%d p=%d" % (div, t, 2 * t, p), got, r32, r64)


@pytest.mark.parametrize("div,t,p,n", [(d, t, p, n) for d, t in TRUNK_CELLS for p, n in LARGE[t]])
def test_trunk_position_major_groups(dev, O, div, t, p, n):
    """>= 128 images: the fused stage-1 tail carries the shifted next conv1 when whole clips fill its tile groups AND the fold is whole
    32-channel passes (256 / shift_div: 4, 2, 1 passes per fold at 2, 4, 8 -- at 2 no unshifted pass is left; 16 gives fold 16: the tail
    runs without the next conv1).  Tile groups of fewer than 128 images leave idle rows (T = 3, 5, 7, 12)."""
    net, sd = _trunk(dev)
    x, x4 = _patches(n, p, 3100 + 16 * div + t + n)
    got, tiles = _trunk_plans(net, x4.to(dev), t, div, t)
    gs = (128 // t) * t
    groups = (n + gs - 1) // gs
    rides = n >= 128 and groups * 128 * 100 <= n * (106 if gs == 128 else 108)
    assert rides                                    # (by construction of LARGE)
    assert sum(e == 92 for e in tiles) == (3 if (256 // div) % 32 == 0 else 0), tiles[:8]
    r32, r64 = _oracle_trunk(O, sd, x, t, div)
    _bounded("sec3 position-major div=%d T=%d n=%d p=%d" % (div, t, n, p), got, r32, r64)


@pytest.mark.parametrize("t,p,n", [(8, 64, 16), (12, 32, 240)])
def test_trunk_block_placement(dev, O, t, p, n):
    """shift_place = 'block' at shift_div = 4: the materialised map in front of every Bottleneck."""
    net, sd = _trunk(dev)
    x, x4 = _patches(n, p, 3200 + t)
    net.tsm_segments, net.tsm_div, net.tsm_place = t, 4, "block"
    x4d = x4.to(dev)
    with torch.no_grad():
        got = net.features_nhwc4(x4d).clone()
        net.set_fusion(False)
        assert torch.equal(net.features_nhwc4(x4d), got)
        net.set_fusion(True)
        assert torch.equal(net.features_nhwc4(x4d[t:].contiguous()), got[t:])
        net.tsm_place = "blockres"
        other = net.features_nhwc4(x4d).clone()
    assert not torch.equal(other, got)
    r32, r64 = _oracle_trunk(O, sd, x, t, 4, place="block")
    _bounded("sec3 block placement div=4 T=%d n=%d p=%d" % (t, n, p), got, r32, r64)


@pytest.mark.parametrize("div,t,p,n", [(2, 8, 64, 16), (4, 8, 64, 16), (2, 12, 32, 240), (4, 3, 32, 252), (8, 8, 64, 16), (8, 8, 32, 256)])
def test_trunk_split_bf16(dev, O, div, t, p, n):
    """set_math("split_bf16"): fp32 operands as three bf16 parts (stage 1 stays on the fp32 pipe, fused tail included)."""
    net, sd = _trunk(dev, "split_bf16")
    x, x4 = _patches(n, p, 3300 + 16 * div + t + n)
    net.tsm_segments, net.tsm_div = t, div
    x4d = x4.to(dev)
    with torch.no_grad():
        got = net.features_nhwc4(x4d).clone()
        net.set_fusion(False)
        assert torch.equal(net.features_nhwc4(x4d), got)
        net.set_fusion(True)
        assert torch.equal(net.features_nhwc4(x4d[t:].contiguous()), got[t:])
    r32, r64 = _oracle_trunk(O, sd, x, t, div)
    _bounded("sec3 split_bf16 div=%d T=%d n=%d p=%d" % (div, t, n, p), got, r32, r64)


@pytest.mark.parametrize("div,t,place", [(2, 8, "blockres"), (4, 8, "blockres"), (4, 12, "blockres"), (2, 3, "blockres"),
                                         (2, 8, "block"), (4, 8, "block"), (16, 8, "block")])
def test_trunk_fp16(dev, div, t, place):
    """The fp16 trunk against test_f16_trunk.py's contract model under its own calibrated bound; 'block' runs the fp16 move (16-byte
    chunks; at shift_div = 16 layer1.0's fold of 4 takes its one-channel form)."""
    from tests.test_f16_trunk import _contract_bound, _feat, _rel_rms, contract_trunk
    net, sd = _trunk(dev, "f16")
    net.tsm_segments, net.tsm_div, net.tsm_place = t, div, place
    x = rnd((2 * t, 3, 64, 64), 3400 + 16 * div + t)
    got = _feat(net, x, dev)
    with torch.no_grad():
        ref = contract_trunk(sd, x, tsm=t, div=div, place=place)
    err, bound = _rel_rms(got, ref), _contract_bound(sd, x, ref, tsm=t, div=div, place=place)
    print("fp16 trunk div=%d T=%d %s: rel rms %.2e (bound %.2e)" % (div, t, place, err, bound))
    assert torch.isfinite(got).all() and err <= bound, (div, t, place, err, bound)
    assert torch.equal(_feat(net, x[t:], dev), got[t:])
    net.tsm_segments = 0
    assert not torch.equal(_feat(net, x, dev), got)


# ------------------------------------------------------------------------------------------------ 4. glancer (MobileNetV2 with TSM)
_GLANCERS = {}


def _glancer(dev, div, t):
    if (div, t) not in _GLANCERS:
        from adafocus_amd.gfv_net_sth import Glancer
        from tests.test_state_dict_compat import sth_args
        a = sth_args()
        a.shift_div, a.num_segments_glancer = div, t
        gl = Glancer(a).eval()
        sd = synth_sd("STH", 78, "glancer.", keep_prefix=False)
        gl.load_state_dict(sd, strict=True)
        _GLANCERS[(div, t)] = (gl.to(dev), sd)
    gl, sd = _GLANCERS[(div, t)]
    gl.net._engine.fusion = True
    return gl, sd


@pytest.mark.parametrize("size", [224, 128, 64])
@pytest.mark.parametrize("t", [2, 8])
@pytest.mark.parametrize("div", [2, 4, 8, 16])
def test_glancer_plans_and_oracle(dev, O, div, t, size):
    """16 frames.  224^2: strip kernels (the 64- / 96-channel blocks' expand -> depthwise strips shift inside their pixel loads when both
    folds lie in the first quarter of the channels, else read a materialised copy); 128^2 / 64^2: tile kernels.  Strips == tiles ==
    unfused, bit for bit; then the float64 oracle."""
    gl, sd = _glancer(dev, div, t)
    x = rnd((16, 3, size, size), 4000 + size)
    xd = x.to(dev)
    outs = []
    with torch.no_grad():
        for strip, fusion in ((1, True), (0, True), (0, False)):
            with L.option("mb_strip", strip):
                gl.net._engine.fusion = fusion
                fm, logit = gl(xd)
                outs.append((fm.clone(), logit.clone()))
        gl.net._engine.fusion = True
        r32 = O.glancer_sth(sd, "net.", x, t, div)
        r64 = O.glancer_sth(_f64(sd), "net.", x.double(), t, div)
    tag = "sec4 glancer div=%d T=%d size=%d" % (div, t, size)
    wrong = []          # every finding of the cell in one message
    for i, (fm, logit) in enumerate(outs[1:]):
        if not (torch.equal(fm, outs[0][0]) and torch.equal(logit, outs[0][1])):
            wrong.append("%s: %s differs from the strip plan, map by %.3e, logits by %.3e" % (
                tag, ("the tile plan", "the unfused plan")[i], _maxerr(fm, outs[0][0]), _maxerr(logit, outs[0][1])))
    wrong.append(_ratio(tag + " map", outs[0][0], r32[0], r64[0]))
    wrong.append(_ratio(tag + " logits", outs[0][1], r32[1], r64[1]))
    wrong = [m for m in wrong if m]
    assert not wrong, "; ".join(wrong)


@pytest.mark.parametrize("t,chunk", [(8, 8), (2, 6)])
@pytest.mark.parametrize("div", [2, 4, 8, 16])
def test_glancer_chunks(dev, div, t, chunk):
    """16 frames of 224^2 in chunks of one clip of 8 (two chunks) and of three clips of 2 (6 + 6 + 4): whole clips per chunk, the same bits."""
    gl, _ = _glancer(dev, div, t)
    xd = rnd((16, 3, 224, 224), 4300 + t).to(dev)
    with torch.no_grad():
        fm, logit = [v.clone() for v in gl(xd)]
        with L.option("mbv2_chunk", chunk):
            fm_c, logit_c = [v.clone() for v in gl(xd)]
    assert torch.isfinite(fm).all() and fm.abs().max().item() > 0.1
    assert torch.equal(fm_c, fm) and torch.equal(logit_c, logit), (div, t, chunk, _maxerr(fm_c, fm))


def test_sth_model_shift_div_4(dev, O):
    """GFV (Something-Something) built with args.shift_div = 4: glance + action_stage2 with a forced action against sth_forward."""
    from adafocus_amd import synth
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.gpu, a.shift_div = 0, 4
    m = GFV(a).eval()
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])      # STH/evaluate.py:83
    m.load_state_dict(synth_sd("STH", 1007), strict=True)
    pol = {k[len("policy."):]: v for k, v in synth_sd("STH_POLICY", 1007).items()}
    m.focuser.policy.policy_old.load_state_dict(pol)
    m.focuser.policy.policy.load_state_dict(pol)
    m.focuser.policy.policy_old.eval()
    m.focuser.policy.policy.eval()
    m = m.to(dev)
    gl = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=3))
    fo = torch.from_numpy(synth.synth_frames(2, 8, 224, seed=4)).view(2, 8, 3, 224, 224)
    forced = torch.tensor([[0.25, 0.75], [0.6, 0.1]])
    with torch.no_grad():
        fm, glog = m.glance(gl.to(dev))
        pred, _, patch = m.action_stage2(fo.to(dev), fm, glog, 0, a, prev_local_patch=None, training=False, forced_action=forced.to(dev))
    sd = synth_sd("STH", 1007)
    sd.update(synth_sd("STH_POLICY", 1007))
    sd = O.canonical_resnet_keys(sd, "focuser.net.base_model.")
    with torch.no_grad():
        r32, p32, _ = O.sth_forward(sd, gl.view(2, 24, 224, 224), fo, 128, 8, 8, shift_div=4, forced_action=forced)
        r64, _, _ = O.sth_forward(_f64(sd), gl.view(2, 24, 224, 224).double(), fo.double(), 128, 8, 8, shift_div=4, forced_action=forced.double())
        r8, _, _ = O.sth_forward(sd, gl.view(2, 24, 224, 224), fo, 128, 8, 8, shift_div=8, forced_action=forced)
    assert torch.equal(patch.cpu(), p32)
    assert _maxerr(r8, r64) > 1e-2                  # (shift_div = 4 is another network than 8)
    _bounded("sec4 GFV shift_div=4 logits", pred, r32, r64)
