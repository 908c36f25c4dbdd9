"""The MobileNetV2 glancer at every family of frame sizes its launch plan distinguishes, against the float64 oracle.

`glance_size` is a user setting and the launch form of each block is picked from the frame size alone (csrc/mobilenetv2.hip block_form:
strip kernels of mbstrip.hip where a map is an even multiple of 14, wave-private tiles of mbconv.hip from 28^2 up, else the conv engine +
the depthwise kernel).  The rest of the suite reaches a strip kernel at 224^2 only, where every strip count, segment and wave block is
full.  The sizes here are the smallest that reach what 224 does not:

  32   the 1 x 1 final map; nothing fused behind the stem (maps 16, 8, 4, 2, 1)
  56   stem strips with tiles_x = 2; the stride-2 whole-block strip with a ragged last segment (OH = 14 = 3 x 4 + 2)
  84   a strip stem (tiles_x = 3) feeds the TILE stride-2 expand -> depthwise kernel (42 -> 21, odd)
  112  mb_block_s_kernel<24> with a ragged last segment of 4 rows (28 = 3 x 8 + 4); b4's stride-2 strip, OH = 14
  113  odd frames: S != 2 * H1, the stem's last window sits on the right / bottom edge without padding; odd maps 57, 29, 15
  168  whole-block strips with a last segment of 2 rows (42 = 5 x 8 + 2), stride-2 strips with OH = 42 = 10 x 4 + 2, then the strip
       block b3 feeds the tile stride-2 kernel on 42 -> 21
  196  strip stem (tiles_x = 7) -> tile kernels on 98 -> 49 -> 25
  280  last segment of 6 rows (70 = 8 x 8 + 6), OH = 70 = 17 x 4 + 2, strip block -> tile stride-2 kernel on 70 -> 35, tile whole
       blocks on an odd 35^2 map
  448  every strip form at once with tiles_x = 16 / 8 / 4 / 2: the expand -> depthwise strips of b8 .. b13 and the stride-2 one of b14
       on 28^2 maps (two strips per frame), the temporal shift riding in their pixel loads (shift_div 8) or materialised (4)

The frame counts (3, 1 at 448; clips: 4, 2 at 448) leave the last block of four waves part empty in every strip launch.

Per case: (1) the plan adaf_mobilenetv2_block_forms reports -- the forward's own decision function -- is the one written out in PLAN
below, so a case cannot silently run another form than it is here for; (2) strips == tiles == expand->depthwise + project == separate
launches, torch.equal; (3) err(kernel, oracle64) <= F_BOUND * err(oracle32, oracle64), max abs, on the map and on the vector / logits:
test_shift_matrix_gpu's bound, imported, not re-calibrated (its docstring has the calibration); (4) shape, finiteness, liveness.
Every case prints its ratios (pytest -s); LABNOTES has the figures measured on an MI355X."""
import pytest
import torch

from adafocus_amd import _lib as L
from adafocus_amd.utils import nchw_to_nhwc4
from tests.helpers import rnd, synth_sd
from tests.test_shift_matrix_gpu import F_BOUND, _f64, _glancer as _sth_glancer, _ratio      # noqa: F401  (F_BOUND: the bound _ratio applies)

pytestmark = pytest.mark.gpu

U, X, W, SW, SX = 0, 1, 2, 3, 4          # unfused | tile expand->dw | tile whole block | strip whole block | strip expand->dw
NONE, IN_STRIP, IN_OPERAND, COPY = 0, 1, 2, 3      # the shift nibble
STRIDE2 = (1, 3)                          # entries of b2, b4: the stride-2 blocks that have a whole-block (strip) form


def _plan(stem, b2, b3, b4, b56, b7, b8_13, b14, b15_17):
    """17 entries: the stem + b1 pair (W tile / SW strip), then b2 .. b17."""
    return [stem, b2, b3, b4, b56, b56, b7] + [b8_13] * 6 + [b14] + [b15_17] * 3


# The default plan (fusion on, mb_strip 1) per frame size, read off the predicates adaf_mb_*_ok; maps = outputs of the stem, b2, b4, b7, b14.
PLAN = {
    32: _plan(W, U, U, U, U, U, U, U, U),            # maps 16, 8, 4, 2, 1
    56: _plan(SW, SW, U, U, U, U, U, U, U),          # 28, 14, 7, 4, 2
    84: _plan(SW, X, U, U, U, U, U, U, U),           # 42, 21, 11, 6, 3
    112: _plan(SW, SW, SW, SW, U, U, U, U, U),       # 56, 28, 14, 7, 4
    113: _plan(W, X, W, X, U, U, U, U, U),           # 57, 29, 15, 8, 4
    168: _plan(SW, SW, SW, X, U, U, U, U, U),        # 84, 42, 21, 11, 6
    196: _plan(SW, X, W, X, U, U, U, U, U),          # 98, 49, 25, 13, 7
    280: _plan(SW, SW, SW, X, W, X, U, U, U),        # 140, 70, 35, 18, 9
    448: _plan(SW, SW, SW, SW, SW, X, SX, SX, U),    # 224, 112, 56, 28, 14
}
SIZES = tuple(PLAN)

# Entries of the residual blocks that have an expand conv (the ones the Something-Something glancer shifts): b3, b5, b6, b8, b9, b10, b12, b13, b15, b16
RESIDUAL = (2, 4, 5, 7, 8, 9, 11, 12, 14, 15)
# ... and their shift treatment under the default plan, per (size, shift_div).  fold = channels / shift_div.  A fused tile or whole-block
# strip kernel reads a materialised copy; the expand -> depthwise strips shift in their loads when both folds lie in the first quarter of
# the channels (shift_div >= 8); an unfused expand conv shifts in its operand load when fold % 4 == 0 (b3 at 8: fold 3, a copy).
SHIFT = {
    (112, 8): {2: COPY},
    (168, 8): {2: COPY},
    (448, 8): {2: COPY, 4: COPY, 5: COPY, 7: IN_STRIP, 8: IN_STRIP, 9: IN_STRIP, 11: IN_STRIP, 12: IN_STRIP},
    (448, 4): {2: COPY, 4: COPY, 5: COPY, 7: COPY, 8: COPY, 9: COPY, 11: COPY, 12: COPY},
}           # (every residual entry not listed: IN_OPERAND)
STH_CASES = tuple(SHIFT)
STH_T = 2

PLANS = ((1, True), (0, True), (1, 9), (1, False))          # (mb_strip, fusion): the default first


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def O():
    from oracle import ref_model
    return ref_model


def _out_side(size):
    for _ in range(5):          # the stem and the four stride-2 blocks: 3 x 3 windows, pad 1, stride 2
        size = (size - 1) // 2 + 1
    return size


_ACT = {}


def _act_glancer(dev):
    if not _ACT:
        from adafocus_amd.mobilenet import mobilenet_v2
        sd = {k: v for k, v in synth_sd("ACT", 505, "glancer.net.", keep_prefix=False).items() if not k.startswith("classifier")}
        net = mobilenet_v2().eval()
        net.load_state_dict(sd, strict=False)            # the stand-alone net's 1000-way head is not on the features path
        _ACT["net"], _ACT["sd"] = net.to(dev), sd
    _ACT["net"]._engine.fusion = True
    return _ACT["net"], _ACT["sd"]


_ORACLE = {}        # (variant, size, T, div) -> ((map32, vec32), (map64, vec64)): computed once, read only


def _oracle(O, variant, size, t, div, sd, x):
    key = (variant, size, t, div)
    if key not in _ORACLE:
        with torch.no_grad():
            if variant == "act":
                _ORACLE[key] = (O.glancer_act(sd, "", x), O.glancer_act(_f64(sd), "", x.double()))
            else:
                _ORACLE[key] = (O.glancer_sth(sd, "net.", x, t, div), O.glancer_sth(_f64(sd), "net.", x.double(), t, div))
    return _ORACLE[key]


def _forms(engine, fusion, strip, size, t=0, div=8):
    """(form nibbles, shift nibbles) of the plan the forward takes under these options."""
    engine.fusion = fusion
    with L.option("mb_strip", strip):
        f = engine.sync().block_forms(size, t, div)
    engine.fusion = True
    assert len(f) == 17 and all(0 <= v < 64 for v in f), f
    return [v & 15 for v in f], [v >> 4 for v in f]


def _check_plans(engine, size, t=0, div=8):
    """Step 1.  The default plan is PLAN[size] (and SHIFT); the other option settings give what the predicates say they give."""
    want = PLAN[size]
    form, shift = _forms(engine, True, 1, size, t, div)
    assert form == want, "size %d: the forward's plan %s is not the intended %s" % (size, form, want)
    if t:
        want_shift = [SHIFT[(size, div)].get(i, IN_OPERAND) if i in RESIDUAL else NONE for i in range(17)]
        assert shift == want_shift, (size, div, shift, want_shift)
    else:
        assert shift == [NONE] * 17, shift
    # mb_strip 0: no strip form.  A strip stem / stride-1 strip block is the tile kernel; the stride-2 whole block exists as a strip only
    # (tile expand -> depthwise + project instead); the expand -> depthwise strips have no tile form (separate launches).
    no_strip = [{SW: X if i in STRIDE2 else W, SX: U}.get(v, v) for i, v in enumerate(want)]
    form, _ = _forms(engine, True, 0, size, t, div)
    assert not set(form) & {SW, SX} and form == no_strip, (size, form, no_strip)
    # fusion 9 (bit 3: no whole-block kernel, no expand -> depthwise strips): tile expand -> depthwise wherever a block is fused by default
    no_whole = [want[0]] + [X if v in (X, W, SW) else U for v in want[1:]]
    form, _ = _forms(engine, 9, 1, size, t, div)
    assert not set(form[1:]) & {W, SW, SX} and form == no_whole, (size, form, no_whole)
    # fusion off: separate launches, the shift in the operand load or (fold % 4 != 0) materialised
    form, shift = _forms(engine, False, 1, size, t, div)
    assert form == [U] * 17, (size, form)
    if t:
        c = (24, 32, 32, 64, 64, 64, 96, 96, 160, 160)
        assert shift == [(IN_OPERAND if (c[RESIDUAL.index(i)] // div) % 4 == 0 else COPY) if i in RESIDUAL else NONE for i in range(17)], (size, div, shift)


def _compare(tag, outs, ref32, ref64, n, size):
    """Steps 2 - 4 on outs[plan] = (map NCHW, vector / logits), outs[0] the default plan.  -> the list of findings."""
    wrong = []
    for (strip, fusion), (fm, vec) in list(zip(PLANS, outs))[1:]:
        if not (torch.equal(fm, outs[0][0]) and torch.equal(vec, outs[0][1])):
            wrong.append("%s: mb_strip %d fusion %s differs from the default plan, map by %.3e, vector by %.3e" % (
                tag, strip, fusion, (fm - outs[0][0]).abs().max().item(), (vec - outs[0][1]).abs().max().item()))
    fm, vec = outs[0]
    wrong.append(_ratio(tag + " map", fm, ref32[0], ref64[0]))
    wrong.append(_ratio(tag + " vector", vec, ref32[1], ref64[1]))
    fs = _out_side(size)
    if tuple(fm.shape) != (n, 1280, fs, fs):
        wrong.append("%s: map shape %s, expected side %d" % (tag, tuple(fm.shape), fs))
    if not (torch.isfinite(fm).all() and torch.isfinite(vec).all()):
        wrong.append("%s: not finite" % tag)
    if not fm.abs().max().item() > 0.1:
        wrong.append("%s: dead map, max |.| = %.3e" % (tag, fm.abs().max().item()))
    return [m for m in wrong if m]


@pytest.mark.parametrize("size", SIZES)
def test_act_glancer_size(dev, O, size):
    """ACT glancer (mobilenet_v2, seed-505 weights) through features_from_nhwc4, 3 frames (1 at 448^2)."""
    net, sd = _act_glancer(dev)
    n = 1 if size == 448 else 3
    _check_plans(net._engine, size)
    x = rnd((n, 3, size, size), 7000 + size)
    x4 = nchw_to_nhwc4(x.to(dev))
    outs = []
    with torch.no_grad():
        for strip, fusion in PLANS:
            with L.option("mb_strip", strip):
                net._engine.fusion = fusion
                fm, fv = net.features_from_nhwc4(x4)
                outs.append((fm.permute(0, 3, 1, 2).clone(), fv.clone()))
        net._engine.fusion = True
    r32, r64 = _oracle(O, "act", size, 0, 0, sd, x)
    wrong = _compare("glancer sizes ACT size=%d n=%d" % (size, n), outs, r32, r64, n, size)
    assert not wrong, "; ".join(wrong)


@pytest.mark.parametrize("size,div", STH_CASES)
def test_sth_glancer_size(dev, O, size, div):
    """Something-Something glancer (TSM on the residual blocks' expand convs), clips of 2 frames, 4 frames (2 at 448^2): the shift
    materialised in front of whole-block strips (b3's fold of 3 at 112 / 168), riding in the two-strip expand -> depthwise loads (448,
    shift_div 8) and materialised in front of them (448, shift_div 4)."""
    gl, sd = _sth_glancer(dev, div, STH_T)
    eng = gl.net._engine
    n = 2 if size == 448 else 4
    _check_plans(eng, size, STH_T, div)
    x = rnd((n, 3, size, size), 7500 + size)
    xd = x.to(dev)
    outs = []
    with torch.no_grad():
        for strip, fusion in PLANS:
            with L.option("mb_strip", strip):
                eng.fusion = fusion
                fm, logit = gl(xd)
                outs.append((fm.clone(), logit.clone()))
        eng.fusion = True
        unshifted = eng.features(nchw_to_nhwc4(xd), 0, div)[0].permute(0, 3, 1, 2)
    r32, r64 = _oracle(O, "sth", size, STH_T, div, sd, x)
    wrong = _compare("glancer sizes STH size=%d div=%d T=%d n=%d" % (size, div, STH_T, n), outs, r32, r64, n, size)
    if torch.equal(unshifted, outs[0][0]):
        wrong.append("size %d div %d: the temporal shift changes nothing" % (size, div))
    assert not wrong, "; ".join(wrong)
