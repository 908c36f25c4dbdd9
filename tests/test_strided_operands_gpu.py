"""Strided and unaligned operands of the C ABI (include/adafocus.h) behind guard bands.

The product never hands the kernels a dense tensor where it matters most (the trunk writes its 2048 features into the tail of the
(B*T, 3328) GRU input, the GRU reads that matrix through ldx, the policy head has 50 columns), yet every other test passes dense,
exactly sized, 16-byte aligned tensors.  Here every operand is a row-strided view inside a NaN-canary allocation (tests/strided.py):
  - guards: no element outside an output's rows x cols payload may change (lead, the ld - cols gap of every row, trail);
  - no gap read: input and residual gaps hold the NaN canary, the output payload must be finite;
  - float64 reference on the CPU, with the bound the existing dense test of the op uses;
  - bit identity with the dense call of the same kernel: a stride changes addresses, not arithmetic.
Every allocation carries at least one full row of guard on either side, so a store that overruns by less than a row is caught inside
memory the test owns."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from adafocus_amd import _lib as L
from adafocus_amd._lib import AdafError
from tests import strided as S
from tests import test_hip_parity as _P
from tests import test_hip_parity_r2 as _P2
from tests.helpers import rnd

pytestmark = pytest.mark.gpu

# the tile codes the dense tests enumerate (0 = automatic is among them), plus the small-batch form
F32_TILES = tuple(_P.test_conv_engine_vs_oracle.pytestmark[0].args[1]) + (95,)
F16_TILES = tuple(_P2.test_conv_f16_operands_vs_fp32_reference.pytestmark[0].args[1])
assert 0 in F32_TILES and 0 in F16_TILES and len(F32_TILES) >= 34 and len(F16_TILES) >= 6

FAMILIES = ("register-staged", "split-6", "split-9", "7x", "fp16", "latency")     # each must accept at least one strided case


def _family(tile):
    if tile == 0:
        return "automatic"
    if tile <= 5:
        return "register-staged"
    if tile < 40:
        return "direct-to-LDS"
    if tile < 50:
        return "split-6"
    if tile < 60:
        return "split-9"
    if tile < 80:
        return "7x"
    return "fp16" if tile < 90 else "latency"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------------------------ conv engine, fp32
# ldx / ldo / ldr: pixel strides in floats, 0 = dense.  oo / orr: extra floats in front of out / residual (1..3: 4-byte but not 16-byte
# aligned).  col: column offset of `out` inside its row (the trunk's features start at column 1280 of the GRU input).
Case = collections.namedtuple("Case", "name n h w cin cout k stride pad act res tsm ldx ldo ldr oo orr col",
                              defaults=(0, 0, 0, 0, 0, 0))
R, N6, SG, SW = S.ACT_RELU, S.ACT_RELU6, S.ACT_SIGMOID, S.ACT_SWISH
CASES = [
    # ---- each stride alone, then all three, unrelated values
    Case("ldx_alone", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, ldx=76),
    Case("ldo_alone", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, ldo=84),
    Case("ldr_alone", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, ldr=68),
    Case("all_three", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, ldx=76, ldo=84, ldr=68),
    Case("interior_tiles", 4, 12, 10, 64, 256, 1, 1, 0, R, True, 0, ldx=76, ldo=276, ldr=260),      # whole 128 x 128 tiles: the lean epilogue
    Case("trunk_tail_2048_into_3328", 5, 3, 3, 512, 2048, 1, 1, 0, R, True, 0, ldo=3328, ldr=2052, col=1280),   # the production pattern
    # ---- strides that are not multiples of 4 with cout % 4 == 0: the scalar epilogue
    Case("ldo_ldr_not_mult4", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, ldx=76, ldo=70, ldr=66),
    Case("ldo_not_mult4", 3, 5, 7, 32, 128, 1, 1, 0, N6, False, 0, ldo=129),
    Case("ldr_not_mult4", 3, 5, 7, 32, 128, 1, 1, 0, 0, True, 0, ldr=131),
    # ---- out / residual 4-byte but not 16-byte aligned
    Case("out_off1", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, oo=1),
    Case("out_off2_res_off3", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, oo=2, orr=3),
    Case("out_off3_res_off1_strided", 4, 6, 5, 64, 64, 1, 1, 0, R, True, 0, ldx=76, ldo=84, ldr=68, oo=3, orr=1),
    Case("res_off2", 4, 6, 5, 64, 64, 1, 1, 0, 0, True, 0, orr=2),
    # ---- column tails: cout 50 (policy head), 174 (Something-Something classes), 200, dense and strided
    Case("cout50_dense", 37, 1, 1, 256, 50, 1, 1, 0, 0, False, 0),
    Case("cout50_strided", 37, 1, 1, 256, 50, 1, 1, 0, 0, True, 0, ldx=268, ldo=70, ldr=54),
    Case("cout174_dense", 9, 2, 3, 128, 174, 1, 1, 0, R, False, 0),
    Case("cout174_strided", 9, 2, 3, 128, 174, 1, 1, 0, R, True, 0, ldx=140, ldo=194, ldr=178),
    Case("cout200_dense", 37, 1, 1, 256, 200, 1, 1, 0, 0, False, 0),
    Case("cout200_strided", 37, 1, 1, 256, 200, 1, 1, 0, 0, True, 0, ldx=268, ldo=220, ldr=204),
    # ---- a row tail and a column tail against the tile in the same case: the masked edge of a tile meets a gap (M = 45, cout = 200)
    Case("m45_cout200_3x3", 5, 3, 3, 64, 200, 3, 1, 1, R, True, 0, ldx=76, ldo=220, ldr=204),
    Case("m45_cout200_scalar", 5, 3, 3, 64, 200, 1, 1, 0, R, True, 0, ldx=76, ldo=221, ldr=203, oo=1),
    # ---- non-square maps, both ways, k = 1, 3, 5, 7, stride 2, pad 0 and k // 2, 1 x W and H x 1
    Case("k1_5x7", 3, 5, 7, 32, 40, 1, 1, 0, SW, True, 0, ldx=44, ldo=60, ldr=44),
    Case("k1_7x4_s2", 3, 7, 4, 32, 40, 1, 2, 0, SG, False, 0, ldx=44, ldo=60),
    Case("k3_6x9_pad1", 2, 6, 9, 32, 48, 3, 1, 1, R, True, 0, ldx=44, ldo=68, ldr=52),
    Case("k3_9x6_s2_pad0", 2, 9, 6, 64, 48, 3, 2, 0, R, True, 0, ldx=76, ldo=68, ldr=52),
    Case("k3_7x10_s2_pad1", 2, 7, 10, 64, 96, 3, 2, 1, N6, False, 0, ldx=76, ldo=116),
    Case("k5_8x5_pad2", 2, 8, 5, 8, 24, 5, 1, 2, R, True, 0, ldx=20, ldo=44, ldr=28),
    Case("k5_5x9_s2_pad0", 2, 5, 9, 8, 24, 5, 2, 0, SW, False, 0, ldx=20, ldo=44),
    Case("k7_9x12_s2_pad3", 2, 9, 12, 4, 64, 7, 2, 3, R, False, 0, ldx=16, ldo=84),               # the stem's shape: K = 196
    Case("k7_12x8_pad0", 2, 12, 8, 4, 64, 7, 1, 0, 0, True, 0, ldx=16, ldo=84, ldr=68),
    Case("k3_1xW", 3, 1, 9, 32, 32, 3, 1, 1, R, True, 0, ldx=44, ldo=52, ldr=36),
    Case("k3_Hx1", 3, 9, 1, 32, 32, 3, 1, 1, R, True, 0, ldx=44, ldo=52, ldr=36),
    Case("k1_1xW", 3, 1, 9, 32, 32, 1, 1, 0, 0, False, 0, ldx=44, ldo=52),
    Case("k1_Hx1_s2", 3, 9, 1, 32, 32, 1, 2, 0, 0, False, 0, ldx=44, ldo=52),
    # ---- enough images for position-major tiles (130 >= 128 rows of the same pixel), padding taps to skip, non-square
    Case("pos_major_3x2", 130, 3, 2, 32, 24, 3, 1, 1, R, True, 0, ldx=44, ldo=44, ldr=28),
    Case("pos_major_2x3_cout200", 130, 2, 3, 32, 200, 3, 1, 1, R, False, 0, ldx=36, ldo=221, oo=1),
    # ---- the fused temporal shift reads the neighbouring frames' rows through the stride
    Case("tsm4", 8, 3, 2, 64, 64, 1, 1, 0, R, False, 4, ldx=76, ldo=84),
    Case("tsm8_res", 8, 2, 3, 256, 128, 1, 1, 0, R, True, 8, ldx=268, ldo=148, ldr=132),             # fold = 32: the lean shifted K loop
    Case("tsm12", 24, 2, 2, 64, 40, 1, 1, 0, R, True, 12, ldx=72, ldo=60, ldr=44),
    Case("tsm12_big", 24, 3, 3, 256, 128, 1, 1, 0, R, False, 12, ldx=260, ldo=132),
]
assert len({c.name for c in CASES}) == len(CASES)


def _strided(c):
    return bool(c.ldx or c.ldo or c.ldr or c.oo or c.orr or c.col)


def _dma_shape(c):
    """Shapes the direct-to-LDS kernels take (adaf_conv_glds_ok); the engine runs a forced 2x / 3x / 4x / 5x / 7x tile of any other shape on the
    register-staged kernel instead, so only these count as that family having run."""
    if c.k == 1 and c.stride == 1 and c.pad == 0:
        return True
    return c.cin % 32 == 0 and c.k * c.k <= 32


def _latency_takes(c):
    """The small-batch form's documented limits (include/adafocus.h tile 95, tests/test_hip_parity_r3.py): cin % 64 == 0, no temporal shift,
    at most 32 filter taps, no sigmoid / swish."""
    return c.cin % 64 == 0 and c.tsm == 0 and c.k * c.k <= 32 and c.act in (S.ACT_NONE, S.ACT_RELU, S.ACT_RELU6)


def _conv_data(c, idx, dev, half=False):
    """Operands scaled as tests/test_hip_parity.py _conv_case scales them (sqrt(2 / K) weights): CONV_TOL keeps its meaning."""
    g = np.random.Generator(np.random.PCG64([1000 + idx, 17]))
    kk = c.cin * c.k * c.k
    x = torch.from_numpy(g.standard_normal((c.n, c.h, c.w, c.cin), dtype=np.float32))
    w = torch.from_numpy(g.standard_normal((c.cout, c.k, c.k, c.cin), dtype=np.float32) * np.float32(np.sqrt((1.0 if half else 2.0) / kk)))
    sc = torch.from_numpy(g.uniform(0.5, 1.5, c.cout).astype(np.float32))
    bi = torch.from_numpy(g.normal(0, 0.1, c.cout).astype(np.float32))
    oh, ow = (c.h + 2 * c.pad - c.k) // c.stride + 1, (c.w + 2 * c.pad - c.k) // c.stride + 1
    res = torch.from_numpy(g.standard_normal((c.n, oh, ow, c.cout), dtype=np.float32)) if c.res else None
    return x, w, sc, bi, res, oh, ow


def _place(dense, ld, off, dev, dtype=torch.float32):
    """A guarded copy of `dense` (rows..., cols) with row stride ld (0 = dense) starting `off` elements past an aligned lead."""
    cols = dense.shape[-1]
    ld = ld or cols
    buf, view = S.guarded(dense.shape[:-1], cols, ld, S.lead_for(ld, off), ld + 8, dtype, dev)
    S.fill(view, dense.to(dev))
    return buf, view


def _empty(rows_shape, cols, ld, off, dev, dtype=torch.float32):
    ld = ld or cols
    return S.guarded(rows_shape, cols, ld, S.lead_for(ld, off), ld + 8, dtype, dev)


_SEEN = {}            # case name -> {(tile, pos_major): "ok" | "refused"}


def _run_conv_case(idx, dev, ops):
    c = CASES[idx]
    if c.name in _SEEN:
        return _SEEN[c.name], []
    x, w, sc, bi, res, oh, ow = _conv_data(c, idx, dev)
    kw = dict(stride=c.stride, pad=c.pad, act=c.act, tsm_segments=c.tsm, tsm_div=8)
    ref = S.conv_ref64(x, w, sc, bi, res, **kw)
    wd, scd, bid = w.to(dev), sc.to(dev), bi.to(dev)
    # inputs: one dense and one strided copy; their guards are checked at the end (nothing may write an input)
    xb_d, xv_d = _place(x, 0, 0, dev)
    xb_s, xv_s = _place(x, c.ldx, 0, dev)
    rb_d, rv_d = _place(res, 0, 0, dev) if c.res else (None, None)
    rb_s, rv_s = _place(res, c.ldr, c.orr, dev) if c.res else (None, None)
    snap = [b.view(torch.int32).clone() for b in (xb_d, xb_s, rb_d, rb_s) if b is not None]
    seen, fails = {}, []

    def one(kind, tile, strided):
        ob, ov = _empty((c.n, oh, ow), c.cout, c.ldo if strided else 0, (c.col + c.oo) if strided else 0, dev)
        S.conv_call(kind, xv_s if strided else xv_d, wd, scd, bid, rv_s if strided else rv_d, ov, tile=tile, **kw)
        return ob, ov

    # the naive kernel takes the same strides (it is the fuzz's reference)
    nb, nv = one("naive", 0, True)
    S.assert_guards_intact(nb, nv, "%s naive out" % c.name)
    err = (S.payload(nv).cpu().double() - ref).abs().max().item()
    assert err < S.CONV_TOL, (c.name, "naive", err)
    try:
        for pm in ((True, False) if c.k > 1 else (True,)):
            ops.set_conv_pos_major(pm, dev)
            for tile in F32_TILES:
                tag = "%s tile %d pos_major %d" % (c.name, tile, pm)
                try:
                    db, dv = one("engine", tile, False)
                except AdafError as e:
                    seen[(tile, pm)] = "refused"
                    if tile != 95 or _latency_takes(c):
                        fails.append("%s: refused against the documented rules: %s" % (tag, e))
                    continue
                if tile == 95 and not _latency_takes(c):
                    fails.append("%s: the latency form took a case beyond its documented limits" % tag)
                sb, sv = one("engine", tile, True)          # a stride is never a reason to refuse what the dense call took
                seen[(tile, pm)] = "ok"
                try:
                    S.assert_guards_intact(db, dv, tag + " dense out")
                    S.assert_guards_intact(sb, sv, tag + " strided out")
                    dense, got = S.payload(dv), S.payload(sv)
                    assert bool(torch.isfinite(got).all()), "%s: %d non-finite outputs (a gap was read, or an element was not written), first at %s" % (
                        tag, int((~torch.isfinite(got)).sum()), tuple(torch.nonzero(~torch.isfinite(got))[0].tolist()))
                    assert bool(torch.isfinite(dense).all()), "%s: non-finite outputs of the dense call" % tag
                    err = (got.cpu().double() - ref).abs().max().item()
                    assert err < S.CONV_TOL, "%s: max |err| vs float64 %.3e >= %.1e" % (tag, err, S.CONV_TOL)
                    if not torch.equal(got, dense):
                        d = torch.nonzero(got != dense)
                        i0 = tuple(d[0].tolist())
                        raise AssertionError("%s: strided result differs from the dense call in %d elements, first at %s: %r vs %r" % (
                            tag, d.shape[0], i0, got[i0].item(), dense[i0].item()))
                except AssertionError as e:
                    fails.append(str(e))
    finally:
        ops.set_conv_pos_major(True, dev)
    for b, s0 in zip([b for b in (xb_d, xb_s, rb_d, rb_s) if b is not None], snap):
        if not torch.equal(b.view(torch.int32), s0):
            fails.append("%s: an INPUT buffer was written" % c.name)
    _SEEN[c.name] = seen
    return seen, fails


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_conv_strided_case_every_tile(dev, ops, idx):
    seen, fails = _run_conv_case(idx, dev, ops)
    assert not fails, "%d failures, first %d:\n%s" % (len(fails), min(len(fails), 12), "\n".join(fails[:12]))
    assert any(v == "ok" for v in seen.values()), "%s: refused by every tile" % CASES[idx].name
    assert all(seen[(t, True)] == "ok" for t in F32_TILES if t != 95), "an engine tile refused %s" % CASES[idx].name


# ------------------------------------------------------------------------------------------------------------------ conv engine, fp16
# x16: fp16 x / w / residual (else fp32 x / w with an fp16 store: the half-precision stem's form, no residual); out16: fp16 store.
# Strides and offsets in ELEMENTS of the operand's type.
HCase = collections.namedtuple("HCase", "name n h w cin cout k stride pad res x16 out16 ldx ldo ldr oo orr", defaults=(0, 0, 0, 0, 0))
H_CASES = [
    HCase("f16_all_strided", 6, 7, 5, 64, 384, 1, 1, 0, True, True, True, ldx=72, ldo=404, ldr=388),
    HCase("f16_in_f32_out_strided", 6, 7, 5, 64, 384, 1, 1, 0, True, True, False, ldx=72, ldo=404, ldr=388),
    HCase("f16_cout200_m45", 5, 3, 3, 128, 200, 1, 1, 0, True, True, True, ldx=136, ldo=220, ldr=204),
    HCase("f16_3x3_s2_9x6", 3, 9, 6, 128, 64, 3, 2, 1, False, True, True, ldx=144, ldo=84),
    HCase("f16_3x3_6x9_res", 2, 6, 9, 64, 64, 3, 1, 1, True, True, True, ldx=80, ldo=84, ldr=68),
    HCase("f16_scalar_ld", 3, 5, 7, 24, 144, 1, 1, 0, True, True, True, ldx=32, ldo=147, ldr=145),
    HCase("f16_out_off2_res_off6", 3, 5, 7, 64, 64, 1, 1, 0, True, True, True, ldx=72, ldo=84, ldr=68, oo=2, orr=6),
    HCase("f16_in_f32_out_off1", 3, 5, 7, 64, 64, 1, 1, 0, True, True, False, ldx=72, ldo=85, ldr=68, oo=1),
    HCase("f16_linear_1280_200", 7, 1, 1, 1280, 200, 1, 1, 0, False, True, False, ldx=1288, ldo=3328),
    HCase("f32_in_f16_out_stem", 2, 9, 12, 4, 32, 3, 2, 1, False, False, True, ldx=16, ldo=52),
]
_H_SEEN = {}


def _f16_takes(c):
    """adaf_conv2d_bn_act_f16's documented rule: fp16 operands need cin % 8 == 0 and ldx % 8 == 0 (k x k filters: cin % 64 == 0)."""
    if not c.x16:
        return not c.res
    return c.cin % 8 == 0 and (c.ldx or c.cin) % 8 == 0 and (c.k == 1 or c.cin % 64 == 0)


def _run_f16_case(idx, dev):
    c = H_CASES[idx]
    if c.name in _H_SEEN:
        return _H_SEEN[c.name], []
    cc = Case(c.name, c.n, c.h, c.w, c.cin, c.cout, c.k, c.stride, c.pad, S.ACT_RELU, c.res, 0)
    # (the existing fp16 test's scaling: 1 / sqrt(K) weights, so its bound keeps its meaning; values rounded to fp16 first, so the
    #  products are exact and only the summation order -- and the one rounding of an fp16 store -- differs from the reference)
    x, w, sc, bi, res, oh, ow = _conv_data(cc, 500 + idx, dev, half=True)
    xt = torch.float16 if c.x16 else torch.float32
    ot = torch.float16 if c.out16 else torch.float32
    x, w = x.to(xt), w.to(xt)
    res = res.half() if c.res else None
    kw = dict(stride=c.stride, pad=c.pad, act=S.ACT_RELU)
    ref = S.conv_ref64(x, w, sc, bi, res, **kw)
    bound = S.conv_f16_bound(ot, ref)
    wd, scd, bid = w.to(dev), sc.to(dev), bi.to(dev)
    xb_d, xv_d = _place(x, 0, 0, dev, xt)
    xb_s, xv_s = _place(x, c.ldx, 0, dev, xt)
    rv_d = _place(res, 0, 0, dev, torch.float16)[1] if c.res else None
    rv_s = _place(res, c.ldr, c.orr, dev, torch.float16)[1] if c.res else None
    seen, fails = {}, []
    for tile in F16_TILES:
        tag = "%s tile %d" % (c.name, tile)
        outs = []
        try:
            for strided in (False, True):
                ob, ov = _empty((c.n, oh, ow), c.cout, c.ldo if strided else 0, c.oo if strided else 0, dev, ot)
                S.conv_call("f16", xv_s if strided else xv_d, wd, scd, bid, rv_s if strided else rv_d, ov, tile=tile, **kw)
                outs.append((ob, ov))
        except AdafError as e:
            seen[tile] = "refused"
            if _f16_takes(c):
                fails.append("%s: refused against the documented rule: %s" % (tag, e))
            continue
        seen[tile] = "ok"
        try:
            for (ob, ov), what in zip(outs, ("dense", "strided")):
                S.assert_guards_intact(ob, ov, "%s %s out" % (tag, what))
            dense, got = S.payload(outs[0][1]), S.payload(outs[1][1])
            assert got.dtype == ot
            assert bool(torch.isfinite(got).all()), "%s: %d non-finite outputs (a gap was read, or an element was not written)" % (
                tag, int((~torch.isfinite(got)).sum()))
            err = (got.cpu().double() - ref).abs().max().item()
            assert err < bound, "%s: max |err| vs float64 %.3e >= %.3e" % (tag, err, bound)
            assert torch.equal(got, dense), "%s: strided result differs from the dense call in %d elements" % (tag, int((got != dense).sum()))
        except AssertionError as e:
            fails.append(str(e))
    _H_SEEN[c.name] = seen
    return seen, fails


@pytest.mark.parametrize("idx", range(len(H_CASES)), ids=[c.name for c in H_CASES])
def test_conv_f16_strided_case_every_tile(dev, idx):
    seen, fails = _run_f16_case(idx, dev)
    assert not fails, "%d failures, first %d:\n%s" % (len(fails), min(len(fails), 12), "\n".join(fails[:12]))
    assert all(v == "ok" for v in seen.values()), (H_CASES[idx].name, seen)


def test_every_tile_family_accepted_strided_cases(dev, ops):
    """No case is refused by every tile, and every tile family really ran strided cases (a forced direct-to-LDS / split / 7x tile counts
    only on a shape its kernel takes: any other shape silently runs on the register-staged kernel)."""
    counts = collections.Counter()
    refused = collections.Counter()
    for i, c in enumerate(CASES):
        seen, _ = _run_conv_case(i, dev, ops)
        assert any(v == "ok" for v in seen.values()), "%s: refused by every tile" % c.name
        for (tile, pm), v in seen.items():
            fam = _family(tile)
            if v == "refused":
                refused[fam] += 1
            elif _strided(c) and (fam in ("automatic", "register-staged", "latency") or _dma_shape(c)):
                counts[fam] += 1
    for i, c in enumerate(H_CASES):
        seen, _ = _run_f16_case(i, dev)
        assert any(v == "ok" for v in seen.values()), "%s: refused by every tile" % c.name
        for tile, v in seen.items():
            if v == "refused":
                refused["fp16"] += 1
            elif tile:
                counts["fp16"] += 1
    print("\nstrided conv (case, tile) runs accepted per tile family: " + ", ".join("%s %d" % (f, counts[f]) for f in sorted(counts)))
    print("refused by a documented rule: " + (", ".join("%s %d" % (f, refused[f]) for f in sorted(refused)) or "none"))
    for fam in FAMILIES:
        assert counts[fam] > 0, "tile family %s accepted no strided case: %r" % (fam, dict(counts))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_strides_are_refused_before_any_launch(dev):
    """Each of these is an AdafError from the argument check: the output stays all canary (nothing was launched on it)."""
    lib, h = L.load_library(), L.handle(dev)
    n, hh, ww, cin, cout = 2, 3, 3, 16, 8
    xb, xv = _place(rnd((n, hh, ww, cin), 1), 24, 0, dev)
    rb, rv = _place(rnd((n, hh, ww, cout), 2), 12, 0, dev)
    w = rnd((cout, 1, 1, cin), 3).to(dev)
    ob, ov = _empty((n, hh, ww), cout, 12, 0, dev)
    untouched = ob.view(torch.int32).clone()

    def refused(kind, ld, x=xv, wt=w, res=rv, out=ov):
        with pytest.raises(AdafError):
            S.conv_call(kind, x, wt, None, None, res, out, ld=ld)
        torch.cuda.synchronize()
        assert torch.equal(ob.view(torch.int32), untouched)

    for kind in ("engine", "naive"):
        refused(kind, (cin - 4, 12, 12))         # ldx < cin
        refused(kind, (24, cout - 1, 12))        # ldo < cout
        refused(kind, (24, 12, cout - 4))        # ldr < cout
        refused(kind, (26, 12, 12))              # ldx % 4 != 0
    S.conv_call("engine", xv, w, None, None, rv, ov)            # ... and the same views with their true strides are taken
    S.assert_guards_intact(ob, ov)
    # fp16 operands: ldx % 8 != 0, cin % 8 != 0
    x16b, x16v = _place(rnd((n, hh, ww, cin), 4), 28, 0, dev, torch.float16)
    o16b, o16v = _empty((n, hh, ww), cout, 12, 0, dev, torch.float16)
    w16 = w.half()
    with pytest.raises(AdafError):
        S.conv_call("f16", x16v, w16, None, None, None, o16v)               # ldx = 28
    x12b, x12v = _place(rnd((n, hh, ww, 12), 5), 16, 0, dev, torch.float16)
    with pytest.raises(AdafError):
        S.conv_call("f16", x12v, w16[..., :12].contiguous(), None, None, None, o16v)      # cin = 12
    torch.cuda.synchronize()
    assert S.find_guard_damage(o16b, o16v) is None and bool(torch.isnan(o16v).all())
    # avgpool: ldo % 4 != 0, ldo < c
    x = rnd((3, 9, 8), 6).to(dev)
    pb, pv = _empty(3, 8, 12, 0, dev)
    for ldo in (10, 4):
        assert lib.adaf_global_avgpool_f32(h, L.ptr(x), 3, 9, 8, L.ptr(pv), ldo, L.stream_ptr()) != 0
    # copy2d: lds < cols, ldd < cols
    src = rnd((3, 8), 7).to(dev)
    assert lib.adaf_copy2d_f32(h, L.ptr(src), 7, L.ptr(pv), 12, 3, 8, L.stream_ptr()) != 0
    assert lib.adaf_copy2d_f32(h, L.ptr(src), 8, L.ptr(pv), 7, 3, 8, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert S.find_guard_damage(pb, pv) is None and bool(torch.isnan(pv).all())
    # GRU: ldx % 4 != 0 (all four entry points), backward ldx < feat
    g = _GruCase(dev, batch=2, steps=2, feat=8, hidden=16, classes=5)
    for ldx in (10, 9):
        with pytest.raises(AdafError):
            g.seq(g.x, ldx)
        with pytest.raises(AdafError):
            g.cls(g.x, ldx)
        with pytest.raises(AdafError):
            g.train(g.x, ldx)
    torch.cuda.synchronize()
    assert len(g._guarded) == 6 and all(S.is_all_canary(buf) for buf, _, _ in g._guarded)      # a refused call writes no workspace word
    g._guarded = []
    fw = g.train(g.x, 8)
    g.check_workspaces()
    with pytest.raises(AdafError):
        g.backward(g.x, 10, fw)
    with pytest.raises(AdafError):
        g.backward(g.x, 4, fw)                   # ldx < feat
    torch.cuda.synchronize()
    assert len(g._guarded) == 2 and all(S.is_all_canary(buf) for buf, _, _ in g._guarded)


# ------------------------------------------------------------------------------------------------------------------ avgpool, copy2d
@pytest.mark.parametrize("c", [4, 1280, 2048])
@pytest.mark.parametrize("hw", [1, 9, 49])
def test_avgpool_into_a_wider_matrix(dev, ops, hw, c):
    lib, h = L.load_library(), L.handle(dev)
    n = 5
    x = rnd((n, hw, c), 40 + hw + c)
    xb, xv = _place(x.reshape(n * hw, c), 0, 0, dev)             # an over-read of x meets NaN
    ld = 1280 + c                                                # the pooled features start at column 1280 of a wider matrix
    ob, ov = S.guarded(n, c, ld, S.lead_for(ld) + 1280, ld, torch.float32, dev)
    L.check(lib.adaf_global_avgpool_f32(h, L.ptr(xv), n, hw, c, L.ptr(ov), ld, L.stream_ptr()), h)
    db, dv = _empty(n, c, 0, 0, dev)
    L.check(lib.adaf_global_avgpool_f32(h, L.ptr(xv), n, hw, c, L.ptr(dv), c, L.stream_ptr()), h)
    S.assert_guards_intact(ob, ov, "avgpool strided out")
    S.assert_guards_intact(db, dv, "avgpool dense out")
    got = S.payload(ov)
    assert bool(torch.isfinite(got).all())
    np.testing.assert_allclose(got.cpu().numpy(), x.double().mean(1).numpy(), rtol=1e-6, atol=1e-6)      # the bound of test_pool_shift_foldbn
    assert torch.equal(got, S.payload(dv))
    assert torch.equal(got, ops.global_avgpool(x.reshape(n, hw, 1, c).to(dev)))


@pytest.mark.parametrize("cols", [1, 3, 1280])
def test_copy2d_strided_and_unaligned(dev, cols):
    lib, h = L.load_library(), L.handle(dev)
    rows = 7
    src = rnd((rows, cols), 60 + cols)
    sb, sv = _place(src, cols + 5, 1, dev)                       # no alignment requirement: both pointers 1 float off
    db, dv = _empty(rows, cols, cols + 9, 1, dev)
    before = sb.view(torch.int32).clone()
    assert sv.data_ptr() % 16 == 4 and dv.data_ptr() % 16 == 4
    L.check(lib.adaf_copy2d_f32(h, L.ptr(sv), sv.stride(0), L.ptr(dv), dv.stride(0), rows, cols, L.stream_ptr()), h)
    S.assert_guards_intact(db, dv, "copy2d dst")
    assert torch.equal(S.payload(dv).cpu(), src)                 # bit-exact, and no NaN from the source's gaps
    assert torch.equal(sb.view(torch.int32), before)


# ------------------------------------------------------------------------------------------------------------------ GRU
class _GruCase:
    """The four GRU entry points through ctypes, every output in a guarded buffer."""

    def __init__(self, dev, batch, steps, feat, hidden, classes, seed=70):
        self.dev, self.b, self.t, self.f, self.hid, self.c = dev, batch, steps, feat, hidden, classes
        self.lib, self.h = L.load_library(), L.handle(dev)
        s = 1.0 / np.sqrt(hidden)
        self.cpu = dict(w_ih=rnd((3 * hidden, feat), seed + 1, 1.0 / np.sqrt(feat)), w_hh=rnd((3 * hidden, hidden), seed + 2, s),
                        b_ih=rnd((3 * hidden,), seed + 3, 0.1), b_hh=rnd((3 * hidden,), seed + 4, 0.1),
                        fc_w=rnd((classes, hidden), seed + 5, s), fc_b=rnd((classes,), seed + 6, 0.1))
        self.p = {k: v.to(dev) for k, v in self.cpu.items()}
        self.x_cpu = rnd((batch, steps, feat), seed, 0.5)
        self.x = self.x_cpu.to(dev)
        self.dlogits_cpu = rnd((batch * steps, classes), seed + 7, 0.1)
        self.dlogits = self.dlogits_cpu.to(dev)
        self._guarded = []      # (buf, ws, nbytes) of every workspace handed out since the last check

    def _out(self, rows_shape, cols):
        return _empty(rows_shape, cols, 0, 0, self.dev)

    def _ws(self, nbytes):
        """Exactly the queried bytes behind guard bands (tests/strided.py guarded_workspace); check_workspaces() looks at every one handed out."""
        buf, ws = S.guarded_workspace(nbytes, self.dev)
        self._guarded.append((buf, ws, nbytes))
        return ws, nbytes

    def check_workspaces(self):
        torch.cuda.synchronize()
        for buf, ws, nbytes in self._guarded:
            S.assert_workspace_intact(buf, ws, "gru workspace of %d bytes" % nbytes, nbytes)
        self._guarded = []

    def seq(self, x, ldx):
        p, (ws, nb) = self.p, self._ws(self.lib.adaf_gru_cls_workspace_bytes(self.b, self.t, self.hid))
        hs = self._out((self.b, self.t), self.hid)
        L.check(self.lib.adaf_gru_seq_forward_f32(self.h, L.ptr(x), ldx, self.b, self.t, self.f, self.hid, L.ptr(p["w_ih"]), L.ptr(p["w_hh"]),
                                                  L.ptr(p["b_ih"]), L.ptr(p["b_hh"]), None, L.ptr(hs[1]), L.ptr(ws), nb, L.stream_ptr()), self.h)
        return dict(hs=hs)

    def cls(self, x, ldx):
        p, (ws, nb) = self.p, self._ws(self.lib.adaf_gru_cls_workspace_bytes(self.b, self.t, self.hid))
        logits, last = self._out(self.b * self.t, self.c), self._out(self.b, self.c)
        L.check(self.lib.adaf_gru_cls_forward_f32(self.h, L.ptr(x), ldx, self.b, self.t, self.f, self.hid, self.c, L.ptr(p["w_ih"]),
                                                  L.ptr(p["w_hh"]), L.ptr(p["b_ih"]), L.ptr(p["b_hh"]), L.ptr(p["fc_w"]), L.ptr(p["fc_b"]),
                                                  L.ptr(logits[1]), L.ptr(last[1]), L.ptr(ws), nb, L.stream_ptr()), self.h)
        return dict(logits=logits, last=last)

    def train(self, x, ldx):
        p, (ws, nb) = self.p, self._ws(self.lib.adaf_gru_cls_train_workspace_bytes(self.b, self.t, self.hid))
        gi, hs = self._out(self.b * self.t, 3 * self.hid), self._out((self.b, self.t), self.hid)
        logits, last = self._out(self.b * self.t, self.c), self._out(self.b, self.c)
        L.check(self.lib.adaf_gru_cls_train_forward_f32(self.h, L.ptr(x), ldx, self.b, self.t, self.f, self.hid, self.c, L.ptr(p["w_ih"]),
                                                        L.ptr(p["w_hh"]), L.ptr(p["b_ih"]), L.ptr(p["b_hh"]), L.ptr(p["fc_w"]), L.ptr(p["fc_b"]),
                                                        None, L.ptr(gi[1]), L.ptr(hs[1]), L.ptr(logits[1]), L.ptr(last[1]), L.ptr(ws), nb,
                                                        L.stream_ptr()), self.h)
        return dict(gi=gi, hs=hs, logits=logits, last=last)

    def backward(self, x, ldx, fw):
        p, (ws, nb) = self.p, self._ws(self.lib.adaf_gru_cls_backward_workspace_bytes(self.b, self.t, self.hid, self.c))
        h3 = 3 * self.hid
        o = dict(dx=self._out((self.b, self.t), self.f), dw_ih=self._out(h3, self.f), dw_hh=self._out(h3, self.hid), db_ih=self._out(1, h3),
                 db_hh=self._out(1, h3), dw_fc=self._out(self.c, self.hid), db_fc=self._out(1, self.c))
        L.check(self.lib.adaf_gru_cls_backward_f32(self.h, L.ptr(x), ldx, self.b, self.t, self.f, self.hid, self.c, L.ptr(p["w_ih"]),
                                                   L.ptr(p["w_hh"]), L.ptr(p["b_hh"]), L.ptr(p["fc_w"]), L.ptr(fw["gi"][1]), L.ptr(fw["hs"][1]),
                                                   None, L.ptr(self.dlogits), L.ptr(o["dx"][1]), L.ptr(o["dw_ih"][1]), L.ptr(o["dw_hh"][1]),
                                                   L.ptr(o["db_ih"][1]), L.ptr(o["db_hh"][1]), L.ptr(o["dw_fc"][1]), L.ptr(o["db_fc"][1]),
                                                   L.ptr(ws), nb, L.stream_ptr()), self.h)
        return o

    def ref64(self):
        """nn.GRU + nn.Linear in float64 on the CPU, gradients by autograd for the given dlogits."""
        gru = torch.nn.GRU(self.f, self.hid, batch_first=True).double()
        fc = torch.nn.Linear(self.hid, self.c).double()
        with torch.no_grad():
            gru.weight_ih_l0.copy_(self.cpu["w_ih"]), gru.weight_hh_l0.copy_(self.cpu["w_hh"])
            gru.bias_ih_l0.copy_(self.cpu["b_ih"]), gru.bias_hh_l0.copy_(self.cpu["b_hh"])
            fc.weight.copy_(self.cpu["fc_w"]), fc.bias.copy_(self.cpu["fc_b"])
        x = self.x_cpu.double().requires_grad_(True)
        hs, _ = gru(x)
        logits = fc(hs.reshape(self.b * self.t, self.hid))
        (logits * self.dlogits_cpu.double()).sum().backward()
        gi = x.detach().reshape(-1, self.f) @ gru.weight_ih_l0.detach().t() + gru.bias_ih_l0.detach()
        return dict(hs=hs.detach(), logits=logits.detach(), last=logits.detach().view(self.b, self.t, self.c)[:, -1], gi=gi, dx=x.grad,
                    dw_ih=gru.weight_ih_l0.grad, dw_hh=gru.weight_hh_l0.grad, db_ih=gru.bias_ih_l0.grad.view(1, -1),
                    db_hh=gru.bias_hh_l0.grad.view(1, -1), dw_fc=fc.weight.grad, db_fc=fc.bias.grad.view(1, -1))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _same_outputs(tag, strided, dense, ref, grads):
    for name in strided:
        (sb, sv), (db, dv) = strided[name], dense[name]
        S.assert_guards_intact(sb, sv, "%s %s (strided x)" % (tag, name))
        S.assert_guards_intact(db, dv, "%s %s (contiguous x)" % (tag, name))
        got = S.payload(sv)
        assert bool(torch.isfinite(got).all()), "%s %s: non-finite values (the gap of x was read)" % (tag, name)
        assert torch.equal(got, S.payload(dv)), "%s %s: strided x and its contiguous copy give different bits" % (tag, name)
        want = ref[name].reshape(got.shape)
        if grads:        # tests/test_stage3_gpu.py: gradients within 1e-4 relative of float64 autograd
            assert _rel(got.cpu(), want) < 1e-4, (tag, name, _rel(got.cpu(), want))
        else:            # tests/test_hip_parity.py: hidden states / logits within 1e-4 of the oracle
            assert (got.cpu().double() - want).abs().max().item() < 1e-4, (tag, name)


def test_gru_entry_points_read_x_through_ldx(dev, ops):
    """x is a column slice of a wider NaN-guarded matrix (the product's: columns [1280, 3328) hold the trunk's features)."""
    g = _GruCase(dev, batch=3, steps=4, feat=128, hidden=1024, classes=50)
    ld = g.f + 72
    xb, xv = S.guarded((g.b, g.t), g.f, ld, S.lead_for(ld) + 40, ld, torch.float32, dev)
    S.fill(xv, g.x)
    before = xb.view(torch.int32).clone()
    ref = g.ref64()
    try:
        for mode in (1, 0):
            ops.set_gru_persistent(mode, dev)
            tag = "gru persistent=%d" % mode
            _same_outputs(tag + " seq", g.seq(xv, ld), g.seq(g.x, g.f), ref, False)
            _same_outputs(tag + " cls", g.cls(xv, ld), g.cls(g.x, 0), ref, False)
            fs, fd = g.train(xv, ld), g.train(g.x, g.f)
            _same_outputs(tag + " train", fs, fd, ref, False)
            _same_outputs(tag + " backward", g.backward(xv, ld, fs), g.backward(g.x, g.f, fd), ref, True)
    finally:
        ops.set_gru_persistent(True, dev)
    assert torch.equal(xb.view(torch.int32), before)
    assert ops.gru_scan_timeouts(dev) == 0
    g.check_workspaces()


# ------------------------------------------------------------------------------------------------------------------ whole networks
def _feature_matrix(n, cols, dev, total=3328):
    """(buf, view): rows of a (n, total)-wide matrix, the view being its last `cols` columns; the columns in front are guard."""
    return S.guarded(n, cols, total, S.lead_for(total) + (total - cols), total, torch.float32, dev)


@pytest.mark.parametrize("math", ["f32", "f16", "split_bf16"])
def test_resnet_trunk_writes_its_features_through_ld(dev, math):
    """ResNet50Trunk.forward / forward_frames(out=view) into columns [1280, 3328) of a guarded matrix: the bits of the dense output, the
    neighbouring columns untouched -- with the pooled last conv3 on and off, and the small-batch form on and off."""
    net, _ = _P._trunk(dev, 1007)
    net.set_math(math)
    trunk = net._sync()
    n, p = 6, 96
    x4 = torch.zeros((n, p, p, 4), device=dev)
    x4[..., :3] = rnd((n, p, p, 3), 801).to(dev)
    frames = rnd((n, 3, 128, 128), 802).to(dev)
    actions = torch.from_numpy(np.random.Generator(np.random.PCG64(803)).random((n, 2), dtype=np.float32)).to(dev)
    first = None
    try:
        with torch.no_grad():
            for pool in (1, 0):
                for lat in (-1, 0):
                    trunk.set_latency_rows(lat)
                    with L.option("conv_pool", pool):
                        tag = "math %s conv_pool %d latency_rows %d" % (math, pool, lat)
                        dense = trunk.forward(x4).clone()
                        ob, ov = _feature_matrix(n, 2048, dev)
                        trunk.forward(x4, out=ov)
                        S.assert_guards_intact(ob, ov, tag + " forward")
                        assert torch.equal(S.payload(ov), dense) and bool(torch.isfinite(dense).all()), tag
                        dense_f = trunk.forward_frames(frames, actions, p).clone()
                        fb, fv = _feature_matrix(n, 2048, dev)
                        trunk.forward_frames(frames, actions, p, out=fv)
                        S.assert_guards_intact(fb, fv, tag + " forward_frames")
                        assert torch.equal(S.payload(fv), dense_f) and bool(torch.isfinite(dense_f).all()), tag
                        first = dense if first is None else first
                        assert torch.equal(dense, first), tag          # every plan of one arithmetic gives the same bits
    finally:
        trunk.set_latency_rows(-1)
    assert first.abs().max().item() > 1e-3


def test_mobilenetv2_writes_its_vector_through_ldvec(dev):
    from tests.test_hip_parity_r6 import _frames, _glancer
    net = _glancer(dev)
    eng = net._engine.sync()
    n, size = 3, 96
    x4 = _frames(dev, n, size, 810)
    with torch.no_grad():
        fmap, fvec = eng.forward(x4)
        fmap, fvec = fmap.clone(), fvec.clone()
        ob, ov = _feature_matrix(n, 1280, dev)
        mb, mv = _empty((n, fmap.shape[1], fmap.shape[2]), 1280, 0, 0, dev)
        need = eng._lib.adaf_mobilenetv2_workspace_bytes(eng._net, n, size, 0)
        ws = torch.empty(max(need // 4, 1), device=dev)
        L.check(eng._lib.adaf_mobilenetv2_forward(eng._net, L.ptr(x4), n, size, 0, 8, L.ptr(mv), L.ptr(ov), ov.stride(0), L.ptr(ws), need,
                                                  L.stream_ptr()), eng._h)
    S.assert_guards_intact(ob, ov, "mobilenetv2 featvec")
    S.assert_guards_intact(mb, mv, "mobilenetv2 featmap")
    assert torch.equal(S.payload(ov), fvec) and torch.equal(S.payload(mv), fmap) and bool(torch.isfinite(fvec).all())


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_effnet_writes_its_vector_through_ldvec(dev, dtype):
    from adafocus_amd.utils import nchw_to_nhwc4
    from tests import test_effnet as _E
    m, _ = _E._net(dev, "efficientnet-b0", 200, dtype=dtype)
    eng = m.engine()
    n, size = 3, 96
    x4 = nchw_to_nhwc4(rnd((n, 3, size, size), 820, 0.5).to(dev))
    with torch.no_grad():
        dense = eng.forward(x4)[1].clone()
        assert dense.shape == (n, 1280)
        ob, ov = _feature_matrix(n, 1280, dev)
        eng.forward(x4, out=ov)
    S.assert_guards_intact(ob, ov, "effnet %s featvec" % dtype)
    assert torch.equal(S.payload(ov), dense) and bool(torch.isfinite(dense).all())
