"""The automatic tile choice of the conv engine (csrc/conv_gemm.hip: conv_tile_cost, pick_tile), checked on the host through
adaf_conv_plan_debug.  A caller whose launches run beside those of other streams (the trunk, when another trunk forward is in flight on another
stream: the debug hook's BESIDE flag) has its tiles priced for that -- a fill-weighted mean of the average and the busiest CU's blocks, the loop
efficiencies of profiles/tile_regime_ab.md; every other caller, and every caller under option conv_tile_regime = 0, gets the choice as it
was (one block per CU as a whole round).  Every fp32 tile gives the same bits, so only these tests notice a changed pick.  Pinned: the
tile of every 1x1 and 3x3 conv of the ResNet-50 trunk after the stem at 1024 patches of 96^2 (the benchmark's step), 512 of 128^2 and
768 of 144^2 (where both regimes agree on 128 x 64), 512 of 96^2 and of 144^2 (where they do not), and the ids the earlier planner gave, recorded from it before the cost model changed."""
import pytest

from adafocus_amd import _lib
from tests.helpers import load_tool
from tests.test_abi import _ensure_built

D = load_tool("conv_launch_digest")
CUS = 256
PLANES = ((64, 3), (128, 4), (256, 6), (512, 3))

# last digit of the DMA tile id (31 128x128, 32 128x64, 33 64x64, 34 64x128) per conv launch 1..52, in the trunk's launch order:
# per block conv1, conv2, conv3, (downsample)
BEFORE = {
    (1024, 96): "2222222222222222222222223223323323323323322322332332",
    (512, 128): "2" * 52,
    (768, 144): "2" * 52,
    (8, 96): "3322332332333333333333333333333333333333333333333333",
    (512, 96): "2222222222232233233233223223323323323323323333333333",
    (512, 144): "2222222222232233233233223223323323323323323322332332",
}
NOW = {
    (1024, 96): "2" * 52,          # stages 3 and 4: conv1 and the position-major conv2 leave the 64 x 64 tile
    (512, 128): "2" * 52,
    (768, 144): "2" * 52,
    (8, 96): BEFORE[(8, 96)],      # small batches: as before
    # half the benchmark's batch, and the 144^2 patches of Something-Something: layers 2-4 leave the 64 x 64 tile wherever 128 x 64 tiles
    # still make 576 blocks or more; stage 4's conv1 and conv2 at 512 x 96^2 (288 blocks of 128 x 64, 1.125 per CU) stay
    (512, 96): "2222222222222222222222222222222222222222222322332332",
    (512, 144): "2" * 52,
}


def conv_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def trunk_convs(patch):
    """(name, input map, cin, cout, k, stride, pad) of the convs after the stem, in launch order."""
    hw = conv_out(conv_out(patch, 7, 2, 3), 3, 2, 1)
    out, cin = [], 64
    for s, (planes, blocks) in enumerate(PLANES):
        for b in range(blocks):
            stride = 2 if (b == 0 and s > 0) else 1
            hw2 = conv_out(hw, 3, stride, 1)
            name = "layer%d.%d." % (s + 1, b)
            out.append((name + "conv1", hw, cin, planes, 1, 1, 0))
            out.append((name + "conv2", hw, planes, planes, 3, stride, 1))
            out.append((name + "conv3", hw2, planes, planes * 4, 1, 1, 0))
            if b == 0:
                out.append((name + "downsample", hw, cin, planes * 4, 1, stride, 0))
            cin, hw = planes * 4, hw2
    return out


def plan(n, hw, cin, cout, k, stride, pad, tile=0, cus=CUS, **flags):
    _ensure_built()
    p = _lib.ConvParams(n=n, h=hw, w=hw, cin=cin, cout=cout, kh=k, kw=k, stride=stride, pad=pad, act=_lib.ACT_RELU, tsm_segments=0, tsm_div=8,
                        ldx=0, ldo=0, ldr=0, tile=tile)
    return D.conv_plan(_lib.load_library(), p, D.plan_flags(**flags), cus)


def picks(n, patch, beside=True, **kw):
    return [plan(n, *c[1:], beside=beside, **kw) for c in trunk_convs(patch)]


@pytest.mark.parametrize("shape", sorted(NOW))
def test_trunk_tiles_pinned(shape):
    n, patch = shape
    convs = trunk_convs(patch)
    assert len(convs) == 52
    got = picks(n, patch)
    for c, p, want in zip(convs, got, NOW[shape]):
        assert p["tile"] == 30 + int(want), (c, p["tile"])
    # the forms that go with the tiles: a k x k conv on small maps position-major and lean, a plain or strided 1x1 lean on every tile above 64 x 64
    for c, p in zip(convs, got):
        if p["tile"] != 33 and c[4] == 1:
            assert (p["dense"], p["lean"], p["pos_major"]) == (1, 1, 0), c
        if c[4] == 3 and c[1] <= 32 and n >= p["bm"]:
            assert (p["pos_major"], p["lean"]) == (1, 1), c
            assert p["nblocks"] == conv_out(c[1], 3, c[5], 1) ** 2 * -(-n // p["bm"]) * -(-c[3] // p["bn"]), c


@pytest.mark.parametrize("shape", sorted(BEFORE))
def test_option_restores_the_earlier_picks(shape):
    n, patch = shape
    assert _lib.get_option("conv_tile_regime") == 1
    with _lib.option("conv_tile_regime", 0):
        got = picks(n, patch)
    assert "".join(str(p["tile"] - 30) for p in got) == BEFORE[shape]
    assert _lib.get_option("conv_tile_regime") == 1
    # ... and so does every caller that does not say its launches overlap others: one stream, the C ABI's conv, the other networks
    assert picks(n, patch, beside=False) == got


def test_small_batch_plans_untouched():
    for n in (1, 8, 16):
        assert picks(n, 96) == picks(n, 96, beside=False)


def test_what_the_option_does_not_reach():
    cases = [dict(n=1024, hw=6, cin=1024, cout=256, k=1, stride=1, pad=0), dict(n=1024, hw=6, cin=256, cout=256, k=3, stride=1, pad=1)]
    for c in cases:
        for tile in (31, 32, 33, 34, 1, 3, 41, 43, 95):      # an explicit tile is taken as asked, in the form it always had
            now = plan(tile=tile, beside=True, **c)
            assert plan(tile=tile, **c) == now and now["tile"] == tile, (c, tile)
        for flags in (dict(in16=True, out16=True), dict(tile=40), dict(tile=40, presplit=True)):      # fp16 and split tiles: the serial regime
            assert plan(beside=True, **c, **flags) == plan(**c, **flags), (c, flags)
    # a shape the DMA kernel cannot take is priced for the register-staged kernel as before
    odd = dict(n=1024, hw=6, cin=12, cout=256, k=3, stride=1, pad=1)
    now = plan(beside=True, **odd)
    assert plan(**odd) == now and D.FAMILIES[now["family"]] == "reg"


def test_position_major_convs_are_priced_by_their_own_blocks():
    # 250 images: the ragged last group of a position-major tile is a whole tile per position
    p = plan(250, 6, 256, 256, 3, 1, 1, beside=True)
    assert p["pos_major"] == 1 and p["nblocks"] == 36 * p["pm_groups"] * p["tiles_n"] and p["pm_groups"] == -(-250 // p["bm"])
    # fewer images than rows of the smallest tile: row-major, the choice the earlier planner made
    few = plan(48, 6, 256, 256, 3, 1, 1, beside=True)
    assert plan(48, 6, 256, 256, 3, 1, 1) == few and few["pos_major"] == 0
    # position-major tiles switched off for the handle: priced row-major, still a DMA tile
    off = plan(1024, 6, 256, 256, 3, 1, 1, pm_allow=0, beside=True)
    assert off["pos_major"] == 0 and off["tile"] in (31, 32, 33, 34)


def test_option_values():
    c = dict(n=1024, hw=6, cin=1024, cout=256, k=1, stride=1, pad=0)
    with _lib.option("conv_tile_regime", 2):      # always: whatever the caller says
        assert plan(**c)["tile"] == 32 and plan(beside=True, **c)["tile"] == 32
    with _lib.option("conv_tile_regime", 0):      # never
        assert plan(**c)["tile"] == 33 and plan(beside=True, **c)["tile"] == 33
    assert plan(**c)["tile"] == 33 and plan(beside=True, **c)["tile"] == 32
    with pytest.raises(_lib.AdafError):
        _lib.set_option("conv_tile_regime", 3)
