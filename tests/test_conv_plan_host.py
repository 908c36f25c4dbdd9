"""Which kernel form a conv gets, checked on the host: csrc/conv_gemm.hip decides it in plan_conv (a pure function over kTileTable) and
shows the plan through the un-headered debug hook adaf_conv_plan_debug, so no device is needed.  Every form gives the same bits, which
is why a wrong decision costs speed and fails no parity test -- these tests are what notices.  The expected values are DESIGN 3.2.1's
rows and the rules as the launcher stated them before the planner existed (fallback chain, narrow outputs, automatic split choice,
position-major gate, 4 GB reach of the scalar-base DMA); tools/conv_launch_digest.py ties the same plans to the kernels a device runs."""
import pytest

from adafocus_amd import _lib
from tests.helpers import load_tool
from tests.test_abi import _ensure_built

D = load_tool("conv_launch_digest")
CUS = 256          # an MI355X
E_BADARG, E_LAYOUT = -1, -2


def plan(n=2, hw=6, cin=64, cout=64, k=1, stride=1, pad=0, tile=0, tsm=(0, 8), ld=(0, 0, 0), cus=CUS, **flags):
    _ensure_built()
    p = _lib.ConvParams(n=n, h=hw, w=hw, cin=cin, cout=cout, kh=k, kw=k, stride=stride, pad=pad, act=_lib.ACT_RELU, tsm_segments=tsm[0],
                        tsm_div=tsm[1], ldx=ld[0], ldo=ld[1], ldr=ld[2], tile=tile)
    out = D.conv_plan(_lib.load_library(), p, D.plan_flags(**flags), cus)
    assert out is not None, "the library has no adaf_conv_plan_debug"
    return out


def form(p):
    return tuple(p[k] for k in ("dense", "special", "lean", "pos_major"))


def test_hook_is_not_part_of_the_c_abi():
    assert "adaf_conv_plan_debug" not in _lib.SYMBOLS
    assert plan()["tile"] > 0 and D.kernel_of(plan()).startswith("conv_gemm_glds_kernel<")


# ---- the temporal shift's form per fold -----------------------------------------------------------------------------------
WIDTHS = (64, 256, 512, 1024, 2048)       # input channels of the trunk's shifted conv1s
DIVS = (2, 4, 8, 16)
# fold = width / shift_div is a multiple of 32 (K = width always is):
WHOLE_SLICES = {64: (2,), 256: (2, 4, 8), 512: DIVS, 1024: DIVS, 2048: DIVS}
LARGE_DMA_TILES, SMALL_DMA_TILES = (31, 32, 34, 39), (33, 38)        # larger than 64 x 64 or not (128 x 32 is not)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("div", DIVS)
def test_shift_form_per_fold(width, div):
    shifted = dict(n=16, hw=6, cin=width, cout=max(64, width // 4), tsm=(8, div))
    lean = div in WHOLE_SLICES[width]
    for t in LARGE_DMA_TILES:       # row "fp32 DMA tiles larger than 64 x 64": lean K loop, a shift kind per 32-channel slice
        p = plan(tile=t, **shifted)
        assert p["tile"] == t and form(p) == (1, 1, int(lean), 0), (t, p)
        assert p["fold"] == width // div
        with _lib.option("tsm_lean", 0):
            assert form(plan(tile=t, **shifted)) == (1, 1, 0, 0), t
    for t in SMALL_DMA_TILES + (21, 22, 25, 71, 72, 41, 42, 45, 51, 52):     # row "every other fp32 tile, all split-bf16 tiles": general form
        p = plan(tile=t, **shifted)
        assert p["tile"] == t and form(p) == (1, 1, 0, 0), (t, p)
    for t in (61, 65, 66):
        p = plan(tile=t, presplit=True, **shifted)
        assert p["tile"] == t and form(p) == (1, 1, 0, 0), (t, p)
    for t in (1, 2, 5):           # the register-staged kernel has no SPECIAL argument: it selects the source itself
        p = plan(tile=t, **shifted)
        assert p["tile"] == t and D.FAMILIES[p["family"]] == "reg" and p["dense"] == 1 and p["lean"] == 0
    for t in (81, 82, 83, 84, 88):      # row "fp16-operand tiles": fold % 8 == 0 else ADAF_E_LAYOUT; counted in 32-bit words
        p = plan(tile=t, in16=True, out16=True, **shifted)
        if (width // div) % 8:
            assert p == {"refused": E_LAYOUT}
        else:
            assert p["tile"] == t and form(p) == (1, 1, 0, 0) and (p["K"], p["cin"], p["ldx"], p["fold"]) == (width // 2,) * 3 + (width // div // 2,)
            assert p["dt"] == 7 and plan(tile=t, in16=True, **shifted)["dt"] == 6


def test_shift_refusals_of_the_first_row():
    assert plan(n=16, cin=24, tsm=(8, 16)) == {"refused": E_LAYOUT}         # fold 1
    assert plan(n=16, cin=24, tsm=(8, 8)) == {"refused": E_LAYOUT}          # fold 3
    assert plan(n=16, cin=32, tsm=(8, 8))["special"] == 1                    # fold 4
    assert plan(n=15, cin=64, tsm=(8, 8)) == {"refused": E_BADARG}          # n % T
    assert plan(n=16, cin=64, tsm=(8, 0)) == {"refused": E_BADARG}
    assert plan(n=16, cin=64, k=3, pad=1, tsm=(8, 8)) == {"refused": E_BADARG}


# ---- the table: fallback ids -----------------------------------------------------------------------------------------------------------
# tile asked for -> tile that runs a shape the DMA kernel cannot take (a 3x3 with 12 input channels: K = 108)
REG_FALLBACK = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 21: 1, 22: 2, 23: 3, 24: 4, 25: 5, 26: 1, 31: 1, 32: 2, 33: 3, 34: 4, 38: 1, 39: 1,
                41: 1, 42: 2, 43: 3, 44: 4, 45: 5, 46: 1, 51: 1, 52: 2, 53: 3, 54: 4, 61: 1, 62: 2, 63: 3, 64: 4, 65: 1, 66: 1, 67: 1,
                71: 1, 72: 2, 73: 3, 74: 4}
# pre-split tile -> the on-the-fly split tile that runs when the weights are not pre-split (or K % 32 != 0)
SPLIT_FALLBACK = {61: 41, 62: 42, 63: 43, 64: 44, 65: 41, 66: 41, 67: 41}
SHAPES = {1: (128, 128, 2, 2), 2: (128, 64, 2, 2), 3: (64, 64, 2, 2), 4: (64, 128, 2, 2), 5: (256, 128, 4, 2), 25: (256, 128, 4, 2),
          26: (256, 128, 2, 2), 38: (128, 32, 4, 1), 39: (256, 32, 4, 1), 45: (256, 128, 4, 2), 46: (256, 128, 2, 2), 65: (128, 128, 4, 1),
          66: (256, 128, 8, 1), 67: (256, 128, 4, 2), 88: (128, 32, 4, 1)}
FAMILY = {0: "reg", 2: "dma_top", 3: "dma_mid", 4: "split6", 5: "split9", 6: "presplit", 7: "bar23", 8: "f16"}      # by tens digit of the id


@pytest.mark.parametrize("tile", sorted(REG_FALLBACK))
def test_fallback_of_every_row(tile):
    odd = dict(n=2, hw=9, cin=12, cout=40, k=3, pad=1)
    for presplit in (False, True):
        p = plan(tile=tile, presplit=presplit, **odd)
        assert p["tile"] == REG_FALLBACK[tile] and D.FAMILIES[p["family"]] == "reg" and p["dense"] == 0
    # an eligible shape stays on the row, and the row is what the id has always meant
    ok = dict(n=2, hw=9, cin=32, cout=40, k=3, pad=1)
    p = plan(tile=tile, presplit=True, **ok)
    assert p["tile"] == tile and D.FAMILIES[p["family"]] == FAMILY[tile // 10]
    assert (p["bm"], p["bn"], p["wgm"], p["wgn"]) == SHAPES.get(tile, SHAPES[tile % 10 if tile % 10 in (1, 2, 3, 4) else 1])
    assert p["fallback"] == (0 if tile <= 5 else SPLIT_FALLBACK.get(tile, REG_FALLBACK[tile]))
    assert (p["pipe"], p["split"], p["presplit"]) == {"reg": (0, 0, 0), "dma_top": (0, 0, 0), "dma_mid": (1, 0, 0), "bar23": (2, 0, 0),
                                                      "split6": (1, 6, 0), "split9": (1, 9, 0), "presplit": (1, 6, 1)}[FAMILY[tile // 10]]
    if tile in SPLIT_FALLBACK:
        assert plan(tile=tile, **ok)["tile"] == SPLIT_FALLBACK[tile]
        assert plan(tile=tile, presplit=True, n=2, hw=9, cin=20, cout=40)["tile"] == SPLIT_FALLBACK[tile]        # 1x1, K = 20


def test_rows_without_a_fallback():
    for t in (81, 82, 83, 84, 88):
        assert plan(tile=t, in16=True, n=2, hw=9, cin=24, cout=40, k=3, pad=1)["tile"] == -1          # k x k needs cin % 64 == 0
        p = plan(tile=t, in16=True, n=2, hw=9, cin=64, cout=40, k=3, pad=1)
        assert p["tile"] == t and D.FAMILIES[p["family"]] == "f16" and (p["bm"], p["bn"], p["wgm"], p["wgn"]) == SHAPES[t if t in SHAPES else t % 10]
    for t in (85, 86, 87):
        assert plan(tile=t, in16=True, cin=64)["tile"] == -1
    assert plan(tile=31, in16=True, cin=64)["tile"] in (81, 82, 83, 84)              # any other id: the automatic choice
    assert plan(in16=True, res16=True, cin=64)["tile"] > 80
    p = plan(tile=95, cin=64)                    # conv_lat.hip decides at the launch whether it takes the shape
    assert p["tile"] == 95 and D.FAMILIES[p["family"]] == "lat" and D.kernel_of(p) == "conv_lat_kernel<64>"
    # fp32 operands with an fp16 store: the register-staged 128 x 64 tile, whatever was asked for
    p = plan(tile=31, out16=True, cin=64)
    assert p["tile"] == 2 and D.kernel_of(p) == "conv_gemm_kernel<128, 64, 2, 2, 32, true, 0, 1>" and p["vec_epi"] == 1


# ---- automatic choices -------------------------------------------------------------------------------------------------------------------
def test_narrow_output_rules():
    many = dict(n=8, hw=64, cin=32)                      # 32768 rows = 256 row tiles of 128
    for cout in (16, 24, 32, 40, 96, 160):               # 64-wide column tiles would spend >= 20 % of their columns on padding
        assert plan(cout=cout, **many)["tile"] == 38, cout
        p = plan(cout=cout, cus=257, **many)             # one row tile short of the device
        assert D.FAMILIES[p["family"]] == "dma_mid" and p["bn"] >= 64, cout
        assert plan(cout=cout, in16=True, out16=True, **many)["tile"] == 88
        assert plan(cout=cout, in16=True, out16=True, cus=257, **many)["tile"] in (81, 82, 83, 84)
    for cout in (64, 128, 192, 56):
        assert plan(cout=cout, **many)["tile"] in (31, 32, 33, 34), cout
    # fewer rows, a long reduction: 25088 rows (196 tiles of 128; 98 of 256 x 5 column tiles of 32), K = 960
    assert plan(n=512, hw=7, cin=960, cout=160)["tile"] == 39
    assert plan(n=512, hw=7, cin=480, cout=160)["tile"] in (31, 32, 33, 34)          # K < 512
    assert plan(n=512, hw=7, cin=960, cout=160, cus=491)["tile"] in (31, 32, 33, 34)
    assert plan(n=512, hw=7, cin=960, cout=160, cus=490)["tile"] == 39
    # a shape the DMA kernel cannot take gets the cost model's register-staged tile, narrow or not
    assert plan(n=8, hw=64, cin=12, cout=24, k=3, pad=1)["tile"] in (1, 2, 3, 4)


def test_automatic_split_choice():
    assert plan(tile=40, n=8, hw=64, cin=64, cout=64)["tile"] == 42             # cout <= 64
    assert plan(tile=40, n=8, hw=64, cin=64, cout=128)["tile"] == 41            # 256 tiles of 128 x 128: twice the tiles >= the CUs
    assert plan(tile=40, n=2, hw=8, cin=64, cout=128)["tile"] == 43             # 1 tile: the cost model's 64 x 64 (128 rows x 128 columns)
    assert plan(tile=40, n=2, hw=8, cin=64, cout=128, cus=2)["tile"] == 41
    # weights pre-split: 41 -> 65 (waves of 32 x 128), otherwise the pre-split row of the same shape
    assert plan(tile=40, presplit=True, n=8, hw=64, cin=64, cout=64)["tile"] == 62
    assert plan(tile=40, presplit=True, n=8, hw=64, cin=64, cout=128)["tile"] == 65
    assert plan(tile=40, presplit=True, n=2, hw=8, cin=64, cout=128)["tile"] == 63
    assert plan(tile=40, presplit=True, n=8, hw=64, cin=36, cout=128)["tile"] == 41         # K % 32 != 0: no pre-split tile
    assert plan(tile=40, presplit=True, n=2, hw=9, cin=12, cout=40, k=3, pad=1)["tile"] in (1, 2, 3, 4)


# ---- position-major tiles ------------------------------------------------------------------------------------------------------------------
def test_position_major_gate():
    small = dict(hw=3, cin=32, cout=64, k=3, pad=1)        # 49 of 81 taps touch the image
    for t, bm in ((31, 128), (33, 64), (39, 256)):
        assert form(plan(tile=t, n=bm - 1, **small)) == (0, 0, 0, 0), t
        p = plan(tile=t, n=bm + 1, **small)
        assert form(p) == (0, 0, 1, 1) and (p["pm_images"], p["pm_groups"]) == (bm + 1, 2), t
        assert p["nblocks"] == 9 * 2 * p["tiles_n"] and p["tiles_n"] == -(-64 // p["bn"])
        p = plan(tile=t, n=bm, **small)
        assert form(p) == (0, 0, 1, 1) and (p["pm_images"], p["pm_groups"], p["nblocks"]) == (bm, 1, 9 * p["tiles_n"]), t
        assert form(plan(tile=t, n=bm, pm_allow=0, **small)) == (0, 0, 0, 0)
        assert form(plan(tile=t, n=bm, pm_allow=2, **small)) == (0, 0, 0, 1)         # all taps walked (an experiment): the general loop
    # the fill threshold 0.96: a 3x3 / pad 1 conv on an H x H map touches ((3H - 2) / 3H)^2 of its taps -- 0.9588 at 32, 0.96000 at 33
    assert (94 / 96) ** 2 < 0.96 < (97 / 99) ** 2
    assert form(plan(tile=31, n=128, hw=32, cin=32, cout=64, k=3, pad=1)) == (0, 0, 1, 1)
    assert form(plan(tile=31, n=128, hw=33, cin=32, cout=64, k=3, pad=1)) == (0, 0, 0, 0)
    assert form(plan(tile=31, n=128, hw=48, cin=32, cout=64, k=3, pad=1)) == (0, 0, 0, 0)
    assert form(plan(tile=31, n=128, hw=65, cin=32, cout=64, k=3, pad=1, stride=2)) == (0, 0, 0, 0) and 33 * 33 <= 4096     # fill, not size
    # other families: only the pre-split split tiles have the form, lean on the tile of 32 x 128 waves alone
    for t in (21, 41, 51, 71, 1):
        assert plan(tile=t, n=128, **small)["pos_major"] == 0, t
    assert form(plan(tile=65, presplit=True, n=128, **small)) == (0, 0, 1, 1)
    assert form(plan(tile=61, presplit=True, n=128, **small)) == (0, 0, 0, 1)
    assert form(plan(tile=65, presplit=True, n=127, **small)) == (0, 0, 0, 0)
    assert form(plan(tile=65, presplit=True, n=128, pm_allow=2, **small)) == (0, 0, 0, 0)
    with _lib.option("split_lean", 0):
        assert form(plan(tile=65, presplit=True, n=128, **small)) == (0, 0, 0, 1)
    assert form(plan(tile=31, n=128, hw=3, cin=32, cout=64)) == (1, 0, 1, 0)                 # a 1x1 has no taps to skip


# ---- the lean forms and the 4 GB reach of their scalar-base DMA ---------------------------------------------------------------------------
def test_lean_dense_and_row_gather():
    for t in (31, 32, 34, 39):
        assert form(plan(tile=t, n=4, hw=8, cin=64, cout=128)) == (1, 0, 1, 0), t
        p = plan(tile=t, n=4, hw=8, cin=64, cout=128, stride=2)          # ResNet's downsample branch: the dense kernel with a row gather
        assert form(p) == (1, 0, 1, 0) and p["gather"] == 1, t
    for t in (33, 38):           # 64 x 64 (and 128 x 32) tiles keep the general form
        assert form(plan(tile=t, n=4, hw=8, cin=64, cout=128)) == (1, 0, 0, 0), t
        assert form(plan(tile=t, n=4, hw=8, cin=64, cout=128, stride=2)) == (0, 0, 0, 0), t
    assert form(plan(tile=31, n=4, hw=8, cin=36, cout=128)) == (1, 1, 0, 0)               # partial last K slice
    assert form(plan(tile=31, n=4, hw=8, cin=64, cout=128, stride=2, k=1, pad=1)) == (0, 0, 0, 0)
    assert form(plan(tile=65, presplit=True, n=4, hw=8, cin=64, cout=128)) == (1, 0, 1, 0)
    assert form(plan(tile=65, presplit=True, n=4, hw=8, cin=64, cout=128, stride=2)) == (1, 0, 1, 0)
    assert form(plan(tile=61, presplit=True, n=4, hw=8, cin=64, cout=128)) == (1, 0, 0, 0)
    with _lib.option("split_lean", 0):
        assert form(plan(tile=65, presplit=True, n=4, hw=8, cin=64, cout=128)) == (1, 0, 0, 0)
    assert plan(tile=31, n=4, hw=8, cin=64, cout=128, vec_epi=True)["vec_epi"] == 2 and plan(tile=31, vec_epi=False)["vec_epi"] == 0


def test_dma_reach_fallbacks():
    rows = dict(n=512, hw=64)                                   # 2^21 rows
    assert form(plan(tile=31, cin=256, cout=64, **rows)) == (1, 0, 1, 0)                       # activations 2^31 bytes
    assert form(plan(tile=31, cin=256, cout=64, ld=(508, 0, 0), **rows)) == (1, 0, 1, 0)       # 0xfe000000
    assert form(plan(tile=31, cin=256, cout=64, ld=(512, 0, 0), **rows)) == (1, 0, 0, 0)       # 2^32: the general form
    assert form(plan(tile=31, n=2, hw=8, cin=32768, cout=8192)) == (1, 0, 1, 0)                # weights 2^30 bytes
    assert form(plan(tile=31, n=2, hw=8, cin=32768, cout=32768)) == (1, 0, 0, 0)               # 2^32
    # a row gather reaches over the INPUT map: 128 x 128 pixels x 128 channels x 4 bytes = 2^23 bytes per image
    assert form(plan(tile=31, n=256, hw=128, cin=128, cout=64, stride=2)) == (1, 0, 1, 0)
    assert form(plan(tile=31, n=512, hw=128, cin=128, cout=64, stride=2)) == (0, 0, 0, 0)
    # position-major tiles beyond the reach keep their form on the general loop
    assert form(plan(tile=31, n=2 ** 16, hw=8, cin=2048, cout=64, k=3, pad=1)) == (0, 0, 0, 1)
    # the shifted conv1's buffer form: 2 GB
    assert form(plan(tile=31, n=256, hw=64, cin=256, cout=64, tsm=(8, 8))) == (1, 1, 1, 0)      # 2^30
    assert form(plan(tile=31, n=512, hw=64, cin=256, cout=64, tsm=(8, 8))) == (1, 1, 0, 0)      # 2^31
    # the pre-split tile also addresses three bf16 planes: 6 bytes per weight
    assert form(plan(tile=31, n=2, hw=8, cin=28672, cout=28672)) == (1, 0, 1, 0)
    assert form(plan(tile=65, presplit=True, n=2, hw=8, cin=28672, cout=28672)) == (1, 0, 0, 0)
    assert form(plan(tile=65, presplit=True, n=2, hw=8, cin=16384, cout=16384)) == (1, 0, 1, 0)


def test_fused_tail_reach():
    """adaf_fused_tail_in_reach, which the trunk asks before it takes the fused stage-1 tail (conv2 3x3 64 -> 64, conv3 to 256 channels):
    the 256-channel map of every patch must lie within 32-bit byte offsets (0x3fffffff words), conv2's input within the DMA's 4 GB."""
    import ctypes as C
    _ensure_built()
    fn = _lib.load_library().adaf_fused_tail_reach_debug
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], C.c_int
    assert "adaf_fused_tail_reach_debug" not in _lib.SYMBOLS

    def reach(n, hw, n3=256, ldx=0):
        p = _lib.ConvParams(n=n, h=hw, w=hw, cin=64, cout=64, kh=3, kw=3, stride=1, pad=1, act=_lib.ACT_RELU, tsm_segments=0, tsm_div=8,
                            ldx=ldx, ldo=0, ldr=0, tile=0)
        return fn(C.byref(p), n3)
    assert (reach(4088, 32), reach(4096, 32)) == (1, 0)             # 128^2 patches: 0xff800000 and 2^32 bytes
    assert (reach(7281, 24), reach(7282, 24)) == (1, 0)             # 96^2 patches: 7282 x 576 x 1 KiB = 2^32 + 131072
    assert reach(4096, 32, n3=128) == 1 and reach(8192, 32, n3=128) == 0
    # conv2's input rows through their pitch: 2^20 rows of 1020 floats are 0xff000000 bytes
    assert (reach(1024, 32, ldx=1020), reach(1024, 32, ldx=1024)) == (1, 0)


def test_pooled_epilogue_eligibility():
    last = dict(n=28, hw=3, cin=512, cout=2048, vec_epi=True)           # the trunk's last conv3 at 96^2 patches: 14 images per 126-row tile
    p = plan(pool_hw=9, **last)
    assert p["tile"] == 32 and p["pool"] == 1 and form(p) == (1, 0, 1, 0) and (p["tiles_n"], p["nblocks"], p["vec_epi"]) == (32, 2 * 32, 2)
    assert D.kernel_of(p) == "conv_gemm_glds_kernel<128, 64, 2, 2, true, 1, false, 0, false, 0, false, true, true>"
    with _lib.option("conv_pool", 0):
        assert plan(pool_hw=9, **last)["tile"] == -1
    assert plan(pool_hw=9, **dict(last, vec_epi=False))["tile"] == -1
    assert plan(pool_hw=9, **dict(last, cin=500))["tile"] == -1              # K % 32
    assert plan(pool_hw=9, **dict(last, n=29))["tile"] == 32 and plan(pool_hw=10, **last)["tile"] == -1        # rows % hw
    assert plan(pool_hw=36, n=4, hw=6, cin=512, cout=2048, vec_epi=True)["tile"] == -1       # 3 images = 108 rows < 90 % of 128
    assert plan(pool_hw=9, n=2 ** 18, hw=3, cin=512, cout=2048, vec_epi=True)["tile"] == -1  # activations beyond the DMA's reach
    for res16, dt in ((False, 4), (True, 6)):            # fp16 operands: EfficientNet's head (DT 4) / the fp16 trunk's last conv3 (DT 6, rounded)
        p = plan(pool_hw=9, in16=True, res16=res16, **last)
        assert p["tile"] == 82 and p["pool"] == 1 and form(p) == (1, 0, 0, 0) and p["dt"] == dt and (p["K"], p["vec_epi"]) == (256, 1)
    assert plan(pool_hw=9, in16=True, **dict(last, cin=544))["tile"] == -1   # K % 64
