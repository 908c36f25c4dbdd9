"""Pins the three host-side plan queries of the EfficientNet object -- adaf_effnet_whole_blocks, adaf_effnet_fused_expand_blocks and
adaf_effnet_workspace_bytes -- to a literal table recorded from the library BEFORE its geometry walk and its block-form rule were
each reduced to one statement: the queries must return, for every input, what they returned then.  They need a net object and with
it a handle, hence the gpu mark; nothing is launched.

Grid, on B3 (width 1.2 / depth 1.4) and B0 (1.0 / 1.0): size in SIZES -- every map side the whole-block kernel is instantiated for
(3 ... 9), the stride-2 9 -> 5 block at 144, a map too large for it at 300 --, pad_size 0 and 300 (75 under 300: dynamic padding),
both dtypes, and per (net, size, pad_size, dtype) the twelve SETTINGS columns: fusion on / off x effnet_plan complete, without
WHOLE_BLOCK, without FUSED_EXPAND x effnet_fused_blocks all / 0x14.  A COUNTS cell is "whole blocks/fused expand blocks"; in fp32
storage both are 0 everywhere.  WORKSPACE: bytes at n in NS, both sides of the half-chunk (512) and chunk (1024) thresholds."""
import itertools

import pytest
import torch

from adafocus_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu

NETS = {"b3": (1.2, 1.4), "b0": (1.0, 1.0)}
SIZES, PADS, NS = (32, 33, 75, 96, 128, 144, 300), (0, 300), (1, 511, 512, 1025)
ALL = 511
SETTINGS = list(itertools.product((True, False), (ALL, ALL & ~_lib.EF_PLAN_WHOLE_BLOCK, ALL & ~_lib.EF_PLAN_FUSED_EXPAND), (0xffffffff, 0x14)))

# (net, size, pad_size): one "whole/fused" cell per SETTINGS entry, fp16 storage
COUNTS = {
    ('b3', 32, 0): "4/3  4/1  0/7  0/2  4/0  4/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 32, 300): "4/3  4/1  0/7  0/2  4/0  4/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 33, 0): "14/2  14/1  0/7  0/2  14/0  14/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 33, 300): "4/3  4/1  0/7  0/2  4/0  4/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 75, 0): "15/7  15/2  0/7  0/2  15/0  15/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 75, 300): "11/5  11/2  0/7  0/2  11/0  11/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 96, 0): "15/7  15/2  0/7  0/2  15/0  15/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 96, 300): "15/7  15/2  0/7  0/2  15/0  15/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 128, 0): "15/7  15/2  0/7  0/2  15/0  15/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 128, 300): "15/7  15/2  0/7  0/2  15/0  15/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 144, 0): "16/7  16/2  0/7  0/2  16/0  16/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 144, 300): "16/7  16/2  0/7  0/2  16/0  16/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 300, 0): "0/7  0/2  0/7  0/2  0/0  0/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b3', 300, 300): "0/7  0/2  0/7  0/2  0/0  0/0  0/7  0/2  0/7  0/2  0/0  0/0",
    ('b0', 32, 0): "2/3  2/0  0/5  0/2  2/0  2/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 32, 300): "2/3  2/0  0/5  0/2  2/0  2/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 33, 0): "8/2  8/0  0/5  0/2  8/0  8/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 33, 300): "2/3  2/0  0/5  0/2  2/0  2/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 75, 0): "9/5  9/2  0/5  0/2  9/0  9/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 75, 300): "6/4  6/1  0/5  0/2  6/0  6/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 96, 0): "9/5  9/2  0/5  0/2  9/0  9/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 96, 300): "9/5  9/2  0/5  0/2  9/0  9/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 128, 0): "9/5  9/2  0/5  0/2  9/0  9/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 128, 300): "9/5  9/2  0/5  0/2  9/0  9/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 144, 0): "10/5  10/2  0/5  0/2  10/0  10/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 144, 300): "10/5  10/2  0/5  0/2  10/0  10/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 300, 0): "0/5  0/2  0/5  0/2  0/0  0/0  0/5  0/2  0/5  0/2  0/0  0/0",
    ('b0', 300, 300): "0/5  0/2  0/5  0/2  0/0  0/0  0/5  0/2  0/5  0/2  0/0  0/0",
}

# (net, dtype, size, pad_size): bytes at each n of NS
WORKSPACE = {
    ('b3', 'f32', 32, 0): (296960, 151746560, 152043520, 608174080),
    ('b3', 'f32', 32, 300): (296960, 151746560, 152043520, 608174080),
    ('b3', 'f32', 33, 0): (339968, 173527808, 173867008, 695468032),
    ('b3', 'f32', 33, 300): (296960, 151746560, 152043520, 608174080),
    ('b3', 'f32', 75, 0): (1589760, 812236800, 813826048, 3255304192),
    ('b3', 'f32', 75, 300): (1494272, 763377152, 764870656, 3059482624),
    ('b3', 'f32', 96, 0): (2525184, 1290369024, 1292894208, 5171576832),
    ('b3', 'f32', 96, 300): (2525184, 1290369024, 1292894208, 5171576832),
    ('b3', 'f32', 128, 0): (4474880, 2286663680, 2291138560, 9164554240),
    ('b3', 'f32', 128, 300): (4474880, 2286663680, 2291138560, 9164554240),
    ('b3', 'f32', 144, 0): (5658624, 2891556864, 2897215488, 11588861952),
    ('b3', 'f32', 144, 300): (5658624, 2891556864, 2897215488, 11588861952),
    ('b3', 'f32', 300, 0): (24529920, 12534593280, 12559122432, 50236489728),
    ('b3', 'f32', 300, 300): (24529920, 12534593280, 12559122432, 50236489728),
    ('b3', 'f16', 32, 0): (157696, 80582656, 80740352, 322961408),
    ('b3', 'f16', 32, 300): (157696, 80582656, 80740352, 322961408),
    ('b3', 'f16', 33, 0): (179712, 91473408, 91652096, 366608384),
    ('b3', 'f16', 33, 300): (157696, 80582656, 80740352, 322961408),
    ('b3', 'f16', 75, 0): (804608, 410828032, 411631616, 1646526464),
    ('b3', 'f16', 75, 300): (756480, 386398208, 387153920, 1548615680),
    ('b3', 'f16', 96, 0): (1271808, 649893888, 651165696, 2604662784),
    ('b3', 'f16', 96, 300): (1271808, 649893888, 651165696, 2604662784),
    ('b3', 'f16', 128, 0): (2246656, 1148041216, 1150287872, 4601151488),
    ('b3', 'f16', 128, 300): (2246656, 1148041216, 1150287872, 4601151488),
    ('b3', 'f16', 144, 0): (2840832, 1451665152, 1454505984, 5818023936),
    ('b3', 'f16', 144, 300): (2840832, 1451665152, 1454505984, 5818023936),
    ('b3', 'f16', 300, 0): (12291328, 6280541952, 6292832256, 25171329024),
    ('b3', 'f16', 300, 300): (12291328, 6280541952, 6292832256, 25171329024),
    ('b0', 'f32', 32, 0): (209920, 107269120, 107479040, 429916160),
    ('b0', 'f32', 32, 300): (209920, 107269120, 107479040, 429916160),
    ('b0', 'f32', 33, 0): (241408, 123065600, 123305984, 493223936),
    ('b0', 'f32', 33, 300): (209920, 107269120, 107479040, 429916160),
    ('b0', 'f32', 75, 0): (1142784, 583799296, 584941568, 2339766272),
    ('b0', 'f32', 75, 300): (1072384, 547792384, 548864000, 2195456000),
    ('b0', 'f32', 96, 0): (1816320, 928139520, 929955840, 3719823360),
    ('b0', 'f32', 96, 300): (1816320, 928139520, 929955840, 3719823360),
    ('b0', 'f32', 128, 0): (3224576, 1647725824, 1650950144, 6603800576),
    ('b0', 'f32', 128, 300): (3224576, 1647725824, 1650950144, 6603800576),
    ('b0', 'f32', 144, 0): (4076544, 2083113984, 2087190528, 8348762112),
    ('b0', 'f32', 144, 300): (4076544, 2083113984, 2087190528, 8348762112),
    ('b0', 'f32', 300, 0): (17679360, 9034054912, 9051734016, 36206936064),
    ('b0', 'f32', 300, 300): (17679360, 9034054912, 9051734016, 36206936064),
    ('b0', 'f16', 32, 0): (109568, 55989248, 56098816, 224395264),
    ('b0', 'f16', 32, 300): (109568, 55989248, 56098816, 224395264),
    ('b0', 'f16', 33, 0): (125696, 63887616, 64012288, 256049152),
    ('b0', 'f16', 33, 300): (109568, 55989248, 56098816, 224395264),
    ('b0', 'f16', 75, 0): (575488, 293959936, 294535168, 1178140672),
    ('b0', 'f16', 75, 300): (541184, 276251136, 276791296, 1107165184),
    ('b0', 'f16', 96, 0): (913664, 466817024, 467730432, 1870921728),
    ('b0', 'f16', 96, 300): (913664, 466817024, 467730432, 1870921728),
    ('b0', 'f16', 128, 0): (1618944, 827247872, 828866560, 3315466240),
    ('b0', 'f16', 128, 300): (1618944, 827247872, 828866560, 3315466240),
    ('b0', 'f16', 144, 0): (2044416, 1044696576, 1046740992, 4186963968),
    ('b0', 'f16', 144, 300): (2044416, 1044696576, 1046740992, 4186963968),
    ('b0', 'f16', 300, 0): (8852480, 4523502848, 4532355072, 18129420288),
    ('b0', 'f16', 300, 300): (8852480, 4523502848, 4532355072, 18129420288),
}


@pytest.fixture(scope="module")
def nets():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert _lib.get_option("effnet_plan") == ALL and _lib.get_option("effnet_chunk") == 1024
    dev = torch.device("cuda:0")
    return {name: hip_ops.EffNetNet(dev, w, d) for name, (w, d) in NETS.items()}


def _counts(ef, size, pad):
    row = []
    for fuse, plan, mask in SETTINGS:
        ef.set_fusion(fuse)
        with _lib.option("effnet_plan", plan), _lib.option("effnet_fused_blocks", mask):
            row.append("%d/%d" % (ef.whole_blocks(size, pad), ef.fused_expand_blocks(size, pad)))
    ef.set_fusion(True)
    return "  ".join(row)


@pytest.mark.parametrize("name", sorted(NETS))
def test_block_form_counts_are_the_recorded_ones(nets, name):
    ef = nets[name]
    ef.set_dtype("f16")
    got = {(name, s, p): _counts(ef, s, p) for s, p in itertools.product(SIZES, PADS)}
    assert got == {k: v for k, v in COUNTS.items() if k[0] == name}
    ef.set_dtype("f32")
    zeros = "  ".join(["0/0"] * len(SETTINGS))
    assert {_counts(ef, s, p) for s, p in itertools.product(SIZES, PADS)} == {zeros}
    # below the smallest input the network takes, and without a net: no blocks
    assert ef.whole_blocks(31, 0) == 0 and ef.fused_expand_blocks(31, 0) == 0
    assert ef._lib.adaf_effnet_whole_blocks(None, 144, 0) == 0 and ef._lib.adaf_effnet_fused_expand_blocks(None, 144, 0) == 0


@pytest.mark.parametrize("name", sorted(NETS))
def test_workspace_bytes_are_the_recorded_ones(nets, name):
    ef, got = nets[name], {}
    for dtype in ("f32", "f16"):
        ef.set_dtype(dtype)
        for s, p in itertools.product(SIZES, PADS):
            got[(name, dtype, s, p)] = tuple(int(ef._lib.adaf_effnet_workspace_bytes(ef._net, n, s, p)) for n in NS)
    assert got == {k: v for k, v in WORKSPACE.items() if k[0] == name}
