"""The handle-free *_workspace_bytes queries, pinned on the host.  A workspace layout is stated once per entry point (csrc: one function
walks an AdafCarver; the query measures with it, the call carves with it), so a query and its call cannot disagree -- what can still
move is the layout itself.  These are the totals the library returned BEFORE the layouts were restated (recorded from that build, not from
the code under test), over tools/workspace_sizes.py's HOST_GRID: batch 1 / 33, steps on both sides of the backward's barrier rounding,
hidden 16 / 1024, classes below and above 3 * hidden, patch 32 / 96 / 144, channels with and without the split-K term, 7 and 1001
pixels, and a non-positive extent in each query (0).  The queries that need a net object are compared by the same tool on a device
(profiles/workspace_layout_refactor_ab.md); tests/test_workspace_contract_gpu.py checks every offset behind guard bands."""
import pytest

from adafocus_amd import _lib
from tests.helpers import load_tool
from tests.test_abi import _ensure_built

W = load_tool("workspace_sizes")

EXPECTED = {
    "adaf_resnet50_workspace_bytes": [
        327680, 2949120, 6635520, 10813440, 97320960, 218972160, 0, 0],
    "adaf_gru_cls_workspace_bytes": [
        448, 28672, 16320, 1044480, 16576, 1060864, 16832, 1077248, 14784, 946176, 538560, 34467840, 547008, 35008512, 555456, 35549184, 0,
        0, 0],
    "adaf_gru_cls_train_workspace_bytes": [
        256, 16384, 4224, 270336, 4288, 274432, 4352, 278528, 8448, 540672, 139392, 8921088, 141504, 9056256, 143616, 9191424, 0, 0, 0],
    "adaf_gru_cls_backward_workspace_bytes": [
        7168, 7296, 442624, 442752, 50816, 50944, 3236096, 3236224, 51776, 51904, 3281408, 3281536, 52480, 52608, 3326464, 3326592, 31744,
        31872, 2015488, 2015616, 1472128, 1472256, 94200064, 94200192, 1495616, 1495744, 95687168, 95687296, 1518848, 1518976, 97174016,
        97174144, 0, 0, 0, 0],
    "adaf_dwconv_same_workspace_bytes": [
        64, 64, 64, 64, 64, 64, 64, 64, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 5120, 256, 128, 320, 192, 256, 128, 192, 256, 25600,
        25600, 25600, 25600, 51200, 51200, 30720, 46080, 64, 128, 64, 64, 64, 128, 64, 64, 5120, 5120, 10240, 10240, 5120, 5120, 10240,
        10240, 576, 576, 576, 512, 576, 576, 384, 192, 46080, 51200, 40960, 46080, 92160, 92160, 61440, 61440, 2112, 2112, 2112, 2112, 2112,
        2112, 2112, 2112, 168960, 168960, 168960, 168960, 168960, 168960, 168960, 168960, 8448, 4224, 10560, 6336, 8448, 4224, 6336, 8448,
        844800, 844800, 844800, 844800, 1689600, 1689600, 1013760, 1520640, 2112, 4224, 2112, 2112, 2112, 4224, 2112, 2112, 168960, 168960,
        337920, 337920, 168960, 168960, 337920, 337920, 19008, 19008, 19008, 16896, 19008, 19008, 12672, 6336, 1520640, 1689600, 1351680,
        1520640, 3041280, 3041280, 2027520, 2027520, 0, 0, 0, 0, 0],
    "adaf_ppo_head_workspace_bytes": [
        8, 264, 504, 16632, 512, 16896, 520, 17160, 0, 0],
    "adaf_ppo_wenc_grad_workspace_bytes": [
        448, 896, 448, 16384, 448, 163840, 64064, 128128, 64064, 262144, 64064, 2621440, 0, 0, 0],
    "adaf_ppo_encoder_backward_workspace_bytes": [
        17344, 1053568, 181184, 1217408, 108736, 6563968, 272576, 6727808, 48064, 1213312, 703424, 1868672, 311488, 6895744, 4571328,
        11155584, 78784, 1373056, 1389504, 2683776, 514240, 7227520, 8706240, 15419520, 2075584, 11756416, 10431424, 20112256, 13693120,
        28792960, 22048960, 37148800, 0, 0, 0, 0, 0, 0],
}


def test_the_grid_is_the_recorded_one():
    assert set(W.HOST_GRID) == set(EXPECTED)
    for q, grid in W.HOST_GRID.items():
        assert len(grid) == len(EXPECTED[q]) and len(set(grid)) == len(grid), q
        assert q in _lib.SYMBOLS, q
    # the shapes the totals must be sensitive to
    gru = W.HOST_GRID["adaf_gru_cls_backward_workspace_bytes"]
    assert {a[0] for a in gru} >= {1, 33} and {a[1] for a in gru} >= {1, 63, 64, 65} and {a[2] for a in gru} >= {16, 1024}
    assert any(a[3] == 5 for a in gru) and any(a[3] > 3 * a[2] > 0 for a in gru)
    assert {a[2] for a in W.HOST_GRID["adaf_resnet50_workspace_bytes"]} >= {32, 96, 144}
    wenc = W.HOST_GRID["adaf_ppo_wenc_grad_workspace_bytes"]
    assert {a[0] for a in wenc} >= {7, 1001} and any(a[1] % 128 for a in wenc if a[1] > 0) and any(a[1] == 1280 for a in wenc)


@pytest.mark.parametrize("query", sorted(EXPECTED))
def test_sizes_are_the_recorded_ones(query):
    _ensure_built()
    fn = getattr(_lib.load_library(), query)
    got = [int(fn(*args)) for args in W.HOST_GRID[query]]
    wrong = [(args, g, e) for args, g, e in zip(W.HOST_GRID[query], got, EXPECTED[query]) if g != e]
    assert not wrong, "%s: (args, bytes, recorded bytes) %s" % (query, wrong[:8])
    # every case whose extents are all positive needs a workspace; a non-positive extent answers 0
    for args, g in zip(W.HOST_GRID[query], got):
        extents = [a for a in args if a is not None]
        if query == "adaf_dwconv_same_workspace_bytes":
            extents = extents[:4] + extents[5:6]          # (k and dtype are not extents)
        assert (g > 0) == all(a > 0 for a in extents), (query, args, g)
