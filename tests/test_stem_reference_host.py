"""tests/stem_reference.py checked on the CPU: the float64 statement of the stem against nn.Conv2d / nn.BatchNorm2d(eval) / nn.ReLU /
nn.MaxPool2d, the spread of every case, and the properties the case tables of tests/test_stem_forms_gpu.py are claimed to have."""
import pytest
import torch

from tests import stem_reference as SR

CUS = 256          # the table arithmetic below is done for an MI355X; the GPU tests take the count from the device


def _modules(w, scale, bias):
    """conv1 / bn1 / relu / maxpool of torchvision's ResNet in float64, with BN statistics that fold to exactly (scale, bias): mean 0,
    var 1 - eps, gamma = scale, beta = bias."""
    conv = torch.nn.Conv2d(3, 64, 7, 2, 3, bias=False).double()
    bn = torch.nn.BatchNorm2d(64).double().eval()
    with torch.no_grad():
        conv.weight.copy_(w.double())
        bn.weight.copy_(scale.double())
        bn.bias.copy_(bias.double())
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0 - bn.eps)
    return conv, bn, torch.nn.ReLU(), torch.nn.MaxPool2d(3, 2, 1)


@pytest.mark.parametrize("p", [1, 2, 7, 18, 33, 50, 98])
def test_reference_is_the_module_chain_in_float64(p):
    prm = SR.params()
    x4 = SR.patches(3, p, lane3=7.0)                        # lane 3 carries a value: the reference must not read it
    conv, bn, relu, pool = _modules(*prm)
    with torch.no_grad():
        y = relu(bn(conv(x4[..., :3].permute(0, 3, 1, 2).double())))
        want = {"conv": y.permute(0, 2, 3, 1), "pool": pool(y).permute(0, 2, 3, 1)}
    got = SR.stem(x4, *prm)
    oh = SR.conv_size(p)
    assert got["conv"].shape == (3, oh, oh, 64) and got["pool"].shape == (3, SR.pool_size(oh), SR.pool_size(oh), 64)
    for k in want:
        assert got[k].dtype == torch.float64
        assert float((got[k] - want[k]).abs().max()) <= 1e-12, k
    assert torch.equal(SR.stem(SR.patches(3, p), *prm)["pool"], got["pool"])


def test_parameters_have_a_dead_and_an_inverted_channel():
    w, scale, bias = SR.params()
    assert scale[1] == 0 and bias[1] < 0 and scale[2] < 0
    rest = torch.cat([scale[:1], scale[3:]])
    assert bool((rest >= 0.5).all()) and bool((rest < 1.5).all())
    x4 = SR.patches(3, 37)
    out = SR.stem(x4, w, scale, bias)
    assert bool((out["pool"][..., 1] == 0).all()) and bool((out["conv"][..., 1] == 0).all())
    assert bool((out["pool"][..., 2] > 0).any())
    zeros = float((out["pool"] == 0).double().mean())
    assert 1.0 / 64 <= zeros <= 0.05, zeros                # the dead channel and a little more: live windows next to dead ones
    assert not torch.equal(x4[0], x4[1]) and not torch.equal(x4[1], x4[2])


@pytest.mark.parametrize("p,n", [(1, 3), (2, 3), (7, 3), (30, 3), (64, 3), (98, 2), (144, 2)])
def test_every_spread_is_positive_and_the_bound_stays_near_fp32_rounding(p, n):
    r = SR.measure(SR.patches(n, p), SR.params())
    for k in ("conv", "pool"):
        assert r.spread[k] > 0 and r.scale[k] > 0, (p, k)
        b = SR.bound_single(r.spread[k])
        print("P=%d n=%d %s: spread %.3e bound %.3e" % (p, n, k, r.spread[k], b))
        assert 2.0 ** -22 <= b < 1e-5, (p, k, r.spread[k])          # a few ulps of the largest entry: 4e-7 at P = 1 .. 4e-6 at P = 144


def test_tile_table():
    assert SR.tile_waves(4) == 5 and SR.tile_waves(6) == 7
    sizes = {p for p, _ in SR.TILE_CASES}
    for p, rows in SR.TILE_PICKS.items():
        assert p in sizes and SR.tile_rows(p) == rows, p                       # forcing the other height is the point
    geometry = {p: (SR.conv_size(p), SR.pool_size(SR.conv_size(p))) for p in sizes}
    assert geometry[1] == geometry[2] == (1, 1)
    assert geometry[18] == (9, 5) and geometry[37] == (19, 10) and geometry[50] == (25, 13) and geometry[100] == (50, 25)
    assert geometry[98] == (49, 25)                                            # odd OH: the last pooling window hangs over the map
    assert {oh % 2 for oh, _ in geometry.values()} == {0, 1} and {ph % 2 for _, ph in geometry.values()} == {0, 1}
    # the tile loop goes round: two tiles per image at either height, more tiles than the 2 x CUs blocks
    p, spec = SR.TILE_CASES[-1]
    ph = geometry[p][1]
    assert p == 32 and -(-ph // 4) == 2 and -(-ph // 6) == 2 and ph <= 8 and 2 * SR.images(spec, CUS) > 2 * CUS


def test_conv_table():
    geometry = {p: SR.conv_size(p) for p, _ in SR.CONV_CASES}
    assert geometry[7] == 4 and geometry[30] == 15 and geometry[33] == 17 and geometry[64] == 32 and geometry[96] == 48
    assert (-(-17 // 8), -(-17 // 16)) == (3, 2) and 32 % 8 == 0 and 48 % 16 == 0       # partial and whole 8 x 16 tiles
    p, spec = SR.CONV_CASES[-1]
    assert geometry[p] == 8 and SR.images(spec, CUS) > 3 * CUS                 # one tile per image, more tiles than blocks


def test_strip_table():
    assert {p: SR.strip_bpc(p) for p in SR.STRIP} == {64: 2, 96: 1, 128: 2, 144: 1}
    for p, (ow, r) in SR.STRIP.items():
        assert 2 * ow == p and ow % r == 0 and r % 2 == 0 and (r * ow) % 32 == 0 and r * ow <= 512
    for p, spec in SR.STRIP_CASES:
        bpc = SR.strip_bpc(p)
        n, grid = SR.images(spec, CUS, bpc), CUS * bpc
        most = -(-n // min(n, grid))                                           # images of block 0
        if spec.bpc_cus:
            assert most == 3 and n // grid == 2                                # blocks with three images and blocks with two
            held = SR.held_images(n, grid)
            assert {i // grid for i in held} == {0, 1, 2} and 0 in held and n - 1 in held and len(held) >= 8
        elif spec.cus:
            assert most == (2 if bpc == 1 else 1)
        else:
            assert n == 1
    assert max(SR.images(s, CUS, SR.strip_bpc(p)) * p * p * 16 for p, s in SR.STRIP_CASES) < 300 << 20


def test_held_images():
    assert SR.held_images(3) == [0, 1, 2] and SR.held_images(8) == list(range(8))
    h = SR.held_images(773, 768)
    assert 0 in h and 772 in h and 768 in h and len(h) >= 8
    assert SR.held_images(100) == [0, 1, 2, 3, 4, 5, 6, 99]


def test_walk_form_table():
    got = {p: (SR.walk_form(p, 8, CUS), SR.walk_form(p, CUS + 3, CUS)) for p in SR.AUTO_SIZES}
    assert got == {96: ("tile6", "strip"), 128: ("unfused", "strip"), 144: ("tile6", "strip"), 160: ("tile6", "tile6"),
                   176: ("unfused", "unfused"), 192: ("tile6", "tile6"), 224: ("unfused", "unfused")}


def test_gather_table():
    seen_lane3 = False
    for c in SR.GATHER_CASES:
        assert c.p in SR.STRIP and c.h >= c.p and c.w >= c.h and c.nf % c.fpa == 0
        act = SR.gather_actions(c)
        assert act.shape == (c.k * c.nf // c.fpa, 2)
        o = SR.origins(act, c.h, c.w, c.p)
        assert o[:, 0].min() >= 0 and o[:, 0].max() <= c.h - c.p and o[:, 1].min() >= 0 and o[:, 1].max() <= c.w - c.p
        seen_lane3 |= c.lane3 != 0
    assert seen_lane3
    assert any(c.h == c.p for c in SR.GATHER_CASES) and any((c.h - c.p) % 4 for c in SR.GATHER_CASES) and any(c.w != c.h for c in SR.GATHER_CASES)
    assert {c.fpa for c in SR.GATHER_CASES} == {1, 8} and any(c.k == 2 for c in SR.GATHER_CASES)
    # the edge table of the first case: corners, clamped values, and products that land on both sides of an integer
    c = SR.GATHER_CASES[0]
    act = SR.gather_actions(c)
    o = SR.origins(act, c.h, c.w, c.p)
    span = c.h - c.p
    assert o[:4].tolist() == [[0, 0], [span, span], [0, span], [span, 0]]
    assert float(act.min()) < 0 and float(act.max()) > 1
    pairs = o[4:8]
    assert any(abs(int(y) - int(x)) == 1 for y, x in pairs), pairs.tolist()   # one ulp of the action moves the window by a pixel
    # the CPU gather cuts the windows the origins say
    fr = SR.frames(c.nf, c.h, c.w)
    g = SR.gather(fr, act, c.p, c.fpa, c.k)
    y0, x0 = o[5]
    assert torch.equal(g[5, :, :, :3], fr[5, :, y0:y0 + c.p, x0:x0 + c.p].permute(1, 2, 0)) and bool((g[..., 3] == 0).all())


def test_maxpool_inputs():
    for h, w, c in SR.MAXPOOL_SHAPES:
        assert c % 4 == 0
        neg = SR.maxpool_input(h, w, c, "negative")
        assert bool((SR.maxpool(neg) < 0).all())                               # zero padding would win here: -inf padding does not
        inf = SR.maxpool_input(h, w, c, "neginf")
        assert bool(torch.isinf(SR.maxpool(inf)[-1]).all()) and not bool(torch.isnan(inf).any())
