"""The trunk under the two automatic tile choices (option conv_tile_regime: 2 = every forward priced for launches that run beside others,
0 = never, the picks before it; 1, the default, prices a forward that way when another trunk forward is in flight on another stream).  Every
fp32 tile walks k in the same order, so the features are the same bits.  256 and 250 patches of 96^2 are two position-major groups of
128-row tiles, the second one ragged at 250; with the temporal shift (T = 8) the shifted conv1s change tile as well.  The trunk refuses 250
patches at T = 8 (clips must be whole) before it launches anything, under either choice; 248 patches are the ragged shifted case.  At 8
patches the plans themselves must not move.  The default is held to its rule: the earlier picks on an idle device and under stream
capture, the busy picks behind a forward still running on another stream."""
import numpy as np
import pytest
import torch

from adafocus_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    from adafocus_amd.resnet import resnet50
    m = resnet50(num_classes=10).eval()
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 23).items()})
    m = m.to(torch.device("cuda:0"))
    m.set_math("f32")
    return m


def patches(n):
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(4100 + n)).standard_normal((n, 96, 96, 4), dtype=np.float32)).to("cuda:0")
    x[..., 3] = 0
    return x


@pytest.fixture(scope="module")
def streams():
    return [torch.cuda.Stream(device="cuda:0") for _ in range(2)]


def run(net, x, tsm, regime):
    """(features, tile id per launch) under one tile choice, on an idle device."""
    net.tsm_segments = tsm
    torch.cuda.synchronize()
    with _lib.option("conv_tile_regime", regime):
        feat = net.features_nhwc4(x).clone()
        tiles = [e["tile"] for e in net._sync().profile(x, tsm_segments=tsm)]
    torch.cuda.synchronize()
    return feat, tiles


@pytest.mark.parametrize("n,tsm", [(256, 0), (256, 8), (250, 0), (248, 8)])
def test_features_bit_identical_under_both_tile_choices(net, n, tsm):
    x = patches(n)
    now, tiles_now = run(net, x, tsm, 2)
    before, tiles_before = run(net, x, tsm, 0)
    assert torch.isfinite(now).all() and now.abs().max() > 0
    assert torch.equal(now, before)
    assert len(tiles_now) == len(tiles_before) and tiles_now != tiles_before        # the two choices really differ at this size
    moved = [(a, b) for a, b in zip(tiles_before, tiles_now) if a != b]
    assert all(a == 33 and b in (31, 32, 34) for a, b in moved), moved               # ... and only away from the 64 x 64 tile


def test_ragged_clips_refused_alike(net):
    x = patches(250)
    for regime in (2, 1, 0):
        with pytest.raises(_lib.AdafError):
            run(net, x, 8, regime)
    net.tsm_segments = 0


@pytest.mark.parametrize("tsm", [0, 8])
def test_small_batch_plans_untouched(net, tsm):
    x = patches(8)
    now, tiles_now = run(net, x, tsm, 2)
    before, tiles_before = run(net, x, tsm, 0)
    assert tiles_now == tiles_before
    assert torch.equal(now, before)


def test_default_follows_what_is_in_flight(net, streams):
    x = patches(256)
    busy, tiles_busy = run(net, x, 0, 2)
    alone, tiles_alone = run(net, x, 0, 0)
    assert _lib.get_option("conv_tile_regime") == 1
    trunk = net._sync()
    # an idle device, whichever stream the forward before was on: the picks of a launch that has the device to itself
    for s in (streams[0], streams[1], streams[0]):
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            assert [e["tile"] for e in trunk.profile(x)] == tiles_alone
    # two forwards still running on one stream while the next is planned on another: priced for launches that run beside others
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        net.features_nhwc4(x)
        net.features_nhwc4(x)
    with torch.cuda.stream(streams[1]):
        tiles = [e["tile"] for e in trunk.profile(x)]
        feat = net.features_nhwc4(x).clone()
    torch.cuda.synchronize()
    assert tiles == tiles_busy and torch.equal(feat, alone)
    # ... but never the same stream's own earlier work
    with torch.cuda.stream(streams[0]):
        net.features_nhwc4(x)
        assert [e["tile"] for e in trunk.profile(x)] == tiles_alone
    torch.cuda.synchronize()


def test_capture_beside_running_forwards(net, streams):
    """Under stream capture the planner asks nothing of the device (an event query would invalidate the capture) and takes the picks of a
    launch that has the device to itself -- a graph may be replayed alone, GFV.capture_hot_path(exclusive=True).  The capture must
    succeed while another stream's forwards are still running, and replay the same bits."""
    x = patches(256)
    alone, _ = run(net, x, 0, 0)
    cap = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(cap):
        net.features_nhwc4(x)                         # the capture stream's scratch exists before the capture
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        for _ in range(3):
            net.features_nhwc4(x)                     # still running while the capture below is planned
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        feat = net.features_nhwc4(x)
    torch.cuda.synchronize()
    feat.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(feat, alone)
