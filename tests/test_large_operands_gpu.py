"""Convs and the ResNet-50 trunk on both sides of the conv engine's 2 GiB / 4 GiB offset limits ("The 32-bit reach").

The fast forms of csrc/conv_gemm.hip address an operand with 32-bit byte offsets from a scalar base; host-side gates hand a conv whose
operand is too large for that to the pointer-walking general form.  tests/test_conv_plan_host.py pins what the planner ANSWERS on either
side of the gates; here the kernels RUN there: the lean forms at the top of their reach (lane offsets up to 0xff000000, the shifted
form's neighbour rows and out-of-range marker just under 2^31) and the general forms with operands, outputs and residuals above 4 GiB.

Part 1, single convs through the C ABI.  A large pixel stride (ldx / ldo / ldr) inflates the byte span while the arithmetic stays a few
milliseconds.  Every buffer is filled with the NaN canary on the device, the payload written through the stride.  Per case:
  - the plan hook must name the form the case is about (lean below the gate, general at it), so no case silently tests another form;
  - float64 reference on the CPU (tests/strided.conv_ref64, bound CONV_TOL) over whole images / clips at the lowest offsets, around byte
    offset 2^31 of the large operand and at the highest offsets;
  - every row, every tile: torch.equal with the same payload run dense (the regime the rest of the suite holds to the oracle);
  - every gap word of the output still the canary, lead and trail too; inputs unchanged (checksum).
Part 2, the trunk at 2040 ... 4096 patches of 128^2 (stage-1 maps of 2 GiB and 4 GiB): a patch's features do not depend on the batch it
came in, so windows of 16 patches must be torch.equal to the same patches run as batches of 16 (small batches against the oracle:
tests/test_hip_parity.py::test_resnet50_trunk_vs_oracle).  At 4096 patches the fused stage-1 tail is beyond its reach and the trunk must
take the unfused launches (adaf_fused_tail_in_reach) instead of refusing the batch.

Each case prints its wall time and the peak device memory; nothing skips: an allocation that fails is a failure that names the bytes."""
import collections
import contextlib
import gc
import time

import pytest
import torch

from adafocus_amd import _lib as L
from tests import strided as S
from tests.helpers import load_tool
from tests.test_hip_parity import CONV_TOL, _trunk

pytestmark = pytest.mark.gpu

D = load_tool("conv_launch_digest")
CANARY = S.CANARY_F32
GUARD = 1024              # canary words in front of and behind every strided buffer (a multiple of 4: the payload stays 16-byte aligned)
LEAN_TILES = (31, 32, 34, 39)          # fp32 DMA tiles larger than 64 x 64: the rows with the lean forms
DMA_TILES = LEAN_TILES + (33, 38)      # every row of that family: all of them have the lean position-major form
TWO_31 = 1 << 31


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _give_memory_back():
    """After every case, failed ones included (their frames are gone by now): the rest of the suite sees the memory again."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _device_memory(dev, need_bytes, what):
    """The body's allocations: a failure states the free and the needed bytes (no skip); afterwards the memory goes back to the device."""
    torch.zeros(1, device=dev)              # (the allocator's statistics exist from the first allocation on)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    free = torch.cuda.mem_get_info(dev)[0]
    t0 = time.perf_counter()
    try:
        yield
        torch.cuda.synchronize(dev)
    except torch.cuda.OutOfMemoryError as e:
        pytest.fail("%s: allocation failed with %d bytes free on the device, about %d needed (%s)" % (what, free, need_bytes, e))
    finally:
        gc.collect()
        torch.cuda.empty_cache()
    print("\n[large operands] %s: %.2f s, peak %.2f GiB allocated" % (what, time.perf_counter() - t0,
                                                                    torch.cuda.max_memory_allocated(dev) / 2.0 ** 30))


# =========================================================================================================================== single convs
# name, n, map h = w, cin, cout, k, stride, pad, shift T, residual, which operand is the large one ("x" or "out")
Conv = collections.namedtuple("Conv", "name n hw cin cout k stride pad T res large")
CONVS = {c.name: c for c in (
    Conv("A_lean_dense_1x1", 4096, 16, 64, 128, 1, 1, 0, 0, False, "x"),                 # M = 2^20
    Conv("B_shifted_conv1", 2048, 16, 256, 64, 1, 1, 0, 8, False, "x"),                  # M = 2^19, fold 32: the lean shifted K loop
    Conv("C_strided_1x1_row_gather", 1024, 32, 64, 128, 1, 2, 0, 0, False, "x"),         # reaches over the 2^20 pixels of the INPUT map
    Conv("D_3x3_position_major", 256, 8, 32, 64, 3, 1, 1, 0, False, "x"),                # M = 2^14
    Conv("E_output_and_residual", 4096, 16, 64, 64, 1, 1, 0, 0, True, "out"),            # A's rows, x dense, ldo = ldr = the pitch
)}
ALL_TILES, PM_TILES = LEAN_TILES + (33, 0), (31, 32, 0)
# (case, pitch of the large operand in floats, its byte span, side of the gate: lean form expected or not, tiles)
RUNS = [
    ("A_lean_dense_1x1", 1020, 0xff000000, True, ALL_TILES),
    ("A_lean_dense_1x1", 1024, 1 << 32, False, ALL_TILES),
    ("B_shifted_conv1", 1020, 0x7f800000, True, ALL_TILES),
    ("B_shifted_conv1", 1024, 1 << 31, False, ALL_TILES),             # the buffer form's 2 GiB: general shift form
    ("B_shifted_conv1", 2048, 1 << 32, False, ALL_TILES),
    ("C_strided_1x1_row_gather", 1020, 0xff000000, True, ALL_TILES),
    ("C_strided_1x1_row_gather", 1024, 1 << 32, False, ALL_TILES),
    ("D_3x3_position_major", 65280, 0xff000000, True, PM_TILES),
    ("D_3x3_position_major", 65536, 1 << 32, False, PM_TILES),        # the general loop, still position-major
    # E: x is dense, so the K loop stays lean on both sides; what grows past 4 GiB is what the epilogue addresses
    ("E_output_and_residual", 1020, 0xff000000, True, PM_TILES),
    ("E_output_and_residual", 1024, 1 << 32, True, PM_TILES),
    ("E_output_and_residual", 1028, 0x101000000, True, PM_TILES),
]


def _expected_form(c, lean_side, tile_run):
    """(dense, special, lean, pos_major) of the plan, by the rules tests/test_conv_plan_host.py pins for small operands."""
    lean = int(lean_side and tile_run in LEAN_TILES)
    if c.k > 1:                            # position-major: every fp32 DMA row has the lean loop, 64 x 64 included
        return (0, 0, int(lean_side and tile_run in DMA_TILES), 1)
    if c.T:
        return (1, 1, lean, 0)
    if c.stride > 1:                       # the row gather exists on the lean form only
        return (lean, 0, lean, 0)
    return (1, 0, lean, 0)


def _canary_buffer(rows, ld, dev):
    """(buf, lo): GUARD + rows * ld + GUARD words of canary, filled where they live; the payload's first row starts at word lo."""
    return torch.full((GUARD + rows * ld + GUARD,), CANARY, dtype=torch.int32, device=dev).view(torch.float32), GUARD


def _nhwc_view(buf, lo, n, hw, cols, ld):
    return buf.as_strided((n, hw, hw, cols), (hw * hw * ld, hw * ld, ld, 1), lo)


def _checksum(buf):
    w = buf.view(torch.int32)
    return int(w.sum(dtype=torch.int64).item()), int(w[::3].sum(dtype=torch.int64).item())


def _gaps_intact(buf, lo, rows, cols, ld):
    """Every word of `buf` outside the rows x cols payload still holds the canary; compared on the device, a quarter of the rows at a time."""
    w = buf.view(torch.int32)
    if bool((w[:lo] != CANARY).any()) or bool((w[lo + rows * ld:] != CANARY).any()):
        return False
    body = w[lo:lo + rows * ld].view(rows, ld)
    step = (rows + 3) // 4
    return ld == cols or not any(bool((body[r:r + step, cols:] != CANARY).any()) for r in range(0, rows, step))


def _windows(c, ld_large, rows_per_image):
    """Three (lo, hi) ranges of whole images -- whole clips under a shift: the first two, the two around byte offset 2^31 of the large
    operand (its last byte where the operand ends below that), the last two."""
    unit = c.T or 1
    span_rows = c.n * rows_per_image
    row = min(TWO_31 // (4 * ld_large), span_rows - 1)
    i = min(max(row // rows_per_image, 1), c.n - 1)
    out = []
    for lo, hi in ((0, 2), (i - 1, i + 1), (c.n - 2, c.n)):
        w = (lo // unit * unit, -(-hi // unit) * unit)
        if w not in out:
            out.append(w)
    return out


@pytest.mark.parametrize("name,pitch,span,lean_side,tiles", RUNS, ids=["%s-ld%d" % (r[0], r[1]) for r in RUNS])
def test_conv_across_the_offset_limits(dev, name, pitch, span, lean_side, tiles):
    c = CONVS[name]
    oh = (c.hw + 2 * c.pad - c.k) // c.stride + 1
    m_in, m_out = c.n * c.hw * c.hw, c.n * oh * oh
    ldx, ldo = (pitch, c.cout) if c.large == "x" else (c.cin, pitch)
    ldr = ldo if c.res else 0
    assert (m_in * ldx if c.large == "x" else m_out * ldo) * 4 == span, "the case's byte span is not what its row claims"
    need = 4 * (m_in * (ldx + c.cin) + m_out * (ldo + c.cout) * (2 if c.res else 1)) + 3 * (m_out * max(ldo - c.cout, 1)) // 4
    lib, h = L.load_library(), L.handle(dev)
    cus = lib.adaf_device_cus(h)
    kw = dict(stride=c.stride, pad=c.pad, act=S.ACT_RELU, tsm_segments=c.T, tsm_div=8)
    with torch.no_grad(), _device_memory(dev, need, "%s, pitch %d (%#x bytes)" % (name, pitch, span)):
        g = torch.Generator(device=dev).manual_seed(4000 + sorted(CONVS).index(name))
        kk = c.cin * c.k * c.k
        x = torch.randn((c.n, c.hw, c.hw, c.cin), device=dev, generator=g)      # scaled as tests/test_hip_parity.py _conv_case: CONV_TOL keeps its meaning
        w = torch.randn((c.cout, c.k, c.k, c.cin), device=dev, generator=g) * (2.0 / kk) ** 0.5
        sc = torch.rand((c.cout,), device=dev, generator=g) + 0.5
        bi = torch.randn((c.cout,), device=dev, generator=g) * 0.1
        res = torch.randn((c.n, oh, oh, c.cout), device=dev, generator=g) if c.res else None

        # ---- the dense run: the whole-output reference, itself anchored to float64 on the windows
        dense = torch.full((c.n, oh, oh, c.cout), float("nan"), device=dev)
        S.conv_call("engine", x, w, sc, bi, res, dense, **kw)
        wins = _windows(c, pitch, (c.hw * c.hw) if c.large == "x" else oh * oh)
        refs = {}
        for lo, hi in wins:
            refs[lo, hi] = S.conv_ref64(x[lo:hi], w, sc, bi, res[lo:hi] if c.res else None, **kw)
            err = (dense[lo:hi].cpu().double() - refs[lo, hi]).abs().max().item()
            print("\n[large operands] %s dense run, images %d..%d: max |err| vs float64 %.3e" % (name, lo, hi - 1, err))
            assert err < CONV_TOL, ("dense", lo, hi, err)

        # ---- the operands behind their pitches
        xbuf, xlo = _canary_buffer(m_in, ldx, dev)
        xv = _nhwc_view(xbuf, xlo, c.n, c.hw, c.cin, ldx)
        xv.copy_(x)
        obuf, olo = _canary_buffer(m_out, ldo, dev)
        ov = _nhwc_view(obuf, olo, c.n, oh, c.cout, ldo)
        rbuf = rv = None
        if c.res:
            rbuf, rlo = _canary_buffer(m_out, ldr, dev)
            rv = _nhwc_view(rbuf, rlo, c.n, oh, c.cout, ldr)
            rv.copy_(res)
        del x, res
        sums = _checksum(xbuf), _checksum(rbuf) if c.res else None

        for tile in tiles:
            p = L.ConvParams(n=c.n, h=c.hw, w=c.hw, cin=c.cin, cout=c.cout, kh=c.k, kw=c.k, stride=c.stride, pad=c.pad, act=S.ACT_RELU,
                             tsm_segments=c.T, tsm_div=8, ldx=ldx, ldo=ldo, ldr=ldr, tile=tile)
            plan = D.conv_plan(lib, p, D.plan_flags(vec_epi=True), cus)
            assert plan is not None and "refused" not in plan, (tile, plan)
            form = tuple(plan[k] for k in ("dense", "special", "lean", "pos_major"))
            assert tile == 0 or plan["tile"] == tile, (tile, plan)
            assert form == _expected_form(c, lean_side, plan["tile"]), (tile, plan["tile"], form, D.kernel_of(plan))
            if tile == 0:       # the automatic choice must land on a row that has the form under test, or the case says nothing about it
                assert plan["tile"] in (DMA_TILES if c.k > 1 else LEAN_TILES), plan

            ov.fill_(float("nan"))          # a launch that stores nothing must not pass on the previous tile's output
            S.conv_call("engine", xv, w, sc, bi, rv, ov, tile=tile, **kw)
            if not torch.equal(ov, dense):
                bad = (ov != dense).flatten(1).any(1).nonzero().flatten()
                pytest.fail("%s tile %d (%s): %d images differ from the dense run, the first at %d, the last at %d"
                            % (name, tile, D.kernel_of(plan), bad.numel(), bad[0].item(), bad[-1].item()))
            assert _gaps_intact(obuf, olo, m_out, c.cout, ldo), "%s tile %d: a word outside the output's payload lost its canary" % (name, tile)
            for lo, hi in wins:
                err = (ov[lo:hi].cpu().double() - refs[lo, hi]).abs().max().item()
                assert err < CONV_TOL, (tile, lo, hi, err)
        assert sums == (_checksum(xbuf), _checksum(rbuf) if c.res else None), "%s: an input buffer was written" % name
        del xbuf, xv, obuf, ov, rbuf, rv, dense


# ================================================================================================================================ the trunk
P = 128
MAP_BYTES = (P // 4) ** 2 * 256 * 4          # a patch's 256-channel stage-1 map: 1 MiB


def _patches(n, dev, seed):
    x = torch.randn((n, P, P, 4), device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    x[..., 3] = 0
    return x


def _window_starts(n):
    """First patches of the 16-patch windows (whole clips of 8): the first, around image 1024, around image 2048, the last."""
    return sorted({0, min(1016, n - 16), min(2040, n - 16), n - 16})


def _trunk_at(dev, n, T, math="f32", unfused_too=False):
    what = "trunk, %d patches of %d^2 (stage-1 map %#x bytes), T = %d, %s" % (n, P, n * MAP_BYTES, T, math)
    with torch.no_grad(), _device_memory(dev, 5 * n * MAP_BYTES + n * P * P * 16 + (1 << 30), what):
        net, _ = _trunk(dev, 1007 + P)
        net.set_math(math)
        net.tsm_segments = T
        x = _patches(n, dev, 52 + n + T)
        big = net.features_nhwc4(x).clone()
        assert bool(torch.isfinite(big).all()) and big.abs().max().item() > 0.1
        for s in _window_starts(n):
            small = net.features_nhwc4(x[s:s + 16].contiguous())
            assert torch.equal(big[s:s + 16], small), "patches %d..%d: %d features differ from the same patches run as a batch of 16" % (
                s, s + 15, int((big[s:s + 16] != small).sum()))
        # what the profiled pass lists is what ran: the fused tails (tile codes 91 / 92) exactly while the stage-1 map is within their reach
        trunk = net._sync()
        rows = trunk.profile(x, T, 8)
        assert len(rows) <= trunk.n_launches and all(r["tile"] > 0 or r["flops"] == 0 for r in rows), rows
        assert any(r["tile"] in (91, 92) for r in rows) == (n * MAP_BYTES < (1 << 32) - 4), sorted({r["tile"] for r in rows})
        if unfused_too:
            net.set_fusion(False)
            unfused = net.features_nhwc4(x)
            assert torch.equal(big, unfused), "fused and unfused trunks differ in %d rows" % int((big != unfused).any(1).sum())
        del net, x, big


def test_trunk_2040_patches_shifted(dev):
    """The shifted conv1s of layer1.1, layer1.2 and layer2.0 on the lean shifted K loop at 0x7f800000 bytes."""
    _trunk_at(dev, 2040, 8)


def test_trunk_2048_patches_shifted(dev):
    """The same conv1s at exactly 2^31 bytes: the general shift form; the shifted next conv1 still rides in the fused tail."""
    _trunk_at(dev, 2048, 8)


def test_trunk_4088_patches_fused_and_unfused(dev):
    """Every stage-1 lean launch and the fused tail at 0xff800000 bytes; fusion off gives the same bits."""
    _trunk_at(dev, 4088, 0, unfused_too=True)


def test_trunk_4096_patches(dev):
    """2^32 bytes: the general forms, and the fused tail beyond its reach -- the trunk takes the three launches it replaces (before
    adaf_fused_tail_in_reach was part of the trunk's decision this batch was refused: "fused bottleneck tail rejected the shape")."""
    _trunk_at(dev, 4096, 0)


def test_trunk_4096_patches_shifted(dev):
    """Both limits in one pass."""
    _trunk_at(dev, 4096, 8)


def test_trunk_4096_patches_split_bf16(dev):
    """The split-bf16 plan keeps stage 1 on the fp32 pipe's launches, fused or not: against its own small batches."""
    _trunk_at(dev, 4096, 0, math="split_bf16")
