"""The ResNet trunk's front, kernel by kernel (csrc/stem.hip: stem7x7_kernel, stem7x7_pool_kernel<4|6>, stem7x7_pool_rows_kernel with and
without its own gather, each pooled form with its fp16 store; csrc/misc_ops.hip: maxpool_kernel, maxpool_f16out_kernel), each against the
float64 statement of the same operation in tests/stem_reference.py under heads_reference's rule for single reductions
(err <= max(2^-22, 8 x spread), relative to the largest float64 entry), and form against form with torch.equal.  The fp16 stores have
no tolerance: .half() of the same form's fp32 output.  Every case prints err, spread, bound and err / bound before it asserts.

Which images see float64: stem_reference.held_images -- all of them up to 8, else the first, the last and the images of a block's second
and later rounds; every other image of a case is torch.equal on the device to a form the case held to float64."""
import functools

import pytest
import torch

from adafocus_amd import _lib, hip_ops as ops
from tests import stem_reference as SR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}                     # family -> (checks, then err / bound, err, bound, spread, tag of its worst one)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    """One line per kernel family when the module is done (shown with -s): cases, the worst err / bound and where."""
    yield
    for fam, (cases, ratio, err, bound, spread, tag) in sorted(WORST.items()):
        print("\nstem forms: %-12s %3d checks  worst err/bound %.3f (err %.3e bound %.3e spread %.3e) at %s" % (fam, cases, ratio, err, bound, spread, tag))


@functools.lru_cache(maxsize=None)
def _cus():
    return int(_lib.load_library().adaf_device_cus(_lib.handle(DEV)))


@functools.lru_cache(maxsize=None)
def _prm():
    cpu = SR.params()
    return cpu, tuple(t.to(DEV) for t in cpu)


def _check(family, tag, got, r, name):
    """got: the held images of a form, (len(idx), ...) on either device."""
    err, bound = SR.rel_err(got.float(), r, name), SR.bound_single(r.spread[name])
    print("%s %s: err %.3e  spread %.3e  bound %.3e  err/bound %.3f" % (tag, name, err, r.spread[name], bound, err / bound))
    cases, *worst = WORST.get(family, (0, -1.0, 0.0, 0.0, 0.0, ""))
    WORST[family] = (cases + 1,) + ((err / bound, err, bound, r.spread[name], tag) if err / bound > worst[0] else tuple(worst))
    assert bool(torch.isfinite(got).all()), (tag, name)
    assert err <= bound, (tag, name, err, bound)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a, b), "%s: %d of %d elements differ" % (what, int((a != b).sum()), a.numel())


def _half_checks(tag, half, full, conv):
    """The fp16 store of a pooled form: one rounding of its fp32 output, and the stand-alone fp16-store pool of the conv map."""
    assert half.dtype == torch.float16
    _same(half, full.half(), tag + " fp16 store vs .half() of the fp32 store")
    _same(half, ops.maxpool3x3s2_f16out(conv), tag + " fp16 store vs maxpool_f16out(conv map)")


def _sid(spec):
    return "n%dcus+%dbpc+%d" % spec


# ---- conv + BN + ReLU only -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,spec", SR.CONV_CASES, ids=lambda v: _sid(v) if isinstance(v, SR.N) else "P%d" % v)
def test_conv_only_kernel(p, spec):
    """stem7x7_kernel on every image (the largest case is 773 images of 16^2): the smallest maps, partial tiles on both axes, whole
    tiles, and more tiles than the 3 x CUs persistent blocks (the loop and its prefetch)."""
    (cpu, dev), n = _prm(), SR.images(spec, _cus())
    x4 = SR.patches(n, p)
    got = ops.stem7x7_bn_relu(x4.to(DEV), *dev)
    oh = SR.conv_size(p)
    assert got.shape == (n, oh, oh, 64)
    if p == 16:
        assert n > 3 * _cus()
    r = SR.reference(("conv", p, n), x4, range(n), cpu)
    _check("conv", "conv P=%d n=%d" % (p, n), got, r, "conv")
    assert bool((got[..., 1] == 0).all()), "the dead channel"


# ---- pooled tile kernels: both heights at every size ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,spec", SR.TILE_CASES, ids=lambda v: _sid(v) if isinstance(v, SR.N) else "P%d" % v)
def test_pooled_tile_kernels_both_heights(p, spec):
    (cpu, dev), cus = _prm(), _cus()
    n = SR.images(spec, cus)
    x4 = SR.patches(n, p)
    xd = x4.to(DEV)
    tag = "tile P=%d n=%d" % (p, n)
    assert ops.stem7x7_pool_form(n, p) == SR.walk_form(p, n, cus)               # n < CUs: 'tile6' where the cost rule picks 6 rows, else two launches
    conv = ops.stem7x7_bn_relu(xd, *dev)
    unfused = ops.maxpool3x3s2(conv)
    t4, t6 = ops.stem7x7_pool(xd, *dev, form="tile4"), ops.stem7x7_pool(xd, *dev, form="tile6")
    ph = SR.pool_size(SR.conv_size(p))
    assert t4.shape == (n, ph, ph, 64)
    _same(t4, t6, tag + " 4-row vs 6-row tiles")
    _same(t4, unfused, tag + " tiles vs maxpool3x3s2(stem7x7_bn_relu)")
    _same(ops.stem7x7_pool(xd, *dev, form="unfused"), unfused, tag + " the unfused form")
    tiles = -(-ph // 4) * -(-ph // 8)                                            # 4-row tiles per image (P = 32: two at either height)
    idx = SR.held_images(n, max(2 * cus // tiles, 1))
    r = SR.reference(("tile", p, n), x4, idx, cpu)
    _check("conv", tag, conv[idx], r, "conv")
    _check("tile4", tag + " 4 rows (picked: %d)" % SR.tile_rows(p), t4[idx], r, "pool")
    _check("tile6", tag + " 6 rows (picked: %d)" % SR.tile_rows(p), t6[idx], r, "pool")
    _check("maxpool", tag + " unfused", unfused[idx], r, "pool")
    for form, full in (("tile4", t4), ("tile6", t6), ("unfused", unfused)):
        _half_checks("%s %s" % (tag, form), ops.stem7x7_pool(xd, *dev, form=form, half=True), full, conv)


# ---- strip kernel -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,spec", SR.STRIP_CASES, ids=lambda v: _sid(v) if isinstance(v, SR.N) else "P%d" % v)
def test_strip_kernel_every_image_count(p, spec):
    """One image; CUs + 3 (BPC = 1: three blocks own a second image); 2 x CUs x BPC + 5 (five blocks own three images, the rest two).
    Every image is torch.equal to the tile form's; the first, the last and the images of every block round are held to float64."""
    (cpu, dev), cus, bpc = _prm(), _cus(), SR.strip_bpc(p)
    n = SR.images(spec, cus, bpc)
    x4 = SR.patches(n, p)
    xd = x4.to(DEV)
    tag = "strip P=%d n=%d" % (p, n)
    strip, used = ops.stem7x7_pool(xd, *dev, form="strip", return_form=True)
    assert used == "strip" and strip.shape == (n, p // 4, p // 4, 64)
    tile = ops.stem7x7_pool(xd, *dev, form="tile%d" % SR.tile_rows(p))
    _same(strip, tile, tag + " strips vs tiles")
    grid = min(n, cus * bpc)
    idx = SR.held_images(n, grid)
    if spec.bpc_cus:
        assert {i // grid for i in idx} == {0, 1, 2}                              # a block's first, second and third image
    r = SR.reference(("strip", p, n), x4, idx, cpu)
    _check("strip", tag, strip[idx], r, "pool")
    _check("tile%d" % SR.tile_rows(p), tag + " (tile form)", tile[idx], r, "pool")
    if not spec.bpc_cus:                                                          # the fp16 store at one small and one multi-image n
        _half_checks(tag, ops.stem7x7_pool(xd, *dev, form="strip", half=True), strip, ops.stem7x7_bn_relu(xd, *dev))


def test_forced_strip_form_refuses_other_sizes():
    (_, dev) = _prm()
    for p in (32, 100, 160):
        x = SR.patches(2, p).to(DEV)
        with pytest.raises(_lib.AdafError, match="strip kernel exists for patches of 64, 96, 128 and 144"):
            ops.stem7x7_pool(x, *dev, form="strip")
    fr = SR.frames(2, 112, 112).to(DEV)
    act = torch.zeros((2, 2), device=DEV)
    with pytest.raises(_lib.AdafError, match="strip kernel exists"):
        ops.stem7x7_pool_frames(fr, act, 100, *dev)
    with pytest.raises(_lib.AdafError, match="larger than the frames' height"):
        ops.stem7x7_pool_frames(fr, act, 128, *dev)
    with pytest.raises(_lib.AdafError, match="width 96 < height 112"):
        ops.stem7x7_pool_frames(fr[..., :96].contiguous(), act, 64, *dev)
    with pytest.raises(ValueError):                                               # two actions for three frames
        ops.stem7x7_pool_frames(SR.frames(3, 112, 112).to(DEV), act, 64, *dev)


# ---- the gathering strip kernel -------------------------------------------------------------------------------------------------------------------------
def _pixel_major(frames_dev, lane3):
    pad = torch.full_like(frames_dev[:, :1], lane3)
    return torch.cat([frames_dev, pad], 1).permute(0, 2, 3, 1).contiguous()


def _gpu_gather(src, act, c):
    per = c.nf // c.fpa
    if ops.pixel_major(src):
        return torch.cat([ops.crop_gather_nhwc4(src, act[g * per:(g + 1) * per].contiguous(), c.p, c.fpa) for g in range(c.k)])
    return torch.cat([ops.crop_gather(src, act[g * per:(g + 1) * per].contiguous(), c.p, c.fpa, ops.LAYOUT_NHWC4) for g in range(c.k)])


@pytest.mark.parametrize("layout", ["planar", "pixel_major"])
@pytest.mark.parametrize("c", SR.GATHER_CASES, ids=lambda c: "P%d-H%d-W%d-nf%d-fpa%d-k%d-l3_%g" % (tuple(c[:6]) + (c.lane3,)))
def test_gathering_strip_kernel(c, layout):
    (cpu, dev) = _prm()
    fr, act = SR.frames(c.nf, c.h, c.w), SR.gather_actions(c)
    frd, actd = fr.to(DEV), act.to(DEV)
    src = frd if layout == "planar" else _pixel_major(frd, c.lane3)
    n = c.k * c.nf
    tag = "gather %s P=%d H=%d W=%d nf=%d fpa=%d k=%d" % (layout, c.p, c.h, c.w, c.nf, c.fpa, c.k)
    got = ops.stem7x7_pool_frames(src, actd, c.p, *dev, frames_per_action=c.fpa)
    assert got.shape == (n, c.p // 4, c.p // 4, 64)
    patches = _gpu_gather(src, actd, c)
    want_cpu = SR.gather(fr, act, c.p, c.fpa, c.k)
    _same(patches[..., :3].cpu(), want_cpu[..., :3], tag + " crop_gather vs get_patch on the CPU")
    if c.lane3:
        if layout == "planar":
            patches[..., 3] = c.lane3
        assert bool((patches[..., 3] == c.lane3).all())
    strip = ops.stem7x7_pool(patches, *dev, form="strip")
    _same(got, strip, tag + " gathering strips vs gather + strips")
    _same(got, ops.stem7x7_pool(patches, *dev, form="tile%d" % SR.tile_rows(c.p)), tag + " gathering strips vs gather + tiles")
    r = SR.reference(("gather", c), want_cpu, range(n), cpu)
    _check("gather " + layout, tag, got, r, "pool")
    if c.lane3:                                                                   # lane 3 is dropped: the lane-3-zero run, bit for bit
        clean = patches.clone()
        clean[..., 3] = 0
        _same(got, ops.stem7x7_pool(clean, *dev, form="strip"), tag + " lane 3 = %g vs lane 3 = 0 (patches)" % c.lane3)
        _same(ops.stem7x7_pool(patches, *dev, form="tile4"), ops.stem7x7_pool(clean, *dev, form="tile4"), tag + " lane 3 (4-row tiles)")
        _same(ops.stem7x7_bn_relu(patches, *dev), ops.stem7x7_bn_relu(clean, *dev), tag + " lane 3 (conv only)")
        if layout == "pixel_major":
            _same(got, ops.stem7x7_pool_frames(_pixel_major(frd, 0.0), actd, c.p, *dev, frames_per_action=c.fpa), tag + " lane 3 of the frames")
    _half_checks(tag, ops.stem7x7_pool_frames(src, actd, c.p, *dev, frames_per_action=c.fpa, half=True), got, ops.stem7x7_bn_relu(patches, *dev))


def test_gathered_origins_beyond_the_lds_table():
    """A strip block keeps the window origins of its first 32 images in LDS and recomputes the later ones: 32 x CUs x BPC + 256 patches of
    64^2 from 8 frames give blocks a 33rd image.  The action sets repeat with period 4 (32 distinct patches), so every group of 32 images
    must equal the first on the device, and the first equals the 32-patch run, which is held to float64."""
    (cpu, dev), cus, p, nf, hw = _prm(), _cus(), 64, 8, 101
    bpc = SR.strip_bpc(p)
    n = SR.MAXO * cus * bpc + 256
    assert n % 32 == 0 and -(-n // (cus * bpc)) > SR.MAXO
    fr = SR.frames(nf, hw, hw)
    base = SR.edge_actions(hw - p, 32, 8600)                                       # 4 action sets over the 8 frames
    frd, based = fr.to(DEV), base.to(DEV)
    small = ops.stem7x7_pool_frames(frd, based, p, *dev)
    want_cpu = SR.gather(fr, base, p, 1, 4)
    r = SR.reference(("maxo", p, hw), want_cpu, range(32), cpu)
    _check("gather planar", "gather 32 patches (origins from the LDS table)", small, r, "pool")
    big = ops.stem7x7_pool_frames(frd, based.repeat(n // 32, 1), p, *dev)
    assert big.shape == (n, 16, 16, 64)
    groups = big.view(n // 32, 32, 16, 16, 64)
    bad = (groups != groups[:1]).flatten(1).any(1)
    assert not bool(bad.any()), "groups %s differ from the first (images past the origin table start at %d)" % (
        bad.nonzero().flatten()[:8].tolist(), SR.MAXO * cus * bpc)
    _same(groups[0], small, "the first 32 of %d gathered images vs the 32-patch run" % n)
    _check("gather planar", "gather %d patches, the last 32 (origins recomputed past the table)" % n, groups[-1], r, "pool")


# ---- the automatic form -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", SR.AUTO_N, ids=_sid)
@pytest.mark.parametrize("p", SR.AUTO_SIZES)
def test_automatic_form_is_the_walks_and_reports_itself(p, spec):
    (cpu, dev), cus = _prm(), _cus()
    n = SR.images(spec, cus)
    x4 = SR.patches(n, p)
    xd = x4.to(DEV)
    tag = "auto P=%d n=%d" % (p, n)
    out, used = ops.stem7x7_pool(xd, *dev, return_form=True)
    assert used == ops.stem7x7_pool_form(n, p) == SR.walk_form(p, n, cus), (tag, used)
    _same(out, ops.stem7x7_pool(xd, *dev, form=used), tag + " vs the forced '%s' run" % used)
    _same(out, ops.stem7x7_pool(xd, *dev, form="tile4"), tag + " vs the forced 4-row tiles")       # (never the automatic form)
    idx = SR.held_images(n, cus if used == "strip" else 0)
    r = SR.reference(("auto", p, n), x4, idx, cpu)
    _check("auto " + used, tag + " (%s)" % used, out[idx], r, "pool")


@pytest.mark.parametrize("p,spec", [(96, SR.N(plus=8)), (128, SR.N(cus=1, plus=3))], ids=["P96-tile6", "P128-strip"])
def test_trunk_features_do_not_depend_on_the_stem_form(p, spec):
    """The walk asks the same plan function as the export: with fusion on it takes the fused stem, with fusion off two launches, and the
    2048-d features are the same bits (tests/test_hip_parity_r5.py does the rest)."""
    from adafocus_amd.resnet import resnet50
    from tests.helpers import synth_sd
    n = SR.images(spec, _cus())
    assert ops.stem7x7_pool_form(n, p) in ("tile6", "strip")
    net = resnet50(num_classes=200).eval()
    net.load_state_dict(synth_sd("ACT", 1007 + p, "focuser.net.", keep_prefix=False), strict=True)
    net = net.to(DEV)
    x = SR.patches(n, p).to(DEV)
    with torch.no_grad():
        fused = net.features_nhwc4(x).clone()
        try:
            net._sync().set_fusion(0)
            plain = net.features_nhwc4(x).clone()
        finally:
            net._sync().set_fusion(1)
    assert bool(torch.isfinite(fused).all()) and fused.abs().max().item() > 0.1
    _same(fused, plain, "trunk features P=%d n=%d, fusion on vs off" % (p, n))


# ---- the stand-alone max-pools ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,c", SR.MAXPOOL_SHAPES)
def test_standalone_maxpools_equal_max_pool2d(h, w, c):
    for kind in SR.MAXPOOL_KINDS:
        x = SR.maxpool_input(h, w, c, kind)
        want = SR.maxpool(x)
        got = ops.maxpool3x3s2(x.to(DEV))
        tag = "maxpool %dx%dx%d %s" % (h, w, c, kind)
        _same(got.cpu(), want, tag)
        _same(ops.maxpool3x3s2_f16out(x.to(DEV)).cpu(), want.half(), tag + " fp16 store")
        if kind == "negative":
            assert bool((got < 0).all()), tag + ": the padding won"
        if kind == "neginf":
            assert bool(torch.isinf(got[-1]).all()) and not bool(torch.isnan(got).any())
