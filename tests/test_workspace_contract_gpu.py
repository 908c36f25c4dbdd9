"""The workspace contract of the C ABI (include/adafocus.h Conventions, DESIGN.md 2.1 "The workspace contract"): every entry point that takes a caller-owned workspace is
called through ctypes with EXACTLY the bytes its *_workspace_bytes query returned, inside a NaN-canary allocation (tests/strided.py
guarded_workspace: max(need, 1 MiB) of canary on either side).  Every case asserts
  (a) the exact size is accepted: ADAF_OK, finite outputs (and no GRU scan time-out);
  (b) both guards of the workspace, and of every output, are intact after the call;
  (c) the outputs do not depend on what the workspace held: NaN canary, zeros and the bytes a preceding call on OTHER inputs left there give
      torch.equal outputs;
  (d) four bytes less are refused with ADAF_E_NOMEM before anything is launched: outputs and workspace stay all canary;
  (e) whole networks: the outputs equal the public Python wrapper's, torch.equal (that output is tied to the oracle elsewhere);
  (f) once per family: a workspace at the documented minimum alignment (16 bytes) gives the same bits, one below it is ADAF_E_LAYOUT.
No tolerance appears in this file.  Three cases the carving's halving paths need (>= 512 frames) take workspaces above 64 MiB; every other one
stays far below."""
import collections
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from adafocus_amd import _lib as L
from tests import strided as S
from tests.helpers import rnd

pytestmark = pytest.mark.gpu

OK, E_BADARG, E_LAYOUT, E_NOMEM = 0, -1, -2, -6
ACCEPTED = collections.Counter()          # family -> cases whose exact-size workspace was accepted and passed (a) - (d)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _tally():
    """One log line when the module is done: the accepted cases per family of whatever selection ran (shown with -s)."""
    yield
    print("\nworkspace contract: exact-size cases accepted per family: " + ", ".join("%s %d" % kv for kv in sorted(ACCEPTED.items())))


@pytest.fixture(scope="module")
def ops():
    from adafocus_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------------------------ the harness
def _outs(spec, dev):
    """spec: name -> shape or (shape, dtype); every output is a dense view inside its own canary allocation."""
    o = {}
    for name, sp in spec.items():
        shape, dt = sp if isinstance(sp[0], (tuple, list)) else (sp, torch.float32)
        cols = shape[-1]
        o[name] = S.guarded(tuple(shape[:-1]) or (1,), cols, cols, S.lead_for(cols), cols + 8, dt, dev)
    return o


def _call(call, spec, dev, need, fill, alt=False, short=0, offset=0):
    buf, ws = S.guarded_workspace(need, dev, fill=fill, offset_bytes=offset)
    outs = _outs(spec, dev)
    rc = call(ws, need - short, {k: v[1] for k, v in outs.items()}, alt)
    torch.cuda.synchronize()
    return rc, buf, ws, outs


def _accepted(tag, rc, buf, ws, outs, need):
    assert rc == OK, "%s: exact workspace of %d bytes refused, rc %d" % (tag, need, rc)
    S.assert_workspace_intact(buf, ws, tag + " workspace", need)
    S.assert_guards_intact(buf, ws, tag + " workspace")
    got = {}
    for name, (ob, ov) in outs.items():
        S.assert_guards_intact(ob, ov, "%s %s" % (tag, name))
        got[name] = S.payload(ov)
        assert bool(torch.isfinite(got[name].float()).all()), "%s %s: %d non-finite values (a workspace word was read before it was written)" % (
            tag, name, int((~torch.isfinite(got[name].float())).sum()))
    return got


def _untouched(tag, buf, outs):
    assert S.is_all_canary(buf), "%s: the workspace was written by a refused call" % tag
    for name, (ob, _) in outs.items():
        assert not bool((ob.view(torch.int16 if ob.dtype == torch.float16 else torch.int32) !=
                         (S.CANARY_F16 if ob.dtype == torch.float16 else torch.tensor(S.CANARY_F32, dtype=torch.int64).to(torch.int32).item())).any()), \
            "%s: output %s was written by a refused call" % (tag, name)


def contract(family, tag, dev, need, call, spec, wrapper=None, align=False, max_bytes=64 << 20):
    """Properties (a) - (d) [+ (e) with `wrapper` = name -> expected tensor, + (f) with align].  call(ws, nbytes, outs, alt) -> rc enqueues the
    entry point on the primary (alt = False) or the other (alt = True) inputs."""
    need = int(need)
    assert 0 < need <= max_bytes, (tag, need)
    rc, buf, ws, outs = _call(call, spec, dev, need, "nan")
    first = _accepted(tag + " [NaN workspace]", rc, buf, ws, outs, need)
    rc, sbuf, stale, souts = _call(call, spec, dev, need, "nan", alt=True)          # another call's leftovers
    other = _accepted(tag + " [other inputs]", rc, sbuf, stale, souts, need)
    for what, fill in (("zero workspace", "zero"), ("stale workspace", stale)):
        rc, b2, w2, o2 = _call(call, spec, dev, need, fill)
        again = _accepted("%s [%s]" % (tag, what), rc, b2, w2, o2, need)
        for k in first:
            assert torch.equal(again[k], first[k]), "%s: %s differs between a NaN and a %s in %d elements (a word is read that this call did not write)" % (
                tag, k, what, int((again[k] != first[k]).sum()))
    # (after the comparison above, whose message says more: the leftovers must come from a call that computed something else)
    assert any(not torch.equal(other[k], first[k]) for k in first), "%s: the other inputs give the same outputs" % tag
    short = 4 if need % 4 == 0 else 1
    rc, b3, w3, o3 = _call(call, spec, dev, need, "nan", short=short)
    assert rc == E_NOMEM, "%s: %d bytes (need %d) gave rc %d, ADAF_E_NOMEM expected" % (tag, need - short, need, rc)
    _untouched(tag + " [short workspace]", b3, o3)
    if wrapper is not None:
        for k, want in wrapper().items():
            assert torch.equal(first[k], want.reshape(first[k].shape)), "%s: %s differs from the Python wrapper's in %d elements" % (
                tag, k, int((first[k] != want.reshape(first[k].shape)).sum()))
    if align:
        rc, b4, w4, o4 = _call(call, spec, dev, need, "nan", offset=16)
        assert w4.data_ptr() % 256 == 16
        at16 = _accepted(tag + " [16-byte aligned workspace]", rc, b4, w4, o4, need)
        for k in first:
            assert torch.equal(at16[k], first[k]), "%s: %s differs at a 16-byte aligned workspace" % (tag, k)
        for off in (4, 8):
            rc, b5, w5, o5 = _call(call, spec, dev, need, "nan", offset=off)
            assert rc == E_LAYOUT, "%s: a workspace %d bytes off a 16-byte boundary gave rc %d, ADAF_E_LAYOUT expected" % (tag, off, rc)
            _untouched(tag + " [misaligned workspace]", b5, o5)
    ACCEPTED[family] += 1
    return first


def _option(key, value):
    """The option for the block, or the library's default when `value` is 0."""
    return L.option(key, value) if value else contextlib.nullcontext()


def _x4(n, p, seed, dev):
    x4 = torch.zeros((n, p, p, 4), device=dev)
    x4[..., :3] = rnd((n, p, p, 3), seed).to(dev)
    return x4


# ------------------------------------------------------------------------------------------------------------------ ResNet trunk
_TRUNKS = {}


def _trunk(dev, math, arch="resnet50"):
    if (math, arch) not in _TRUNKS:
        from adafocus_amd import resnet, synth
        net = getattr(resnet, arch)(num_classes=200).eval()
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()})
        net.set_math(math)
        _TRUNKS[(math, arch)] = net.to(dev)
    return _TRUNKS[(math, arch)]


TCase = collections.namedtuple("TCase", "api p n tsm math place fusion lat arch frames align", defaults=(0, "f32", "blockres", 1, -1, "resnet50", None, False))
# five slabs ('blockres') or six ('block'); the slab is max(stem map, 256-channel map): equal at even stem sizes, the 256-channel map wins at odd
# ones (P = 98: 49 -> 25; P = 100: 50 -> 25 ties); f16 reuses the fp32 slabs
T_CASES = [TCase("forward", p, n, math=m) for m in ("f32", "f16", "split_bf16") for p in (32, 64, 96, 98, 100) for n in (1, 6)]
T_CASES += [TCase("forward", 64, 16, 8, m, place) for m in ("f32", "f16", "split_bf16") for place in ("blockres", "block")]
T_CASES += [
    TCase("forward", 98, 8, 8, "f32", "block"),                       # six slabs at an odd stem size
    TCase("forward", 96, 6, fusion=0), TCase("forward", 100, 6, fusion=0), TCase("forward", 96, 6, math="f16", fusion=0),
    TCase("forward", 96, 6, fusion=2),                                # the fused stem + stage-1 tails forced on a small batch
    TCase("forward", 96, 6, lat=0), TCase("forward", 64, 1, lat=0),   # never the small-batch form
    TCase("forward", 96, 6, align=True),
    TCase("map", 96, 6), TCase("map", 100, 3), TCase("map", 64, 1, math="f16"), TCase("map", 64, 8, 8, "f32", "block"),
    TCase("map", 96, 4, math="split_bf16"),
    TCase("frames", 100, 3, frames=("nchw", 128)),                    # no strip stem at 100^2: the gather goes into a slab
    TCase("frames", 96, 6, frames=("nchw", 128)),                     # fewer images than CUs: the same fall-back at a strip-stem size
    TCase("frames", 96, 4, frames=("nhwc4", 112)),                    # pixel-major frames
    TCase("frames", 100, 8, 8, "f32", "block", frames=("nchw", 112)),  # the gather slab beside the sixth (shifted) slab
    TCase("frames", 64, 4, math="f16", frames=("nchw", 96)),
    TCase("forward", 64, 8, 8, arch="resnet101"), TCase("frames", 64, 8, 8, arch="resnet101", frames=("nchw", 96)),
]


def _tid(c):
    return "%s-p%d-n%d-t%d-%s-%s-fuse%d-lat%d-%s%s%s" % (c.api, c.p, c.n, c.tsm, c.math, c.place, c.fusion, c.lat, c.arch,
                                                        ("-%s%d" % c.frames) if c.frames else "", "-align" if c.align else "")


@pytest.mark.parametrize("c", T_CASES, ids=_tid)
def test_resnet_trunk_workspace(dev, c):
    net = _trunk(dev, c.math, c.arch)
    net.tsm_place = c.place
    net.set_fusion(c.fusion)
    trunk = net._sync()
    lib = trunk._lib
    trunk.set_latency_rows(c.lat)
    try:
        n, p, div = c.n, c.p, 8
        need = lib.adaf_resnet50_workspace_bytes(trunk._net, n, p)
        slabs = 6 if c.place == "block" else 5
        s1 = (p + 6 - 7) // 2 + 1
        s2 = (s1 + 2 - 3) // 2 + 1
        assert need == slabs * n * max(s1 * s1 * 64, s2 * s2 * 256) * 4
        spec = {"feat": (n, 2048)}
        if c.api == "frames":
            layout, hw = c.frames
            fr = [rnd((n, 3, hw, hw), 900 + i).to(dev) for i in (0, 1)]
            if layout == "nhwc4":
                from adafocus_amd.utils import nchw_to_nhwc4
                fr = [nchw_to_nhwc4(f).contiguous() for f in fr]
            act = torch.from_numpy(np.random.Generator(np.random.PCG64(903)).random((n, 2), dtype=np.float32)).to(dev)
            code = L.LAYOUT_NHWC4 if layout == "nhwc4" else L.LAYOUT_NCHW

            def call(ws, nb, o, alt):
                return lib.adaf_resnet50_forward_frames(trunk._net, L.ptr(fr[alt]), code, n, hw, hw, L.ptr(act), n, 1, p, c.tsm, div, L.ptr(o["feat"]), 2048,
                                                        L.ptr(ws), nb, L.stream_ptr())

            def wrapper():
                return {"feat": trunk.forward_frames(fr[0], act, p, 1, c.tsm, div).clone()}
        else:
            x = [_x4(n, p, 910 + i, dev) for i in (0, 1)]
            if c.api == "map":
                s = lib.adaf_resnet50_map_size(p)
                spec["fmap"] = (n, s, s, 2048)

                def call(ws, nb, o, alt):
                    return lib.adaf_resnet50_forward_map(trunk._net, L.ptr(x[alt]), n, p, c.tsm, div, L.ptr(o["fmap"]), L.ptr(o["feat"]), 2048, L.ptr(ws), nb,
                                                         L.stream_ptr())

                def wrapper():
                    fm, ft = trunk.forward_map(x[0], c.tsm, div)
                    return {"fmap": fm.clone(), "feat": ft.clone()}
            else:
                def call(ws, nb, o, alt):
                    return lib.adaf_resnet50_forward(trunk._net, L.ptr(x[alt]), n, p, c.tsm, div, L.ptr(o["feat"]), 2048, L.ptr(ws), nb, L.stream_ptr())

                def wrapper():
                    return {"feat": trunk.forward(x[0], c.tsm, div).clone()}
        with torch.no_grad():
            contract("resnet trunk", _tid(c), dev, need, call, spec, wrapper, align=c.align)
    finally:
        trunk.set_latency_rows(-1)
        net.tsm_place = "blockres"
        net.set_fusion(True)
        net._sync()


@pytest.mark.parametrize("p,n,tsm", [(96, 6, 0), (64, 8, 8)])
def test_resnet_trunk_profiled_workspace(dev, p, n, tsm):
    """adaf_resnet50_forward_profiled: the same walk with an event record in front of every launch and the pool as a launch of its own."""
    net = _trunk(dev, "f32")
    trunk = net._sync()
    lib = trunk._lib
    k = lib.adaf_resnet50_launch_count(trunk._net)
    need = lib.adaf_resnet50_workspace_bytes(trunk._net, n, p)
    x = [_x4(n, p, 920 + i, dev) for i in (0, 1)]
    tiles = []

    def call(ws, nb, o, alt):
        ms, fl, by, tl = (C.c_float * k)(), (C.c_double * k)(), (C.c_double * k)(), (C.c_int * k)(*([-1] * k))
        rc = lib.adaf_resnet50_forward_profiled(trunk._net, L.ptr(x[alt]), n, p, tsm, 8, L.ptr(o["feat"]), 2048, L.ptr(ws), nb, L.stream_ptr(), ms, fl, by, tl)
        tiles.append(sum(1 for i in range(k) if tl[i] != -1))
        return rc
    with torch.no_grad():
        contract("resnet trunk", "profiled-p%d-n%d-t%d" % (p, n, tsm), dev, need, call, {"feat": (n, 2048)},
                 lambda: {"feat": trunk.forward(x[0], tsm, 8).clone()})
    assert tiles[0] > 20 and tiles[4] == 0, tiles          # the accepted runs launched the whole plan, the refused one nothing


# ------------------------------------------------------------------------------------------------------------------ MobileNetV2
_GL = {}


def _glancer(dev):
    if "net" not in _GL:
        from adafocus_amd.mobilenet import mobilenet_v2
        from tests.helpers import synth_sd
        net = mobilenet_v2().eval()
        net.load_state_dict({k: v for k, v in synth_sd("ACT", 505, "glancer.net.", keep_prefix=False).items() if not k.startswith("classifier")}, strict=False)
        _GL["net"] = net.to(dev)
    return _GL["net"]


MCase = collections.namedtuple("MCase", "size n tsm div fusion strip chunk align big", defaults=(0, 8, True, 1, 0, False, False))
M_CASES = [MCase(s, 3, fusion=f) for s in (32, 56, 64, 96) for f in (True, 9, False)]
M_CASES += [MCase(s, 2, fusion=f, strip=st) for s in (56, 224) for st in (0, 1) for f in (True, 9)] + [MCase(224, 2, fusion=False)]
M_CASES += [MCase(32, n, chunk=4) for n in (4, 5, 8, 9, 12)]           # one chunk, a pair, a pair + a ragged tail... three chunks
M_CASES += [MCase(64, 9, chunk=4, fusion=5)]                           # bit 2: one chunk at a time in the first half of the same workspace
M_CASES += [MCase(s, 8, 4, d, f, chunk=ch) for s in (32, 64) for d in (8, 4) for f in (True, False) for ch in (5, 3)]   # chunk rounds down to 4 / is raised to T
M_CASES += [MCase(224, 4, 4, d, True, st) for d in (8, 4) for st in (0, 1)]     # shift_div 4: the shift materialised into bufE / bufD
M_CASES += [MCase(96, 3, align=True)]
M_CASES += [MCase(32, 520, 8, chunk=1024, big=True), MCase(32, 513, chunk=1024, big=True)]     # 512 <= n <= chunk: halves of 264 + 256 (whole clips), 257 + 256
M_CASES += [MCase(32, 520, 8, big=True)]                               # the default chunk of 512: 512 + 8 frames side by side
# odd maps (113: 57, 29, 15, 8, 4; 196: 98, 49, 25, 13, 7) and strip blocks handing over to tile kernels (168: 84, 42, 21, 11, 6): where cdiv_out and a
# hand-written maximum could part ways (tests/test_glancer_sizes_gpu.py has the plans of these sizes)
M_CASES += [MCase(s, 2, strip=st) for s in (113, 168, 196) for st in (0, 1)] + [MCase(168, 4, 2, 8)]


def _mid(c):
    return "s%d-n%d-t%d-div%d-fuse%s-strip%d-chunk%d%s" % (c.size, c.n, c.tsm, c.div, int(c.fusion), c.strip, c.chunk, "-align" if c.align else "")


@pytest.mark.parametrize("c", M_CASES, ids=_mid)
def test_mobilenetv2_workspace(dev, c):
    net = _glancer(dev)
    net._engine.fusion = c.fusion
    eng = net._engine.sync()
    lib = eng._lib
    try:
        with L.option("mb_strip", c.strip), _option("mbv2_chunk", c.chunk):
            n, size = c.n, c.size
            need = lib.adaf_mobilenetv2_workspace_bytes(eng._net, n, size, c.tsm)
            x = [_x4(n, size, 930 + i, dev) for i in (0, 1)]
            fs = size
            for _ in range(5):
                fs = (fs - 1) // 2 + 1
            spec = {"fmap": (n, fs, fs, 1280), "fvec": (n, 1280)}

            def call(ws, nb, o, alt):
                return lib.adaf_mobilenetv2_forward(eng._net, L.ptr(x[alt]), n, size, c.tsm, c.div, L.ptr(o["fmap"]), L.ptr(o["fvec"]), 1280, L.ptr(ws), nb,
                                                    L.stream_ptr())

            def wrapper():
                fm, fv = eng.forward(x[0], c.tsm, c.div)
                return {"fmap": fm.clone(), "fvec": fv.clone()}
            with torch.no_grad():
                contract("mobilenetv2", _mid(c), dev, need, call, spec, wrapper, align=c.align, max_bytes=(512 << 20) if c.big else (64 << 20))
    finally:
        net._engine.fusion = True
        net._engine.sync()


# ------------------------------------------------------------------------------------------------------------------ EfficientNet
_EF = {}


def _effnet(dev, name, dtype, image_size):
    key = (name, dtype, image_size)
    if key not in _EF:
        from adafocus_amd import synth
        from adafocus_amd.efficientnet import EfficientNet
        m = EfficientNet.from_name(name, num_classes=200, image_size=image_size, dtype=dtype).eval()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
        _EF[key] = m.to(dev)
    return _EF[key]


ECase = collections.namedtuple("ECase", "name dtype size n pad chunk upto want_map align big", defaults=("native", 0, -1, False, False, False))
E_CASES = [ECase(nm, dt, s, 3, pad) for nm in ("efficientnet-b0", "efficientnet-b3") for dt in ("f32", "f16") for s in (64, 75, 100) for pad in ("native", None)]
E_CASES += [ECase("efficientnet-b0", dt, 64, n, chunk=4) for dt in ("f32", "f16") for n in (3, 4, 5, 9)]      # one chunk, a pair, a pair + a tail
E_CASES += [ECase("efficientnet-b3", "f16", 75, 9, None, chunk=4), ECase("efficientnet-b0", "f16", 64, 3, want_map=True),
            ECase("efficientnet-b0", "f32", 100, 2, None, want_map=True), ECase("efficientnet-b0", "f16", 64, 3, align=True)]
# upto_block: "whole" = the block behind the first whole-image block, "fused" = the block behind the first fused-expand block (fp16 storage)
E_CASES += [ECase("efficientnet-b3", "f16", 100, 3, None, upto="whole"), ECase("efficientnet-b3", "f16", 100, 3, None, upto="fused"),
            ECase("efficientnet-b0", "f32", 64, 3, upto=3), ECase("efficientnet-b0", "f16", 75, 3, None, upto=0)]
E_CASES += [ECase("efficientnet-b0", "f16", 64, 513, big=True)]        # >= 512 patches that fit one chunk: two half chunks side by side


def _eid(c):
    return "%s-%s-s%d-n%d-pad%s-chunk%d-upto%s-map%d%s" % (c.name[-2:], c.dtype, c.size, c.n, c.pad, c.chunk, c.upto, c.want_map, "-align" if c.align else "")


def _upto(eng, c):
    if not isinstance(c.upto, str):
        return c.upto
    pad = int(eng.pad_size)
    whole, fused = eng.whole_blocks(c.size, pad), eng.fused_expand_blocks(c.size, pad)
    assert whole > 0 and fused > 0, (whole, fused)
    blocks = eng.blocks()
    # the whole-image blocks are the tail of the network (small maps), the fused-expand blocks the narrow-input ones in front of them
    first_fused = next(i for i, b in enumerate(blocks) if b["expand"] != 1 and b["cin"] <= 64)
    return (len(blocks) - whole + 1) if c.upto == "whole" else first_fused + 1


@pytest.mark.parametrize("c", E_CASES, ids=_eid)
def test_effnet_workspace(dev, c):
    m = _effnet(dev, c.name, c.dtype, c.pad)
    eng = m.engine()
    lib = eng._lib
    pad = int(eng.pad_size)
    with _option("effnet_chunk", c.chunk):
        n, size = c.n, c.size
        need = lib.adaf_effnet_workspace_bytes(eng._net, n, size, pad)
        x = [_x4(n, size, 950 + i, dev) * 0.5 for i in (0, 1)]
        upto = _upto(eng, c)
        f = eng.feature_dim
        if upto >= 0:
            with torch.no_grad():
                want = eng.forward_blocks(x[0], upto, pad).clone()
            spec = {"block": (tuple(want.shape), want.dtype)}

            def call(ws, nb, o, alt):
                return lib.adaf_effnet_forward(eng._net, L.ptr(x[alt]), n, size, pad, upto, L.ptr(o["block"]), None, None, 0, L.ptr(ws), nb, L.stream_ptr())

            def wrapper():
                return {"block": want}
        else:
            spec = {"fvec": (n, f)}
            if c.want_map:
                fs = eng.out_size(size, pad)
                spec["fmap"] = (n, fs, fs, f)

            def call(ws, nb, o, alt):
                return lib.adaf_effnet_forward(eng._net, L.ptr(x[alt]), n, size, pad, -1, None, L.ptr(o.get("fmap")), L.ptr(o["fvec"]), f, L.ptr(ws), nb,
                                               L.stream_ptr())

            def wrapper():
                fm, fv = eng.forward(x[0], pad, want_map=c.want_map)
                return dict(fvec=fv.clone(), **({"fmap": fm.clone()} if c.want_map else {}))
        with torch.no_grad():
            contract("effnet", _eid(c), dev, need, call, spec, wrapper, align=c.align, max_bytes=(512 << 20) if c.big else (64 << 20))


# (k, stride, size, c) from tests/test_effnet.py test_dwconv_same_vs_torch: a 3 x 3 map, a 5 x 5 window at stride 2, a large map, a tiny-map 5 x 5
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("k,stride,size,c", [(3, 1, 3, 2304), (5, 2, 9, 816), (3, 2, 72, 144), (5, 1, 4, 64)])
def test_dwconv_same_pool_workspace(dev, ops, k, stride, size, c, dtype):
    lib, h = L.load_library(), L.handle(dev)
    n = 11 if size <= 9 else 3
    dt = L.DTYPE_F16 if dtype == torch.float16 else L.DTYPE_F32
    x = [rnd((n, size, size, c), 970 + i).to(dev).to(dtype) for i in (0, 1)]
    wk = ops.pack_dw_weight_kxk(rnd((c, 1, k, k), 972, 0.3).to(dev))
    scale, bias = (rnd((c,), 973, 0.2) + 1.0).to(dev), rnd((c,), 974, 0.1).to(dev)
    o = -(-size // stride)
    need = lib.adaf_dwconv_same_workspace_bytes(n, size, size, c, k, stride, dt)
    spec = {"out": ((n, o, o, c), dtype), "pool": (n, c)}

    def call(ws, nb, outs, alt):
        return lib.adaf_dwconv_same_bn_act(h, L.ptr(x[alt]), dt, n, size, size, c, k, stride, L.ptr(wk), L.ptr(scale), L.ptr(bias), L.ACT_SWISH,
                                           L.ptr(outs["out"]), L.ptr(outs["pool"]), L.ptr(ws), nb, L.stream_ptr())

    def wrapper():
        out, pool = ops.dwconv_same_bn_act(x[0], wk, scale, bias, k, stride, ops.ACT_SWISH, want_pool=True)
        return {"out": out, "pool": pool}
    contract("dwconv_same", "dwconv_same k%d s%d %d^2 c%d %s" % (k, stride, size, c, dtype), dev, need, call, spec, wrapper, align=(size == 3))


# ------------------------------------------------------------------------------------------------------------------ GRU
def _gru_case(dev, b, t, hid, feat=64, classes=50):
    from tests.test_strided_operands_gpu import _GruCase
    g = _GruCase(dev, batch=b, steps=t, feat=feat, hidden=hid, classes=classes)
    g.x_alt = rnd((b, t, feat), 71, 0.5).to(dev)
    g.dl_alt = rnd((b * t, classes), 78, 0.1).to(dev)
    return g


# The persistent scan borrows its barrier words from the gh region (batch * 3 * hidden words).  adaf_gru_scan_plan needs 17 words per step
# and slice, (T + 1) records: at a pitch of 16 words each where 16 * records fit, packed where only the records fit, else one counter per step:
#   (1, 1), (3, 4): pitch 16;  (33, 8), (65, 4): pitch 16, two slices of the batch with "gru_scan_slices" = 2 (batch > 32), else one;
#   (1, 16): packed (289 records * 16 > 3072 words);  (1, 200): the flat counter (3417 records > 3072 words).
# H = 16 takes the launch-per-step form whatever the mode (the persistent kernel is built for H = 1024).
G_SHAPES = [(1, 1), (1, 16), (3, 4), (33, 8), (65, 4), (1, 200)]


@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("b,t", G_SHAPES)
def test_gru_workspaces_h1024(dev, ops, b, t, mode, slices):
    _gru_contract(dev, ops, b, t, 1024, mode, slices, align=(b, t, mode, slices) == (3, 4, 1, 1))


def test_gru_workspaces_launch_per_step_h16(dev, ops):
    _gru_contract(dev, ops, 2, 2, 16, 1, 1, feat=8, classes=5)


def _gru_contract(dev, ops, b, t, hid, mode, slices, feat=64, classes=50, align=False):
    g = _gru_case(dev, b, t, hid, feat, classes)
    lib, h, p = g.lib, g.h, g.p
    P = L.ptr
    tag = "gru B%d T%d H%d mode%d slices%d " % (b, t, hid, mode, slices)
    ops.set_gru_persistent(mode, dev)
    try:
        with L.option("gru_scan_slices", slices):
            need = lib.adaf_gru_cls_workspace_bytes(b, t, hid)
            assert need == (b * t * 3 * hid + b * 3 * hid + b * t * hid) * 4

            def seq(ws, nb, o, alt):
                return lib.adaf_gru_seq_forward_f32(h, P(g.x_alt if alt else g.x), feat, b, t, feat, hid, P(p["w_ih"]), P(p["w_hh"]), P(p["b_ih"]), P(p["b_hh"]),
                                                    None, P(o["hs"]), P(ws), nb, L.stream_ptr())
            contract("gru", tag + "seq", dev, need, seq, {"hs": (b, t, hid)}, lambda: {"hs": ops.gru_seq_forward(g.x, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])},
                     align=align)

            def cls(ws, nb, o, alt):
                return lib.adaf_gru_cls_forward_f32(h, P(g.x_alt if alt else g.x), feat, b, t, feat, hid, classes, P(p["w_ih"]), P(p["w_hh"]), P(p["b_ih"]),
                                                    P(p["b_hh"]), P(p["fc_w"]), P(p["fc_b"]), P(o["logits"]), P(o["last"]), P(ws), nb, L.stream_ptr())

            def cls_wrapper():
                lg, last = ops.gru_cls_forward(g.x, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"], p["fc_w"], p["fc_b"])
                return {"logits": lg, "last": last}
            contract("gru", tag + "cls", dev, need, cls, {"logits": (b * t, classes), "last": (b, classes)}, cls_wrapper, align=align)

            need_t = lib.adaf_gru_cls_train_workspace_bytes(b, t, hid)
            assert need_t == (b * 3 * hid + b * t * hid) * 4
            mask = [(torch.from_numpy(np.random.Generator(np.random.PCG64(75 + i)).random((b, t, hid), dtype=np.float32)) > 0.5).float().to(dev) * 2.0 for i in (0, 1)]

            def train(ws, nb, o, alt):
                return lib.adaf_gru_cls_train_forward_f32(h, P(g.x_alt if alt else g.x), feat, b, t, feat, hid, classes, P(p["w_ih"]), P(p["w_hh"]), P(p["b_ih"]),
                                                          P(p["b_hh"]), P(p["fc_w"]), P(p["fc_b"]), P(mask[alt]), P(o["gi"]), P(o["hs"]), P(o["logits"]),
                                                          P(o["last"]), P(ws), nb, L.stream_ptr())

            def train_wrapper():
                lg, gi, hs = ops.gru_cls_train_forward(g.x, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"], p["fc_w"], p["fc_b"], mask[0])
                return {"logits": lg, "gi": gi, "hs": hs}
            fw = contract("gru", tag + "train_forward", dev, need_t, train,
                          {"gi": (b * t, 3 * hid), "hs": (b, t, hid), "logits": (b * t, classes), "last": (b, classes)}, train_wrapper, align=align)

            need_b = lib.adaf_gru_cls_backward_workspace_bytes(b, t, hid, classes)
            gi, hs = fw["gi"], fw["hs"]
            # (the "other inputs" run differentiates the same forward with another dlogits and mask: other bytes in every region)

            def backward(ws, nb, o, alt):
                return lib.adaf_gru_cls_backward_f32(h, P(g.x), feat, b, t, feat, hid, classes, P(p["w_ih"]), P(p["w_hh"]), P(p["b_hh"]), P(p["fc_w"]), P(gi), P(hs),
                                                     P(mask[alt]), P(g.dl_alt if alt else g.dlogits), P(o["dx"]), P(o["dw_ih"]), P(o["dw_hh"]), P(o["db_ih"]),
                                                     P(o["db_hh"]), P(o["dw_fc"]), P(o["db_fc"]), P(ws), nb, L.stream_ptr())

            def backward_wrapper():
                names = ("dx", "dw_ih", "dw_hh", "db_ih", "db_hh", "dw_fc", "db_fc")
                return dict(zip(names, ops.gru_cls_backward(g.x, p["w_ih"], p["w_hh"], p["b_hh"], p["fc_w"], gi, hs, mask[0], g.dlogits)))
            h3 = 3 * hid
            contract("gru", tag + "backward", dev, need_b, backward,
                     {"dx": (b, t, feat), "dw_ih": (h3, feat), "dw_hh": (h3, hid), "db_ih": (1, h3), "db_hh": (1, h3), "dw_fc": (classes, hid), "db_fc": (1, classes)},
                     backward_wrapper, align=align)
    finally:
        ops.set_gru_persistent(True, dev)
    assert ops.gru_scan_timeouts(dev) == 0


# ------------------------------------------------------------------------------------------------------------------ smaller entry points
@pytest.mark.parametrize("glob", [False, True])
@pytest.mark.parametrize("b,t,c", [(3, 8, 174), (1, 1, 5)])
def test_fc_meanpool_workspace(dev, ops, b, t, c, glob):
    lib, h = L.load_library(), L.handle(dev)
    f = 64
    feat = [rnd((b * t, f), 980 + i).to(dev) for i in (0, 1)]
    w, bias = rnd((c, f), 982, 0.1).to(dev), rnd((c,), 983, 0.1).to(dev)
    gl = rnd((b, 3, c), 984).to(dev) if glob else None
    need = b * t * c * 4                                                       # include/adafocus.h: "ws holds B*T*C floats"

    def call(ws, nb, o, alt):
        return lib.adaf_fc_meanpool_forward_f32(h, L.ptr(feat[alt]), b, t, f, c, L.ptr(w), L.ptr(bias), L.ptr(gl), 3 if glob else 0, L.ptr(o["out"]), L.ptr(ws), nb,
                                                L.stream_ptr())
    contract("fc_meanpool", "fc_meanpool B%d T%d C%d glob%d" % (b, t, c, glob), dev, need, call, {"out": (b, c)},
             lambda: {"out": ops.fc_meanpool_forward(feat[0], b, w, bias, gl)}, align=(b == 3 and glob))


@pytest.mark.parametrize("t,b,a", [(5, 3, 49), (1, 2, 25)])
def test_ppo_head_loss_workspace(dev, ops, t, b, a):
    lib, h = L.load_library(), L.handle(dev)
    g = np.random.Generator(np.random.PCG64(990))
    head = [rnd((t * b, a + 1), 991 + i).to(dev) for i in (0, 1)]
    actions = torch.from_numpy(g.integers(0, a, (t, b))).to(dev)
    old, ret = rnd((t, b), 993, 0.5).to(dev) - 3.0, rnd((t, b), 994).to(dev)
    need = lib.adaf_ppo_head_workspace_bytes(t, b)
    assert need == 2 * t * b * 4
    spec = {"logprobs": (t, b), "values": (t, b), "entropy": (t, b), "loss": (1, 1), "dhead": (t * b, a + 1)}

    def call(ws, nb, o, alt):
        return lib.adaf_ppo_head_f32(h, L.ptr(head[alt]), 1, t, b, a, L.ptr(actions), L.ptr(old), L.ptr(ret), C.c_float(0.2), None, None, None, L.ptr(o["logprobs"]),
                                     L.ptr(o["values"]), L.ptr(o["entropy"]), L.ptr(o["loss"]), L.ptr(o["dhead"]), L.ptr(ws), nb, L.stream_ptr())

    def wrapper():
        return dict(zip(("logprobs", "values", "entropy", "loss", "dhead"), ops.ppo_loss_head(head[0], actions, old, ret, 0.2)))
    contract("ppo", "ppo_head T%d B%d A%d" % (t, b, a), dev, need, call, spec, wrapper, align=(t == 5))


@pytest.mark.parametrize("split_k", [1, 0])
@pytest.mark.parametrize("pixels,channels", [(7, 128), (1001, 384), (735, 1280)])
def test_ppo_wenc_grad_workspace(dev, ops, pixels, channels, split_k):
    """The split-K slice count follows the device's CU count, the query assumes 256 (never fewer slices than used)."""
    lib, h = L.load_library(), L.handle(dev)
    st = [rnd((pixels, channels), 1000 + i).to(dev) for i in (0, 1)]
    de1, e1 = rnd((pixels, 32), 1002).to(dev), rnd((pixels, 32), 1003).to(dev)
    need = lib.adaf_ppo_wenc_grad_workspace_bytes(pixels, channels, 32)

    def call(ws, nb, o, alt):
        return lib.adaf_ppo_wenc_grad_f32(h, L.ptr(st[alt]), L.ptr(de1), L.ptr(e1), pixels, channels, 32, split_k, L.ptr(o["dw"]), L.ptr(ws), nb, L.stream_ptr())
    contract("ppo", "ppo_wenc_grad %d x %d split_k %d" % (pixels, channels, split_k), dev, need, call, {"dw": (32, channels)},
             lambda: {"dw": ops.ppo_wenc_grad(st[0], de1, e1, bool(split_k))}, align=(pixels == 1001 and split_k == 1))


@pytest.mark.parametrize("t,b", [(5, 3), (1, 1)])
def test_ppo_encoder_backward_workspace(dev, ops, t, b):
    lib, h = L.load_library(), L.handle(dev)
    hw, cin, cmid, hid = 49, 1280, 32, 1024
    states = [rnd((t * b, 7, 7, cin), 1010 + i).to(dev) for i in (0, 1)]
    e1 = rnd((t * b, hw * cmid), 1012).to(dev).clamp(min=0)
    e_bt, dx = rnd((b, t, hid), 1013).to(dev).clamp(min=0), rnd((b, t, hid), 1014, 0.1).to(dev)
    w_lin = rnd((hid, hw * cmid), 1015, 0.02).to(dev)
    need = lib.adaf_ppo_encoder_backward_workspace_bytes(t, b, hw, cin, cmid, hid)
    spec = {"dw_enc": (cmid, cin), "dw_lin": (hid, cmid * hw), "db_lin": (1, hid)}

    def call(ws, nb, o, alt):
        return lib.adaf_ppo_encoder_backward_f32(h, L.ptr(states[alt]), L.ptr(e1), L.ptr(e_bt), L.ptr(dx), t, b, hw, cin, cmid, hid, L.ptr(w_lin), L.ptr(o["dw_enc"]),
                                                 L.ptr(o["dw_lin"]), L.ptr(o["db_lin"]), L.ptr(ws), nb, L.stream_ptr())

    def wrapper():
        return dict(zip(("dw_enc", "dw_lin", "db_lin"), ops.ppo_encoder_backward(states[0], e1, e_bt, dx, t, b, w_lin)))
    contract("ppo", "ppo_encoder_backward T%d B%d" % (t, b), dev, need, call, spec, wrapper, align=(t == 5))


def _stem_params(dev):
    w = rnd((64, 3, 7, 7), 1030, 147 ** -0.5).to(dev)
    return w, (rnd((64,), 1031, 0.2) + 1.0).to(dev), rnd((64,), 1032, 0.1).to(dev)


@pytest.mark.parametrize("form,p,half", [("tile4", 50, False), ("tile6", 37, True), ("strip", 64, False), ("strip", 96, True), ("unfused", 33, False),
                                         ("unfused", 33, True), ("auto", 96, False), ("auto", 100, True)])
def test_stem_pool_workspace(dev, ops, form, p, half):
    """adaf_stem7x7_pool, every form: the workspace is adaf_stem7x7_bn_relu_f32's packed filter bank (no size query of its own)."""
    lib, h = L.load_library(), L.handle(dev)
    n = 3
    x = [_x4(n, p, 1033 + i, dev) for i in (0, 1)]
    w, scale, bias = _stem_params(dev)
    oh = (p - 1) // 2 + 1
    ph = (oh - 1) // 2 + 1
    need = lib.adaf_stem7x7_workspace_bytes()
    assert need == 2 * 74 * 64 * 4
    conv_map = torch.empty((n, oh, oh, 64), device=dev)
    dtype = torch.float16 if half else torch.float32

    def call(ws, nb, o, alt):
        return lib.adaf_stem7x7_pool(h, L.ptr(x[alt]), n, p, L.ptr(w), L.ptr(scale), L.ptr(bias), ops.STEM_FORMS[form], L.DTYPE_F16 if half else L.DTYPE_F32,
                                     L.ptr(o["out"]), L.ptr(conv_map), None, L.ptr(ws), nb, L.stream_ptr())
    contract("stem", "stem7x7_pool %s P%d %s" % (form, p, dtype), dev, need, call, {"out": ((n, ph, ph, 64), dtype)},
             lambda: {"out": ops.stem7x7_pool(x[0], w, scale, bias, form=form, half=half)}, align=(form == "strip" and not half))


@pytest.mark.parametrize("layout,half", [("nchw", False), ("nhwc4", True)])
def test_stem_pool_frames_workspace(dev, ops, layout, half):
    lib, h = L.load_library(), L.handle(dev)
    nf, hw, p, fpa, k = 4, 80, 64, 2, 2
    fr = [rnd((nf, 3, hw, hw), 1040 + i).to(dev) for i in (0, 1)]
    if layout == "nhwc4":
        from adafocus_amd.utils import nchw_to_nhwc4
        fr = [nchw_to_nhwc4(f).contiguous() for f in fr]
    act = torch.from_numpy(np.random.Generator(np.random.PCG64(1042)).random((k * nf // fpa, 2), dtype=np.float32)).to(dev)
    w, scale, bias = _stem_params(dev)
    need = lib.adaf_stem7x7_workspace_bytes()
    code = L.LAYOUT_NHWC4 if layout == "nhwc4" else L.LAYOUT_NCHW
    dtype = torch.float16 if half else torch.float32

    def call(ws, nb, o, alt):
        return lib.adaf_stem7x7_pool_frames(h, L.ptr(fr[alt]), code, nf, hw, hw, L.ptr(act), act.shape[0], fpa, p, L.ptr(w), L.ptr(scale), L.ptr(bias),
                                            L.DTYPE_F16 if half else L.DTYPE_F32, L.ptr(o["out"]), L.ptr(ws), nb, L.stream_ptr())
    contract("stem", "stem7x7_pool_frames %s %s" % (layout, dtype), dev, need, call, {"out": ((k * nf, p // 4, p // 4, 64), dtype)},
             lambda: {"out": ops.stem7x7_pool_frames(fr[0], act, p, w, scale, bias, frames_per_action=fpa, half=half)}, align=not half)


def test_stem_conv_workspace(dev, ops):
    """adaf_stem7x7_bn_relu_f32, the training walk's stem: the same workspace."""
    lib, h = L.load_library(), L.handle(dev)
    n, p = 3, 33
    x = [_x4(n, p, 1050 + i, dev) for i in (0, 1)]
    w, scale, bias = _stem_params(dev)
    need = lib.adaf_stem7x7_workspace_bytes()

    def call(ws, nb, o, alt):
        return lib.adaf_stem7x7_bn_relu_f32(h, L.ptr(x[alt]), n, p, L.ptr(w), L.ptr(scale), L.ptr(bias), L.ptr(o["out"]), L.ptr(ws), nb, L.stream_ptr())
    contract("stem", "stem7x7_bn_relu P%d" % p, dev, need, call, {"out": (n, 17, 17, 64)}, lambda: {"out": ops.stem7x7_bn_relu(x[0], w, scale, bias)}, align=True)


# ------------------------------------------------------------------------------------------------------------------ non-positive extents
def test_queries_return_zero_for_non_positive_extents_and_the_calls_are_refused(dev, ops):
    lib, h = L.load_library(), L.handle(dev)
    trunk = _trunk(dev, "f32")._sync()
    eng = _glancer(dev)._engine.sync()
    ef = _effnet(dev, "efficientnet-b0", "f32", "native").engine()
    for n, size in ((0, 64), (-1, 64), (2, 0), (2, -32)):
        assert lib.adaf_resnet50_workspace_bytes(trunk._net, n, size) == 0
        assert lib.adaf_mobilenetv2_workspace_bytes(eng._net, n, size, 0) == 0
        assert lib.adaf_effnet_workspace_bytes(ef._net, n, size, 0) == 0
    assert lib.adaf_effnet_workspace_bytes(ef._net, 2, 31, 0) == 0                # below the smallest input the network takes
    for args in ((0, 9, 9, 8, 3, 1), (-2, 9, 9, 8, 3, 1), (2, 0, 9, 8, 3, 1), (2, 9, -1, 8, 3, 1), (2, 9, 9, 0, 3, 1), (2, 9, 9, 8, 3, 0)):
        assert lib.adaf_dwconv_same_workspace_bytes(*args, L.DTYPE_F32) == 0, args
    # ... and the calls with such extents are refused before anything is launched (a 1 MiB-guarded workspace and canary outputs)
    buf, ws = S.guarded_workspace(4096, dev)
    outs = _outs({"a": (4, 2048), "b": (4, 1280), "m": (4, 1, 1, 1280)}, dev)
    a, b, m = outs["a"][1], outs["b"][1], outs["m"][1]
    x = _x4(2, 64, 1020, dev)
    for n, size in ((0, 64), (-1, 64), (2, 0)):
        assert lib.adaf_resnet50_forward(trunk._net, L.ptr(x), n, size, 0, 8, L.ptr(a), 2048, L.ptr(ws), 4096, L.stream_ptr()) == E_BADARG
        assert lib.adaf_mobilenetv2_forward(eng._net, L.ptr(x), n, size, 0, 8, L.ptr(m), L.ptr(b), 1280, L.ptr(ws), 4096, L.stream_ptr()) == E_BADARG
        assert lib.adaf_effnet_forward(ef._net, L.ptr(x), n, size, 0, -1, None, None, L.ptr(b), 1280, L.ptr(ws), 4096, L.stream_ptr()) == E_BADARG
    one = torch.ones(64, device=dev)
    for n, hh in ((0, 4), (-1, 4), (2, 0)):
        assert lib.adaf_dwconv_same_bn_act(h, L.ptr(x), L.DTYPE_F32, n, hh, 4, 8, 3, 1, L.ptr(one), L.ptr(one), L.ptr(one), 0, L.ptr(a), L.ptr(b), L.ptr(ws), 4096,
                                           L.stream_ptr()) == E_BADARG
    for bt in ((-1, 2), (2, 0), (2, -3)):
        assert lib.adaf_fc_meanpool_forward_f32(h, L.ptr(x), bt[0], bt[1], 64, 5, L.ptr(one), L.ptr(one), None, 0, L.ptr(a), L.ptr(ws), 4096, L.stream_ptr()) == E_BADARG
    torch.cuda.synchronize()
    _untouched("non-positive extents", buf, outs)
