#!/usr/bin/env python3
"""Bit-level fingerprint of the conv engine's launch decisions (csrc/conv_gemm.hip: kTileTable, plan_conv, launch_row).  For every case one
JSON line with the sha256 of the output bytes, or the error code and message of a refused case -- no times, so two builds of the library that
take the same decisions and compute the same bits print the same lines.  Inputs and weights are seeded; only the public surface is used (the
C ABI through tools/guard_bands.conv_call, hip_ops, resnet), so the same file runs against another build through ADAF_LIB.  A library that
has the debug hook adaf_conv_plan_debug also prints, per direct conv case, a {"plan": ...} line with the plan and the kernel it names.

Cases: every tile id (and 0, and the ids the entry point refuses) on a dense 1x1, a 3x3 on 6x6 maps of 160 images, a 1x1 with K % 32 != 0 and
a 3x3 the DMA kernel cannot take; 1x1 / strided 1x1 / 3x3 / 7x7 on 3x3 ... 48x48 maps with and without identity; cin not a multiple of 4
(refused); cout 16 / 24 / 32 / 96 / 160 with many and few rows; row-strided operands; the temporal shift at shift_div 2 / 4 / 8 / 16, T = 8 /
12, option tsm_lean 0 / 1; image counts on both sides of the tile's rows for the position-major gate and set_conv_pos_major off; the fp16
entry point with every dtype combination; the ResNet-50 trunk under the options conv_pool / split_lean / tsm_lean 0 and 1.

Usage: python tools/conv_launch_digest.py > digest.jsonl                      (compare the lines without "plan" of two builds with cmp)
       python tools/conv_launch_digest.py --check-trace digest.jsonl kernel_trace.csv     (rocprofv3 --kernel-trace of the run above: every
                                                     case's traced kernel is the one its plan names; prints the conv launch list)"""
import csv
import ctypes as C
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLAN_FIELDS = ("tile", "bm", "bn", "wgm", "wgn", "family", "fallback", "pipe", "split", "presplit", "dt", "dense", "gather", "special", "lean",
               "pos_major", "pool", "tiles_n", "nblocks", "pm_images", "pm_groups", "vec_epi", "K", "cin", "ldx", "fold")
FAMILIES = ("reg", "dma_top", "dma_mid", "bar23", "split6", "split9", "presplit", "f16", "lat")
F_IN16, F_OUT16, F_RES16, F_PRESPLIT, F_VEC_EPI, F_BESIDE = 1, 2, 4, 8, 64, 128
ENGINE_IDS = [0, 1, 2, 3, 4, 5, 21, 22, 23, 24, 25, 26, 31, 32, 33, 34, 38, 39, 40, 41, 42, 43, 44, 45, 46, 51, 52, 53, 54,
              61, 62, 63, 64, 65, 66, 67, 71, 72, 73, 74, 81, 82, 83, 84, 88, 95]
F16_IDS = [0, 81, 82, 83, 84, 88]


def plan_flags(in16=False, out16=False, res16=False, presplit=False, pm_allow=1, vec_epi=True, pool_hw=0, beside=False):
    return (F_IN16 * in16 | F_OUT16 * out16 | F_RES16 * res16 | F_PRESPLIT * presplit | (pm_allow & 3) << 4 | F_VEC_EPI * vec_epi |
            F_BESIDE * beside | pool_hw << 8)


def conv_plan(lib, params, flags, cus):
    """The plan adaf_conv_plan_debug gives as a dict, or {"refused": code}; None when the library has no such hook."""
    try:
        fn = lib.adaf_conv_plan_debug
    except AttributeError:
        return None
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    out = (C.c_int * len(PLAN_FIELDS))()
    rc = fn(C.byref(params), flags, cus, out, len(PLAN_FIELDS))
    return dict(zip(PLAN_FIELDS, out)) if rc == 0 else {"refused": rc}


def kernel_of(plan):
    """The kernel instantiation a plan names, spelled as the demangler spells it."""
    if plan is None or "refused" in plan or plan["tile"] < 0:
        return None
    b = lambda v: "true" if v else "false"      # noqa: E731
    shape = "%d, %d, %d, %d" % (plan["bm"], plan["bn"], plan["wgm"], plan["wgn"])
    fam = FAMILIES[plan["family"]]
    if fam == "lat":
        return "conv_lat_kernel<%d>" % (128 if plan["cin"] % 128 == 0 else 64)
    if fam == "reg":
        return "conv_gemm_kernel<%s, 32, %s, 0, %d>" % (shape, b(plan["dense"]), plan["dt"])
    return "conv_gemm_glds_kernel<%s, %s, %d, %s, %d, %s, %d, %s, %s, %s>" % (
        shape, b(plan["dense"]), plan["pipe"], b(plan["special"]), plan["split"], b(plan["presplit"]), plan["dt"], b(plan["pos_major"]),
        b(plan["lean"]), b(plan["pool"]))


def direct_cases():
    """(name, settings) of the single-launch cases, in run order."""
    out = []

    def add(name, **kw):
        out.append((name, kw))
    shapes = dict(dense=dict(n=2, hw=12, cin=64, cout=96), k3pm=dict(n=160, hw=6, cin=64, cout=64, k=3, pad=1),
                  k20=dict(n=2, hw=12, cin=20, cout=24), k3reg=dict(n=2, hw=9, cin=12, cout=40, k=3, pad=1))
    for sname, s in shapes.items():
        for t in ENGINE_IDS:
            add("ids/%s/t%d" % (sname, t), tile=t, **s)
    for hw in (3, 6, 12, 24, 48):
        n = max(2, 2304 // (hw * hw))
        for res in (False, True):
            add("grid/1x1/hw%d/res%d" % (hw, res), n=n, hw=hw, cin=128, cout=64, res=res)
            add("grid/1x1s2/hw%d/res%d" % (hw, res), n=n, hw=hw, cin=64, cout=128, stride=2, res=res)
            add("grid/3x3/hw%d/res%d" % (hw, res), n=n, hw=hw, cin=32, cout=64, k=3, pad=1, res=res)
            add("grid/3x3s2/hw%d/res%d" % (hw, res), n=n, hw=hw, cin=32, cout=64, k=3, pad=1, stride=2, res=res)
            add("grid/7x7/hw%d/res%d" % (hw, res), n=n, hw=hw, cin=4, cout=64, k=7, pad=3, stride=2, res=res)
    add("grid/1x1s2/big", n=256, hw=12, cin=256, cout=512, stride=2)          # a downsample branch that fills 128 x 128 tiles
    add("grid/1x1s2/big/t65", n=256, hw=12, cin=256, cout=512, stride=2, tile=65)
    for cin in (6, 36, 100, 132):     # 6: refused (cin % 4); the others K % 32 != 0
        add("k/cin%d" % cin, n=4, hw=8, cin=cin, cout=64)
        add("k/cin%d/3x3" % cin, n=4, hw=8, cin=cin, cout=64, k=3, pad=1)
    for cout in (16, 24, 32, 96, 160):
        add("narrow/cout%d/many" % cout, n=8, hw=64, cin=32, cout=cout)             # 32768 rows: 256 row tiles of 128
        add("narrow/cout%d/few" % cout, n=2, hw=7, cin=32, cout=cout)
        add("narrow/cout%d/longk" % cout, n=512, hw=7, cin=960, cout=cout)          # 25088 rows, K = 960: the 256 x 32 tile's rule
    for t in (0, 1, 33, 41):
        add("strided/1x1/t%d" % t, n=4, hw=6, cin=64, cout=64, res=True, tile=t, ld=(72, 68, 76))
        add("strided/3x3/t%d" % t, n=130, hw=3, cin=32, cout=64, k=3, pad=1, res=True, tile=t, ld=(40, 68, 64))
    for T in (8, 12):
        for div in (2, 4, 8, 16):
            for cin in (64, 256):
                for lean in (1, 0):
                    for t in (0, 33, 41):
                        if lean == 0 and t != 0:
                            continue
                        add("tsm/T%d/div%d/cin%d/lean%d/t%d" % (T, div, cin, lean, t), n=2 * T, hw=4, cin=cin, cout=128, tsm=(T, div), tile=t,
                            opts={"tsm_lean": lean})
    for t, bm in ((31, 128), (33, 64), (39, 256)):
        for n in (bm - 1, bm, bm + 1):
            add("pm/t%d/n%d" % (t, n), n=n, hw=3, cin=32, cout=64, k=3, pad=1, tile=t)
    add("pm/off/t31", n=130, hw=3, cin=32, cout=64, k=3, pad=1, tile=31, pos_major=0)
    add("pm/off/auto", n=160, hw=6, cin=64, cout=64, k=3, pad=1, pos_major=0)
    add("pm/fill/hw12", n=130, hw=12, cin=32, cout=64, k=3, pad=1, tile=31)     # 0.84 of the taps inside: position-major
    add("pm/fill/hw48", n=130, hw=48, cin=32, cout=64, k=3, pad=1, tile=31)     # 0.96 and more inside: row-major
    for xd, od in (("f16", "f16"), ("f16", "f32"), ("f32", "f16"), ("f32", "f32")):     # (f32, f32: refused by the fp16 entry point)
        for res in (False, True):
            for t in F16_IDS:
                add("f16/%s_%s/res%d/1x1/t%d" % (xd, od, res, t), f16=(xd, od), n=4, hw=6, cin=64, cout=96, res=res, tile=t)
            add("f16/%s_%s/res%d/3x3" % (xd, od, res), f16=(xd, od), n=4, hw=6, cin=64, cout=64, k=3, pad=1, res=res)
            add("f16/%s_%s/res%d/k40" % (xd, od, res), f16=(xd, od), n=4, hw=6, cin=40, cout=64, res=res)
            add("f16/%s_%s/res%d/narrow" % (xd, od, res), f16=(xd, od), n=8, hw=64, cin=32, cout=24, res=res)
    for div in (2, 4, 8, 16):
        add("f16/tsm/div%d" % div, f16=("f16", "f16"), n=16, hw=4, cin=64, cout=128, tsm=(8, div))
    add("f16/ids/t31", f16=("f16", "f16"), n=4, hw=6, cin=64, cout=96, tile=31)         # refused: not an fp16 id
    return out


def run_direct(name, cfg, idx, lib, L, torch, conv_call, hip_ops):
    dev = torch.device("cuda:0")
    n, hw, cin, cout = cfg["n"], cfg["hw"], cfg["cin"], cfg["cout"]
    k, stride, pad, tile = cfg.get("k", 1), cfg.get("stride", 1), cfg.get("pad", 0), cfg.get("tile", 0)
    T, div = cfg.get("tsm", (0, 8))
    xd, od = cfg.get("f16", ("f32", "f32"))
    dt = {"f16": torch.float16, "f32": torch.float32}
    ohw = (hw + 2 * pad - k) // stride + 1
    ldx, ldo, ldr = cfg.get("ld", (cin, cout, cout))
    g = torch.Generator().manual_seed(1000 + idx)
    rnd = lambda *s: torch.randn(*s, generator=g)       # noqa: E731

    def strided(dense, ld, dtype):      # the payload as a row-strided view of a wider zero tensor
        full = torch.zeros(dense.shape[:-1] + (ld,), dtype=dtype, device=dev)
        full[..., :dense.shape[-1]] = dense.to(dev).to(dtype)
        return full[..., :dense.shape[-1]]
    x = strided(rnd(n, hw, hw, cin), ldx, dt[xd])
    w = (rnd(cout, k, k, cin) / (k * k * cin) ** 0.5).to(dev).to(dt[xd]).contiguous()
    scale, bias = (1 + 0.1 * rnd(cout)).to(dev), (0.1 * rnd(cout)).to(dev)
    res = strided(rnd(n, ohw, ohw, cout), ldr, torch.float16 if "f16" in cfg else torch.float32) if cfg.get("res") else None
    out = strided(torch.zeros(n, ohw, ohw, cout), ldo, dt[od])
    rec = dict(case=name)
    h = L.handle(dev)
    pm = cfg.get("pos_major", 1)
    hip_ops.set_conv_pos_major(pm, dev)
    olds = {key: L.set_option(key, v) for key, v in cfg.get("opts", {}).items()}
    try:
        params = L.ConvParams(n=n, h=hw, w=hw, cin=cin, cout=cout, kh=k, kw=k, stride=stride, pad=pad, act=L.ACT_RELU, tsm_segments=T, tsm_div=div,
                              ldx=ldx, ldo=ldo, ldr=ldr if res is not None else 0, tile=tile)
        vec = cout % 4 == 0 and ldo % 4 == 0 and (res is None or ldr % 4 == 0)
        plan = conv_plan(lib, params, plan_flags(xd == "f16", od == "f16", res is not None and "f16" in cfg, pm_allow=pm, vec_epi=vec),
                         lib.adaf_device_cus(h))
        try:
            conv_call("f16" if "f16" in cfg else "engine", x, w, scale, bias, res, out, stride=stride, pad=pad, act=L.ACT_RELU, tsm_segments=T,
                      tsm_div=div, tile=tile)
            torch.cuda.synchronize()
            rec["sha"] = hashlib.sha256(out.contiguous().cpu().numpy().tobytes()).hexdigest()
        except L.AdafError as e:
            rec["error"] = str(e)
    finally:
        for key, v in olds.items():
            L.set_option(key, v)
        hip_ops.set_conv_pos_major(1, dev)
    print(json.dumps(rec, sort_keys=True), flush=True)
    if plan is not None:
        print(json.dumps(dict(case=name, plan=plan, kernel=kernel_of(plan)), sort_keys=True), flush=True)


def run_trunk(L, torch):
    """The ResNet-50 trunk (pooled last conv3, pre-split split tiles, shifted conv1s) with each of the three options at 1 and 0."""
    from adafocus_amd import resnet, synth
    from adafocus_amd.utils import nchw_to_nhwc4
    dev = torch.device("cuda:0")
    net = resnet.resnet50()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, 1007).items()}, strict=True)
    net = net.eval().to(dev)
    x = nchw_to_nhwc4(torch.from_numpy(synth.synth_frames(128, 1, 96, seed=196)).to(dev))
    for math in ("f32", "split_bf16", "f16"):
        net.set_math(math)
        trunk = net._sync()
        for T in (0, 8):
            for key in ("conv_pool", "split_lean", "tsm_lean"):
                for v in (1, 0):
                    rec = dict(case="trunk/%s/T%d/%s%d" % (math, T, key, v))
                    with L.option(key, v):
                        try:
                            feat = trunk.forward(x, T, 8)
                            torch.cuda.synchronize()
                            rec["sha"] = hashlib.sha256(feat.contiguous().cpu().numpy().tobytes()).hexdigest()
                            rec["launches"] = [(r["flops"], r["bytes"], r["tile"]) for r in trunk.profile(x, T, 8)]
                        except L.AdafError as e:
                            rec["error"] = str(e)
                    print(json.dumps(rec, sort_keys=True), flush=True)


def short_name(kernel_name):
    return re.sub(r"\(.*", "", kernel_name.replace("(anonymous namespace)::", "")).replace("void ", "")


def check_trace(digest_path, trace_path):
    """The conv launches of a kernel trace, in order; the first ones belong to the direct cases that were not refused: compared with the
    kernel each plan names.  Prints one line per conv launch (name, grid, workgroup, LDS) and the verdict; exit status 1 on a mismatch.
    Plans and launches are paired BY POSITION: the i-th conv launch belongs to the i-th direct case that ran.  That holds only while every
    direct case launches exactly one conv kernel; a case that launched none or two would shift every later comparison (and show as a
    run of mismatches from that case on)."""
    recs = [json.loads(ln) for ln in open(digest_path) if ln.startswith("{")]
    ran = [r["case"] for r in recs if "sha" in r and not r["case"].startswith("trunk/")]
    named = {r["case"]: r["kernel"] for r in recs if "plan" in r}
    rows = sorted(csv.DictReader(open(trace_path)), key=lambda r: int(r["Start_Timestamp"]))
    convs = [r for r in rows if re.match(r"conv_(gemm|lat|fused_tail)", short_name(r["Kernel_Name"]))]
    bad = []
    for i, r in enumerate(convs):
        nm = short_name(r["Kernel_Name"])
        print("%s grid %s wg %s lds %s" % (nm, r["Grid_Size_X"], r["Workgroup_Size_X"], r["LDS_Block_Size"]))
        if i < len(ran) and named and named.get(ran[i]) != nm:
            bad.append((ran[i], named.get(ran[i]), nm))
    if len(convs) < len(ran):
        bad.append(("trace has %d conv launches, the digest %d direct cases that ran" % (len(convs), len(ran)), None, None))
    print("# %d conv launches, %d direct cases checked against their plans, %d mismatches" % (len(convs), len(ran) if named else 0, len(bad)))
    for b in bad:
        print("# MISMATCH case %s: plan %s, trace %s" % b)
    return 1 if bad else 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--check-trace":
        return check_trace(sys.argv[2], sys.argv[3])
    import torch
    from adafocus_amd import _lib as L, hip_ops
    from tools.guard_bands import conv_call
    lib = L.load_library()
    with torch.no_grad():
        for idx, (name, cfg) in enumerate(direct_cases()):
            run_direct(name, cfg, idx, lib, L, torch, conv_call, hip_ops)
        run_trunk(L, torch)
    return 0


if __name__ == "__main__":
    sys.exit(main())
