#!/usr/bin/env python3
"""Tile picks of the ResNet-50 trunk measured under the benchmark's own concurrency (profiles/tile_regime_ab.md): bench.py's default step --
64 clips x 16 frames, 96^2 patches, hot_path round-robined over 3 streams -- with one class of conv launches at a time moved to another
tile of its family through set_tiles.  All variants run in one process, interleaved, `--rounds` rounds of `--steps` steps each; every fp32
tile gives the same bits, so only the time differs.  Prints a markdown table (median / min / max ms per step per variant, and the spread of
the baseline against itself) and one JSON line per round.

`base` is the planner's own pick: a forward issued while another trunk forward of the handle is in flight on another stream is priced for launches that run
beside others, any other forward (--streams 1, a stream capture) as before.  A variant may fix the regime (option conv_tile_regime:
`before` = 0, the earlier picks everywhere; `always` = 2, the busy pricing everywhere).  --mode pipelined times GFV.offline_forward_pipelined
from uint8 clips (the loop of evaluate.validate: front and back stream), --mode graph a replayed GFV.capture_hot_path(exclusive=True) graph
of the same step, captured once per variant, and --shape N,P,T runs the trunk alone on N patches of P^2 with temporal shift T (the other configurations: 512 x 96^2, 1024 x 128^2,
512 x 128^2 shifted, 768 x 144^2 shifted) instead of the benchmark's step.

Usage: python tools/tile_regime_ab.py [--rounds 6] [--steps 30] [--streams 3] [--variants base,l3c1_32,...] [--shape 512,128,8]
                                      [--mode bench|pipelined|graph]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLANES = ((64, 3), (128, 4), (256, 6), (512, 3))


def conv_index():
    """launch index -> name, in adaf_resnet50's order: stem, then per block conv1, conv2, conv3, (downsample)."""
    names = ["stem"]
    for s, (_, nb) in enumerate(PLANES):
        for b in range(nb):
            names += ["L%d.%d.%s" % (s + 1, b, c) for c in (("c1", "c2", "c3", "ds") if b == 0 else ("c1", "c2", "c3"))]
    return names


NAMES = conv_index()


def tiles_for(rules):
    """rules: {predicate name: tile}; a launch takes the tile of the first class it is in, 0 (the planner's pick) otherwise."""
    classes = {
        "l3c1": lambda n: n.startswith("L3.") and n.endswith(".c1") and not n.startswith("L3.0"),
        "l4c1": lambda n: n.startswith("L4.") and n.endswith(".c1") and not n.startswith("L4.0"),
        "l3c2": lambda n: n.startswith("L3.") and n.endswith(".c2"),
        "l4c2": lambda n: n.startswith("L4.") and n.endswith(".c2"),
        "l3c3": lambda n: n.startswith("L3.") and n.endswith(".c3"),
        # (the last conv3 keeps the planner's pick: an override would take the pooled epilogue away from it)
        "l4c3": lambda n: n.startswith("L4.") and n.endswith(".c3") and n != "L4.2.c3",
        "l4ds": lambda n: n == "L4.0.ds",
        "l40c1": lambda n: n == "L4.0.c1",
        "l2c2": lambda n: n.startswith("L2.") and n.endswith(".c2"),
        "l2c13": lambda n: n.startswith("L2.") and (n.endswith(".c1") or n.endswith(".c3")) and n != "L2.0.c1",
    }
    out = []
    for n in NAMES:
        t = 0
        for cls, tile in rules.items():
            if cls != "regime" and classes[cls](n):
                t = tile
                break
        out.append(t)
    return out


VARIANTS = {
    "base": {},
    "base2": {},                     # the baseline a second time: its distance to `base` is the noise of this table
    "l3c1_32": {"l3c1": 32}, "l3c1_34": {"l3c1": 34}, "l3c1_31": {"l3c1": 31},
    "l4c1_32": {"l4c1": 32}, "l4c1_34": {"l4c1": 34}, "l4c1_31": {"l4c1": 31},
    "l3c2_32": {"l3c2": 32}, "l3c2_34": {"l3c2": 34}, "l3c2_31": {"l3c2": 31},
    "l4c2_32": {"l4c2": 32}, "l4c2_34": {"l4c2": 34}, "l4c2_31": {"l4c2": 31},
    "l4c3_31": {"l4c3": 31}, "l4c3_34": {"l4c3": 34}, "l4c3_33": {"l4c3": 33},
    "l4ds_31": {"l4ds": 31}, "l4ds_34": {"l4ds": 34},
    "l3c3_31": {"l3c3": 31}, "l3c3_34": {"l3c3": 34},
    "l2c2_31": {"l2c2": 31}, "l2c13_31": {"l2c13": 31},
    "all_32": {"l3c1": 32, "l4c1": 32, "l3c2": 32, "l4c2": 32},
    "all_31": {"l3c1": 31, "l4c1": 31, "l3c2": 31, "l4c2": 31},
    "l3_31_l4_32": {"l3c1": 31, "l3c2": 31, "l4c1": 32, "l4c2": 32},
    "l3_31_l4_34": {"l3c1": 31, "l3c2": 31, "l4c1": 34, "l4c2": 34},
    "all_33": {"l3c1": 33, "l4c1": 33, "l3c2": 33, "l4c2": 33},
    "before": {"regime": 0}, "before2": {"regime": 0}, "always": {"regime": 2},
    # one class moved on top of the earlier picks
    "b_l3c1_32": {"regime": 0, "l3c1": 32}, "b_l3c1_31": {"regime": 0, "l3c1": 31}, "b_l3c1_34": {"regime": 0, "l3c1": 34},
    "b_l3c2_32": {"regime": 0, "l3c2": 32}, "b_l3c2_31": {"regime": 0, "l3c2": 31}, "b_l3c2_34": {"regime": 0, "l3c2": 34},
    "b_l4c1_32": {"regime": 0, "l4c1": 32}, "b_l4c1_34": {"regime": 0, "l4c1": 34}, "b_l4c2_32": {"regime": 0, "l4c2": 32},
    "b_l4c2_34": {"regime": 0, "l4c2": 34},
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--variants", type=str, default="")
    ap.add_argument("--shape", type=str, default="", help="N,P,T: the trunk alone on N patches of P^2, temporal shift T (0 = none)")
    ap.add_argument("--mode", choices=["bench", "pipelined", "graph"], default="bench")
    a = ap.parse_args()
    import numpy as np
    import torch
    from adafocus_amd import _lib, synth
    from adafocus_amd.gfv_net import GFV
    from bench_extras import act_args, synth_model_state

    dev = torch.device("cuda:0")
    b, t, p = 64, 16, 96
    model = GFV(act_args(t, p, b)).eval()
    model.load_state_dict(synth_model_state(model, 1007), strict=True)
    model = model.to(dev)
    frames = torch.from_numpy(synth.synth_frames(b, t, 224, seed=100)).to(dev).view(b * t, 3, 224, 224)
    _, act_np = synth.synth_actions(b * t, 7, seed=2)
    actions = torch.from_numpy(act_np).to(dev)
    gvec = torch.from_numpy(np.random.Generator(np.random.PCG64(300)).standard_normal((b, t, 1280), dtype=np.float32)).to(dev)
    trunk = model.focuser.net._sync()
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(a.streams, 1))]
    if a.shape:
        sn, sp, st = (int(v) for v in a.shape.split(","))
        x = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).standard_normal((sn, sp, sp, 4), dtype=np.float32)).to(dev)
        x[..., 3] = 0

    def step():
        if a.shape:
            return None, trunk.forward(x, st, 8)
        return model.hot_path(frames, gvec, actions, b, t)

    graphs = {}
    if a.mode == "pipelined":
        u8 = torch.randint(0, 256, (b, 224, 224, t * 3), device=dev, dtype=torch.uint8)
        u8s = [u8, u8.clone(), u8.clone()]

    def run_mode(n, v):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            if a.mode == "pipelined":
                for i in range(n):
                    out = model.offline_forward_pipelined(u8s[i % 3], t)
                model.pipeline_flush()
            else:
                for i in range(n):
                    out = graphs[v].replay()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, (out[0], out[1].clone())

    def run(n, v=None):
        if a.mode != "bench":
            return run_mode(n, v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = None
        for i in range(n):
            with torch.no_grad(), torch.cuda.stream(streams[i % len(streams)]):
                out = step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, out

    def select(v):
        _lib.set_option("conv_tile_regime", VARIANTS[v].get("regime", 1))
        trunk.set_tiles(tiles_for(VARIANTS[v]))

    names = [v for v in (a.variants.split(",") if a.variants else VARIANTS)]
    ref = None
    ms = {v: [] for v in names}
    for v in names:      # warm every variant (workspaces, code objects) and check the bits once
        select(v)
        if a.mode == "graph":      # captured under the variant's regime; replayed alone
            graphs[v] = model.capture_hot_path(b, t, exclusive=True)
            graphs[v].frames.copy_(frames)
            graphs[v].gvec.copy_(gvec)
            graphs[v].actions.copy_(actions)
        _, out = run(6, v)
        last = out[1].clone()
        ref = last if ref is None else ref
        assert torch.equal(last, ref), "variant %s changed the logits" % v
    for r in range(a.rounds):
        order = names if r % 2 == 0 else names[::-1]
        for v in order:
            select(v)
            run(3, v)
            ms[v].append(run(a.steps, v)[0])
        print(json.dumps({"round": r, **{v: round(ms[v][-1], 4) for v in names}}), flush=True)
    base = statistics.median(ms[names[0]])
    print("\n| variant | overrides | median ms/step | min | max | median vs %s |" % names[0])
    print("|---|---|---|---|---|---|")
    for v in names:
        m = statistics.median(ms[v])
        print("| %s | %s | %.4f | %.4f | %.4f | %+.2f %% |" % (v, ", ".join("%s->%d" % kv for kv in VARIANTS[v].items()) or "-", m, min(ms[v]),
                                                                 max(ms[v]), 100.0 * (m - base) / base))


if __name__ == "__main__":
    main()
