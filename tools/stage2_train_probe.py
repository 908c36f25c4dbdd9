#!/usr/bin/env python3
"""Stage-2 step on one MI355X at B = 64, T = 16, P = 96, A = 49 (C = 1280, 7 x 7 map, H = 1024): one JSON line with ms per call of
  rollout_ms            glance + T x one_step_act(training=True) + rewards (no update)
  returns_ms            the discounted, normalised returns kernel
  evaluate_fwd_ms       the policy's training forward over the stored roll-out (encoder, GRU scan, stacked heads; activations kept)
  loss_head_ms          the PPO loss head (forward and backward in one pass)
  gru_heads_bwd_ms      backward of the GRU + stacked heads (adaf_gru_cls_backward_f32 with dx)
  encoder_bwd_ms        backward of the state encoder, including the split-K weight gradient of the 1x1 conv
  wenc_splitk_call_ms   that gradient on its own PER CALL of hip_ops.ppo_wenc_grad: HIP events around --splitk-calls calls that rotate over
                        two state buffers (no call reads what the previous one left in a cache).  It includes the host's enqueue work, so
                        it is an UPPER BOUND of the kernel time
  wenc_splitk_kernel_us with --trace DIR: the kernel's own time (median over its launches in a rocprofv3 --kernel-trace of a
                        `--splitk-only` run, same rotation), the reduce kernel's, and the rate of the 257 MB of states (and of all bytes the
                        two kernels move) as a fraction of 6.3 TB/s
  wenc_chain_ms         context: the same gradient by the single-chain strided GEMM
  ppo_update_ms / torch_update_ms   PPO.update (K_epochs = 1, Adam step included) and, as context, the same update through PyTorch-ROCm
                        autograd (nn.Conv2d / Linear / GRU) on the same stored roll-out: --rounds rounds, the two ALTERNATING within a
                        round, --steps calls each; median over rounds, with the smallest and largest round beside it
  full_batch_ms         train_stage2_batch end to end
Times are HIP-event means over --steps calls after --warmup calls unless said otherwise; one process, one device.

`--rollout` is a mode of its own (profiles/stage2_rollout_probe.json): for reward = 'random' and 'prev', `train_stage2_batch` (the step
loop) and `train_stage2_batch_fused` (all T steps in one batched pass) ALTERNATING within a round, --rounds rounds of --steps calls each
after a warm-up; the mean over rounds with the smallest and largest round beside it, the ratio of the means, and the fused body's parts
on their own (glance, policy roll-out, trunk pass over the sampled crops, the random crops' pass, classifier scan + baseline branch,
rewards, update).  It ASSERTS that the fused body is at least 1.5x faster than the step loop for both reward kinds (after writing --out).

Every GPU step runs under a time limit of its own and the steps are chained, so that a failure ends the run:

    timeout -k 10 300 rocprofv3 --kernel-trace -d TRACE -- python tools/stage2_train_probe.py --splitk-only && \
    timeout -k 10 420 python tools/stage2_train_probe.py --trace TRACE --out profiles/stage2_train_probe.json
    timeout -k 10 300 python tools/stage2_train_probe.py --rollout --out profiles/stage2_rollout_probe.json

Nothing is caught inside: an error in any part, the PyTorch context included, ends the process with a non-zero status.
"""
import argparse
import copy
import csv
import glob
import json
import statistics
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import hip_ops, synth, train  # noqa: E402
from adafocus_amd.gfv_net import GFV, random_crop_actions  # noqa: E402
from adafocus_amd.ppo import Memory  # noqa: E402
from tests.helpers import manifest  # noqa: E402

B, T, P, A, C, HW, H = 64, 16, 96, 49, 1280, 7, 1024
HBM_BPS = 6.3e12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def splitk_inputs(dev):
    """Two sets of (states, dE1, E1) at full size: calls alternate between them."""
    npix = T * B * HW * HW
    sets = []
    for seed in (1, 2):
        g = torch.Generator(device=dev).manual_seed(seed)
        s = torch.randn((npix, C), device=dev, generator=g) * 0.5
        de1 = torch.randn((npix, 32), device=dev, generator=g) * 1e-3
        e1 = torch.relu(torch.randn((npix, 32), device=dev, generator=g))
        sets.append((s, de1, e1))
    return sets


def splitk_calls(sets, calls):
    for i in range(calls):
        hip_ops.ppo_wenc_grad(*sets[i & 1], split_k=True)


def splitk_from_trace(d):
    """Median kernel time of the split-K kernel and of its reduce kernel over the launches of a --splitk-only trace."""
    us = {"splitk_wgrad_kernel": [], "slice_sum_kernel": []}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in us:
                if k in r["Kernel_Name"]:
                    us[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not us["splitk_wgrad_kernel"]:
        raise SystemExit("no split-K launches in the trace under %s" % d)
    npix = T * B * HW * HW
    chunks, slices = C // 256, 256 // (C // 256)
    k_us, r_us = statistics.median(us["splitk_wgrad_kernel"]), statistics.median(us["slice_sum_kernel"])
    state_bytes = npix * C * 4
    k_bytes = state_bytes + 2 * npix * 32 * 4 * chunks + slices * 32 * C * 4        # states once, both 32-wide operands per chunk, partials
    return dict(wenc_splitk_launches=len(us["splitk_wgrad_kernel"]), wenc_splitk_kernel_us=round(k_us, 2),
                wenc_splitk_kernel_us_min_max=[round(min(us["splitk_wgrad_kernel"]), 2), round(max(us["splitk_wgrad_kernel"]), 2)],
                wenc_reduce_kernel_us=round(r_us, 2), wenc_splitk_state_bytes=state_bytes, wenc_splitk_kernel_bytes=k_bytes,
                wenc_splitk_state_frac_of_6p3_tb_s=round(state_bytes / (k_us * 1e-6) / HBM_BPS, 3),
                wenc_splitk_bytes_frac_of_6p3_tb_s=round(k_bytes / (k_us * 1e-6) / HBM_BPS, 3))


def torch_update(ppo, pol, opt, states_nchw, actions, old, returns):
    t, b = actions.shape
    e = pol.state_encoder(states_nchw.view(t * b, C, HW, HW)).view(t, b, -1)
    out, _ = pol.gru(e, torch.zeros(1, b, H, device=e.device))
    s = out.reshape(t * b, -1)
    logp = torch.log_softmax(pol.actor[0](s), -1)
    lp = logp.gather(1, actions.reshape(-1, 1)).view(t, b)
    ent = -(logp.exp() * logp).sum(-1).view(t, b)
    val = pol.critic(s).view(t, b)
    ratios = torch.exp(lp - old)
    adv = returns - val.detach()
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - ppo.eps_clip, 1 + ppo.eps_clip) * adv)
            + 0.5 * torch.nn.functional.mse_loss(val, returns) - 0.01 * ent).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()


ROLLOUT_GATE = 1.5


def rollout_mode(a, dev):
    """The step loop against the fused body, alternating; see the module docstring."""
    res = {"probe": "stage2_rollout", "B": B, "T": T, "P": P, "A": A, "C": C, "H": H, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "calls_per_round": a.steps, "gate": ROLLOUT_GATE}
    images = torch.from_numpy(synth.synth_frames(B, T, 224, seed=5)).to(dev)
    target = torch.randint(0, 200, (B,), device=dev)
    for reward in ("random", "prev"):
        args = types.SimpleNamespace(num_segments=T, num_classes=200, reward=reward, dataset="actnet", input_size=224, batch_size=B,
                                     patch_size=P, with_glancer=True, feature_map_channels=C, glance_size=224, action_dim=A,
                                     hidden_state_dim=H, policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003,
                                     random_patch=False, dropout=0.5, consensus="gru", hidden_dim=1024, train_stage=2)
        model = GFV(args)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(manifest()["ACT"], 1007).items()}, strict=True)
        model = model.to(dev)
        model.policy_train_mode()

        def loop():
            return train.train_stage2_batch(model, images, target, args)

        def fused():
            return train.train_stage2_batch_fused(model, images, target, args)
        timed(loop, 1, 2)
        timed(fused, 1, 2)
        ours, theirs = [], []
        for _ in range(a.rounds):
            theirs.append(timed(loop, a.steps, 0))
            ours.append(timed(fused, a.steps, 0))
        r = {"step_loop_ms": round(statistics.mean(theirs), 4), "step_loop_ms_min_max": [round(min(theirs), 4), round(max(theirs), 4)],
             "fused_ms": round(statistics.mean(ours), 4), "fused_ms_min_max": [round(min(ours), 4), round(max(ours), 4)]}
        r["speedup"] = round(statistics.mean(theirs) / statistics.mean(ours), 3)
        # the fused body's parts, each on its own (the sum leaves out what overlaps and the host work between the parts)
        foc, cls, mem = model.focuser, model.classifier, model.focuser.memory
        flat = images.view(B * T, 3, 224, 224)
        table = foc.action_table(dev)
        with torch.no_grad():
            r["glance_ms"] = round(timed(lambda: model.glance(images), a.steps, a.warmup), 4)
            fmap, fvec = model.glance(images)
            nhwc = fmap.permute(0, 1, 3, 4, 2).reshape(B * T, HW, HW, C)

            def policy():
                mem.clear_memory()
                return foc.policy.policy_old.act_rollout_nhwc(nhwc, B, T, mem, table)
            r["policy_rollout_ms"] = round(timed(policy, a.steps, a.warmup), 4)
            _, coords = policy()
            r["trunk_pass_ms"] = round(timed(lambda: model.hot_path_features(flat, fvec, coords, B, T), a.steps, a.warmup), 4)
            feature = model.hot_path_features(flat, fvec, coords, B, T)

            def random_crops():
                return torch.from_numpy(np.stack([random_crop_actions(B, 224, 224, P) for _ in range(T)], 1).reshape(B * T, 2)).to(dev)
            r["random_crop_draw_ms"] = round(timed(random_crops, a.steps, a.warmup), 4)

            def classifier():
                logits, _, _, hs = cls._steps_from(feature, None, want_hs=True)
                return logits, cls.branch_forward(feature, hs)
            r["classifier_ms"] = round(timed(classifier, a.steps, a.warmup), 4)
            logits, base = classifier()
            r["rewards_ms"] = round(timed(lambda: hip_ops.ppo_rewards(logits, base, target, T, reward, want_ce_last=True), a.steps, a.warmup), 4)
            rewards = hip_ops.ppo_rewards(logits, base, target, T, reward)
        mem.rewards.extend(rewards[s:s + 1] for s in range(T))
        stored = Memory()
        for name in ("states", "actions", "logprobs", "rewards"):
            getattr(stored, name).extend(getattr(mem, name))
        r["ppo_update_ms"] = round(timed(lambda: foc.policy.update(stored), a.steps, a.warmup), 4)
        mem.clear_memory()
        assert hip_ops.gru_scan_timeouts() == 0
        res[reward] = r
        del model, stored, fmap, fvec, nhwc, feature, logits, base
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for reward in ("random", "prev"):
        assert res[reward]["speedup"] >= ROLLOUT_GATE, "fused body %.2fx the step loop for reward %r: below %.1fx" % (
            res[reward]["speedup"], reward, ROLLOUT_GATE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rollout", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--splitk-calls", type=int, default=200)
    ap.add_argument("--splitk-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if a.rollout:
        rollout_mode(a, dev)
        return
    if a.splitk_only:
        sets = splitk_inputs(dev)
        splitk_calls(sets, 20)
        torch.cuda.synchronize()
        splitk_calls(sets, a.splitk_calls)
        torch.cuda.synchronize()
        print(json.dumps({"splitk_only_calls": a.splitk_calls + 20}))
        return
    args = types.SimpleNamespace(num_segments=T, num_classes=200, reward="random", dataset="actnet", input_size=224, batch_size=B,
                                 patch_size=P, with_glancer=True, feature_map_channels=C, glance_size=224, action_dim=A,
                                 hidden_state_dim=H, policy_conv=True, gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003,
                                 random_patch=False, dropout=0.5, consensus="gru", hidden_dim=1024, train_stage=2)
    model = GFV(args)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(manifest()["ACT"], 1007).items()}, strict=True)
    model = model.to(dev)
    model.policy_train_mode()
    images = torch.from_numpy(synth.synth_frames(B, T, 224, seed=5)).to(dev)
    target = torch.randint(0, 200, (B,), device=dev)
    ppo, pol = model.focuser.policy, model.focuser.policy.policy
    res = {"probe": "stage2_train", "B": B, "T": T, "P": P, "A": A, "C": C, "H": H, "device": torch.cuda.get_device_name(0)}

    def rollout(keep=None):
        mem = model.focuser.memory
        mem.clear_memory()
        fmap, fvec = model.glance(images)
        frames = images.view(B, T, 3, 224, 224)
        last = 0
        for s in range(T):
            out, _, _, base = model.one_step_act(frames[:, s], fmap[:, s], fvec[:, s], restart_batch=s == 0, training=True)
            conf = torch.gather(torch.softmax(out, 1), 1, target.view(-1, 1)).view(1, -1)
            bconf = torch.gather(torch.softmax(base, 1), 1, target.view(-1, 1)).view(1, -1)
            r, last = train.get_reward(args, conf, last, bconf)
            mem.rewards.append(r)
    with torch.no_grad():
        res["rollout_ms"] = round(timed(rollout, a.steps, 2), 4)
        rollout()
    src = model.focuser.memory
    stored = Memory()
    for name in ("states", "actions", "logprobs", "rewards"):
        getattr(stored, name).extend(x.clone() for x in getattr(src, name))
    src.clear_memory()
    rewards = torch.cat([r.reshape(1, -1) for r in stored.rewards], 0)
    states = torch.stack([s.permute(0, 2, 3, 1) for s in stored.states], 0).contiguous()
    actions, old = torch.stack(stored.actions), torch.stack(stored.logprobs)
    res["returns_ms"] = round(timed(lambda: hip_ops.ppo_returns(rewards, ppo.gamma), a.steps, a.warmup), 4)
    returns = hip_ops.ppo_returns(rewards, ppo.gamma)
    res["evaluate_fwd_ms"] = round(timed(lambda: pol._train_forward(states), a.steps, a.warmup), 4)
    fwd = pol._train_forward(states)
    res["loss_head_ms"] = round(timed(lambda: hip_ops.ppo_loss_head(fwd["head"], actions, old, returns, ppo.eps_clip), a.steps, a.warmup), 4)
    dhead = hip_ops.ppo_loss_head(fwd["head"], actions, old, returns, ppo.eps_clip)[4]
    x = fwd["e_bt"].view(B, T, -1)

    def gru_bwd():
        return hip_ops.gru_cls_backward(x, fwd["w_ih"], fwd["w_hh"], fwd["b_hh"], fwd["head_w"], fwd["gi"], fwd["hs"], None, dhead)
    res["gru_heads_bwd_ms"] = round(timed(gru_bwd, a.steps, a.warmup), 4)
    dx = gru_bwd()[0]
    e1 = fwd["e1"].view(T * B, -1)
    res["encoder_bwd_ms"] = round(timed(lambda: hip_ops.ppo_encoder_backward(fwd["states"], e1, fwd["e_bt"], dx, T, B, fwd["w_lin"]),
                                        a.steps, a.warmup), 4)
    npix = T * B * HW * HW
    s2, e2 = fwd["states"].view(npix, C), fwd["e1"].view(npix, 32)
    de1 = torch.randn_like(e2) * 1e-3
    res["wenc_chain_ms"] = round(timed(lambda: hip_ops.ppo_wenc_grad(s2, de1, e2, split_k=False), 5, 1), 4)
    assert hip_ops.gru_scan_timeouts() == 0

    # the whole update, ours and PyTorch's, from the same starting weights on the same stored roll-out, alternating
    torch_pol = copy.deepcopy(pol)
    torch_opt = torch.optim.Adam(torch_pol.parameters(), lr=ppo.lr, betas=ppo.betas)
    states_nchw = states.permute(0, 1, 4, 2, 3).contiguous()

    def ref():
        ret = hip_ops.ppo_returns(rewards, ppo.gamma)
        torch_update(ppo, torch_pol, torch_opt, states_nchw, actions, old, ret)
    ours, theirs = [], []
    timed(lambda: ppo.update(stored), 1, a.warmup)
    timed(ref, 1, a.warmup)
    for _ in range(a.rounds):
        ours.append(timed(lambda: ppo.update(stored), a.steps, 1))
        theirs.append(timed(ref, a.steps, 1))
    res.update(ppo_update_ms=round(statistics.median(ours), 4), ppo_update_ms_min_max=[round(min(ours), 4), round(max(ours), 4)],
               torch_update_ms=round(statistics.median(theirs), 4), torch_update_ms_min_max=[round(min(theirs), 4), round(max(theirs), 4)],
               update_rounds=a.rounds, update_calls_per_round=a.steps)
    res["update_vs_torch"] = ("faster" if max(ours) < min(theirs) else "slower" if min(ours) > max(theirs) else "parity")
    del fwd, states, states_nchw, s2, e2, de1, dx
    torch.cuda.empty_cache()
    res["full_batch_ms"] = round(timed(lambda: train.train_stage2_batch(model, images, target, args), a.steps, 2), 4)
    del model, images
    torch.cuda.empty_cache()
    sets = splitk_inputs(dev)
    splitk_calls(sets, 20)
    res["wenc_splitk_call_ms"] = round(timed(lambda: splitk_calls(sets, a.splitk_calls), 1, 0) / a.splitk_calls, 4)
    res["wenc_splitk_calls"] = a.splitk_calls
    if a.trace:
        res.update(splitk_from_trace(a.trace))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
