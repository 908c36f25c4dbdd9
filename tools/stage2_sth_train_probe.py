#!/usr/bin/env python3
"""Stage-2 step of the Something-Something model on one MI355X at the shipped shape (B = 64, Tg = 8, Tf = 12, P = 144, video_div = 1,
continuous policy with BatchNorm: 10 240 input channels, 7 x 7 map, H = 1024): one JSON line with ms per call of

  full_batch_ms         train_stage2_batch_sth end to end
  glance_ms             the glancer over B * Tg frames
  policy_step_ms        policy_old.act_nhwc(training=True): dense state, encoder with batch statistics, GRU step, actor, sampling
  trunk_pass_ms         the TSM trunk over the B * Tf sampled patches AND the B * Tf baseline patches (they ride in one pass), and
  trunk_main_only_ms    the same over the sampled patches alone, as context
  fc_rewards_ms         FC + consensus of both halves, softmax confidences, reward
  update_ms             PPO_Continuous.update (K_epochs = 1, Adam step included), and its parts on their own:
  returns_ms, forward_ms, loss_head_ms, gru_heads_bwd_ms, encoder_bwd_ms
  torch_update_ms       context: the same update through PyTorch-ROCm autograd on nn modules (Conv2d / BatchNorm / Linear / GRU) in the same
                        process
  wenc_splitk_ms / wenc_chain_ms   the 64-output weight gradient in its streaming form and as the single chain on the strided GEMM
full_batch, update / torch_update and wenc_splitk / wenc_chain are measured over --rounds rounds (the members of a pair ALTERNATING within
a round) of --steps calls each: the mean over rounds with the smallest and largest round beside it (HIP events).  The parts are HIP-event
means over --steps calls after --warmup calls.
  wenc_splitk_kernel_us with --trace DIR: the kernel's own time (median over its launches in a rocprofv3 --kernel-trace of a
                        `--splitk-only` run that rotates over two state buffers), the reduce kernel's, and the bytes the kernel moves over
                        that time as a fraction of 6.3 TB/s

    timeout -k 10 300 rocprofv3 --kernel-trace -d TRACE -- python tools/stage2_sth_train_probe.py --splitk-only && \
    timeout -k 10 420 python tools/stage2_sth_train_probe.py --trace TRACE --out profiles/stage2_sth_probe.json

Nothing is caught inside: an error in any part ends the process with a non-zero status.
"""
import argparse
import copy
import csv
import glob
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from adafocus_amd import hip_ops, synth, train  # noqa: E402
from adafocus_amd.gfv_net_sth import GFV  # noqa: E402
from adafocus_amd.ppo import Memory  # noqa: E402
from adafocus_amd.utils import get_patch_nhwc4  # noqa: E402
from tests.helpers import synth_sd  # noqa: E402
from tests.test_state_dict_compat import sth_args  # noqa: E402

B, TG, TF, P, C, HW, H, CMID = 64, 8, 12, 144, 1280, 7, 1024, 64
NPIX, CIN = B * HW * HW, TG * C
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


def alternating(fns, rounds, steps):
    """{name: (mean over rounds, smallest round, largest round)} with the functions taking turns inside every round."""
    for fn in fns.values():
        timed(fn, 1, 2)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, steps, 0))
    return {k: (round(statistics.mean(v), 4), round(min(v), 4), round(max(v), 4)) for k, v in ms.items()}


def splitk_inputs(dev):
    """Two sets of (states, dC) at the shipped size: calls alternate between them (no call reads what the previous one left in a cache)."""
    sets = []
    for seed in (1, 2):
        g = torch.Generator(device=dev).manual_seed(seed)
        sets.append((torch.randn((NPIX, CIN), device=dev, generator=g) * 0.5, torch.randn((NPIX, CMID), device=dev, generator=g) * 1e-3))
    return sets


def splitk_calls(sets, calls, split_k=True):
    for i in range(calls):
        hip_ops.ppo_wenc_grad(sets[i & 1][0], sets[i & 1][1], None, split_k=split_k)


def splitk_from_trace(d):
    us = {"splitk_wgrad_kernel": [], "slice_sum_kernel": []}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in us:
                if k in r["Kernel_Name"]:
                    us[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if not us["splitk_wgrad_kernel"]:
        raise SystemExit("no split-K launches in the trace under %s" % d)
    chunks = CIN // 128
    slices = max(1, min(256 // chunks, (NPIX + 63) // 64))
    k_us, r_us = statistics.median(us["splitk_wgrad_kernel"]), statistics.median(us["slice_sum_kernel"])
    state_bytes = NPIX * CIN * 4
    k_bytes = state_bytes + NPIX * CMID * 4 * chunks + slices * CMID * CIN * 4        # states once, the 64-wide gradient per chunk, partials
    return dict(wenc_splitk_launches=len(us["splitk_wgrad_kernel"]), wenc_splitk_kernel_us=round(k_us, 2),
                wenc_splitk_kernel_us_min_max=[round(min(us["splitk_wgrad_kernel"]), 2), round(max(us["splitk_wgrad_kernel"]), 2)],
                wenc_reduce_kernel_us=round(r_us, 2), wenc_splitk_state_bytes=state_bytes, wenc_splitk_kernel_bytes=k_bytes,
                wenc_splitk_state_frac_of_6p3_tb_s=round(state_bytes / (k_us * 1e-6) / HBM_BPS, 3),
                wenc_splitk_bytes_frac_of_6p3_tb_s=round(k_bytes / (k_us * 1e-6) / HBM_BPS, 3))


def torch_update(ppo, pol, opt, states, actions, old, returns):
    """The reference's update (STH/models/ppo_continuous.py:111-139,181-194) on nn modules through PyTorch-ROCm autograd."""
    t, b = actions.shape[:2]
    e = pol.state_encoder(states.view(t * b, CIN, HW, HW)).view(t, b, -1)
    out, _ = pol.gru(e, torch.zeros(1, b, H, device=e.device))
    s = out.reshape(t * b, -1)
    dist = torch.distributions.MultivariateNormal(pol.actor(s), scale_tril=torch.diag(torch.full((2,), pol.action_std, device=s.device)))
    lp = dist.log_prob(actions.view(t * b, 2)).view(t, b)
    ent = dist.entropy().view(t, b)
    val = pol.critic(s).view(t, b)
    ratios = torch.exp(lp - old)
    adv = returns - val.detach()
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - ppo.eps_clip, 1 + ppo.eps_clip) * adv)
            + 0.5 * torch.nn.functional.mse_loss(val, returns) - 0.01 * ent).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()


def main():
    ap = argparse.ArgumentParser()
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
    if a.splitk_only:
        sets = splitk_inputs(dev)
        splitk_calls(sets, 20)
        torch.cuda.synchronize()
        splitk_calls(sets, a.splitk_calls)
        torch.cuda.synchronize()
        print(json.dumps({"splitk_only_calls": a.splitk_calls + 20}))
        return
    args = sth_args()
    args.gpu, args.video_div, args.num_segments_glancer, args.num_segments_focuser, args.patch_size, args.batch_size = 0, 1, TG, TF, P, B
    model = GFV(args).eval()
    model.focuser.net.base_model = torch.nn.Sequential(*list(model.focuser.net.base_model.children())[:-1])
    model.load_state_dict(synth_sd("STH", 1007), strict=True)
    policy_sd = {k[len("policy."):]: v for k, v in synth_sd("STH_POLICY", 1007).items()}
    ppo = model.focuser.policy
    ppo.policy.load_state_dict(policy_sd)
    ppo.policy_old.load_state_dict(policy_sd)
    model = model.to(dev)
    model.policy_train_mode()
    pol, mem = ppo.policy, model.focuser.memory
    gl = torch.from_numpy(synth.synth_frames(B, TG, 224, seed=3)).to(dev)
    fo = torch.from_numpy(synth.synth_frames(B, TF, 224, seed=4)).to(dev)
    target = torch.randint(0, args.num_classes, (B,), device=dev)
    res = {"probe": "stage2_sth_train", "B": B, "Tg": TG, "Tf": TF, "P": P, "channels": CIN, "H": H, "with_bn": True,
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_round": a.steps}

    def batch():
        return train.train_stage2_batch_sth(model, gl, fo, target, args)
    full = alternating({"full_batch": batch}, a.rounds, max(1, a.steps // 2))["full_batch"]
    res.update(full_batch_ms=full[0], full_batch_ms_min_max=list(full[1:]))

    # ---- the parts of the roll-out
    with torch.no_grad():
        res["glance_ms"] = round(timed(lambda: model.glance(gl), a.steps, a.warmup), 4)
        fm, glog = model.glance(gl)
        nhwc = fm.permute(0, 1, 3, 4, 2).contiguous().view(B * TG, HW, HW, C)

        def policy_step():
            mem.clear_memory()
            return ppo.policy_old.act_nhwc(nhwc, B, TG, mem, restart_batch=True, training=True)
        res["policy_step_ms"] = round(timed(policy_step, a.steps, a.warmup), 4)
        action = policy_step()
        cur = fo.view(B * TF, 3, 224, 224)
        main4 = get_patch_nhwc4(cur, action, P, TF)
        base4 = get_patch_nhwc4(cur, torch.rand(B, 2, device=dev), P, TF)
        both = torch.cat([main4, base4], 0)
        net = model.focuser.net
        res["trunk_pass_ms"] = round(timed(lambda: net.features_nhwc4(both), a.steps, a.warmup), 4)
        res["trunk_main_only_ms"] = round(timed(lambda: net.features_nhwc4(main4), a.steps, a.warmup), 4)
        feat = net.features_nhwc4(both)
        w, bias = model.classifier.weight.detach(), model.classifier.bias.detach()

        def fc_rewards():
            lg = [hip_ops.fc_meanpool_forward(feat[k * B * TF:(k + 1) * B * TF], B, w, bias, glog) for k in range(2)]
            conf = [torch.softmax(x, 1).gather(1, target.view(-1, 1)).view(1, -1) for x in lg]
            return conf[0] - conf[1]
        res["fc_rewards_ms"] = round(timed(fc_rewards, a.steps, a.warmup), 4)
        reward = fc_rewards()
    mem.rewards.append(reward)
    stored = Memory()
    for name in ("states", "actions", "logprobs", "rewards"):
        getattr(stored, name).extend(x.clone() for x in getattr(mem, name))
    mem.clear_memory()
    del both, main4, base4, feat

    # ---- the parts of the update
    rewards = torch.cat([r.reshape(1, -1) for r in stored.rewards], 0)
    states = pol._states_dense(torch.stack([s.permute(0, 2, 3, 1) for s in stored.states], 0))
    actions, old = torch.stack(stored.actions), torch.stack(stored.logprobs)
    sigma = pol.action_std
    with torch.no_grad():
        res["returns_ms"] = round(timed(lambda: hip_ops.ppo_returns(rewards, ppo.gamma), a.steps, a.warmup), 4)
        returns = hip_ops.ppo_returns(rewards, ppo.gamma)
        res["forward_ms"] = round(timed(lambda: pol._train_forward(states), a.steps, a.warmup), 4)
        fwd = pol._train_forward(states)
        res["loss_head_ms"] = round(timed(lambda: hip_ops.ppo_gauss_loss_head(fwd["head"], actions, sigma, old, returns, ppo.eps_clip),
                                          a.steps, a.warmup), 4)
        dhead = hip_ops.ppo_gauss_loss_head(fwd["head"], actions, sigma, old, returns, ppo.eps_clip)[4]
        x = fwd["e_bt"].view(B, 1, -1)

        def gru_bwd():
            return hip_ops.gru_cls_backward(x, fwd["w_ih"], fwd["w_hh"], fwd["b_hh"], fwd["head_w"], fwd["gi"], fwd["hs"], None, dhead)
        res["gru_heads_bwd_ms"] = round(timed(gru_bwd, a.steps, a.warmup), 4)
        dx = gru_bwd()[0]
        bn = tuple(fwd[k] for k in ("c1", "gamma1", "mean1", "invstd1", "l1", "gamma2", "mean2", "invstd2"))
        res["encoder_bwd_ms"] = round(timed(lambda: hip_ops.ppo_encoder_backward(fwd["states"], fwd["e1"], fwd["e_bt"], dx, 1, B,
                                                                                fwd["w_lin"], bn), a.steps, a.warmup), 4)
    assert hip_ops.gru_scan_timeouts() == 0
    del fwd, dx, bn

    # ---- the whole update, ours and PyTorch's, from the same starting weights on the same stored roll-out, alternating
    torch_pol = copy.deepcopy(pol).train()
    torch_opt = torch.optim.Adam(torch_pol.parameters(), lr=ppo.lr, betas=ppo.betas)
    states_nchw = states.permute(0, 1, 4, 2, 3).contiguous()

    def ref():
        torch_update(ppo, torch_pol, torch_opt, states_nchw, actions, old, hip_ops.ppo_returns(rewards, ppo.gamma))
    upd = alternating({"update": lambda: ppo.update(stored), "torch_update": ref}, a.rounds, a.steps)
    res.update(update_ms=upd["update"][0], update_ms_min_max=list(upd["update"][1:]), torch_update_ms=upd["torch_update"][0],
               torch_update_ms_min_max=list(upd["torch_update"][1:]))
    res["update_vs_torch"] = ("faster" if upd["update"][2] < upd["torch_update"][1] else
                              "slower" if upd["update"][1] > upd["torch_update"][2] else "parity")
    del model, states, states_nchw, torch_pol, stored, gl, fo
    torch.cuda.empty_cache()

    # ---- the 64-output weight gradient: streaming form against the single chain, alternating
    sets = splitk_inputs(dev)
    calls = 20
    w = alternating({"splitk": lambda: splitk_calls(sets, calls), "chain": lambda: splitk_calls(sets, 2, split_k=False)}, a.rounds, 1)
    res.update(wenc_splitk_ms=round(w["splitk"][0] / calls, 4), wenc_splitk_ms_min_max=[round(v / calls, 4) for v in w["splitk"][1:]],
               wenc_chain_ms=round(w["chain"][0] / 2, 4), wenc_chain_ms_min_max=[round(v / 2, 4) for v in w["chain"][1:]])
    res["wenc_splitk_vs_chain"] = "faster" if w["splitk"][2] / calls < w["chain"][1] / 2 else "slower" if w["splitk"][1] / calls > w["chain"][2] / 2 else "parity"
    if a.trace:
        res.update(splitk_from_trace(a.trace))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
