#!/usr/bin/env python3
"""Stage-2 fixture: the roll-out and one PPO update of the REAL reference policy (ACT/models/ppo.py), imported exactly like
tools/gen_golden.py does (its shims; no reference source is copied).  Writes tests/golden/g18_act_stage2.npz.

Real dimensions (C = 1280, 7 x 7 map, A = 49, H = 1024), B = 4, T = 4.  Weights come from gen_golden.load_synth (seed SEED_W; the `clip`
case's policy_old from a second seed), states from GG.rnd (seed SEED_S), rewards from seed SEED_R: none of them is stored.

  rollout_*  T steps of policy_old.act(training=True) under torch.manual_seed(SEED_T): per step the actor probabilities, the sampled
             action, its log-probability and the hidden state.  The torch seed is searched until every sampled action has a probability of
             at least PROB_FLOOR, so a test that feeds the midpoint of the action's interval of the CDF has PROB_FLOOR / 2 of margin.
  same_*     PPO.update with policy_old == policy (ratios are 1 up to rounding), K_epochs = 1.
  clip_*     policy_old from a second weight seed, searched until the ratios fall below 1 - eps_clip and above 1 + eps_clip, each with a
             positive and with a negative advantage (>= 1 entry in each of the four classes), with the decision margins -- the smallest
             |ratio - (1 +- eps_clip)| and the smallest |surr1 - surr2| where they differ -- above RATIO_MARGIN_MIN / SURR_GAP_MIN.
             K_epochs = 2: the second epoch runs on updated weights.
For `same` and `clip`: normalised returns, evaluate's three outputs, loss.mean() and the gradients before the first optimizer step -- the
biases, actor.0.weight, critic.0.weight and state_encoder.0.weight in full; state_encoder.3.weight, gru.weight_ih_l0 and gru.weight_hh_l0
as the fixed random projections G v (v of seed 174+i) and u^T G (u of seed 184+i) of G17.  They are read off the running update (the
optimizer's first step, the loss's backward call and the MSE term's arguments are observed), not recomputed.
`spread_*`: the same step by the reference module in float64 on the same inputs, relative difference per quantity.
`reward_*`: the reference's get_reward (ACT/main_dist.py:574-581) for 'prev', 'conf', 'random'.

Usage:  python tools/gen_golden_stage2.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_golden_depths import save_stable  # noqa: E402

SEED_W, SEED_S, SEED_R = 1818, 181, 182
B, T, C, HW, A, H = 4, 4, 1280, 7, 49, 1024
EPS_CLIP, GAMMA = 0.2, 0.7
PROB_FLOOR = 1e-3          # 10x the 1e-4 by which the HIP policy's logits (hence its CDF) may differ from the reference's
RATIO_MARGIN_MIN = 1e-3    # 100x the ~1e-5 relative error of a ratio from log-probabilities that differ by ~1e-5
SURR_GAP_MIN = 1e-4
FULL = ("state_encoder.3.bias", "gru.bias_ih_l0", "gru.bias_hh_l0", "actor.0.bias", "critic.0.bias", "actor.0.weight", "critic.0.weight",
        "state_encoder.0.weight")
PROJECTED = ("state_encoder.3.weight", "gru.weight_ih_l0", "gru.weight_hh_l0")


def states():
    return GG.rnd((T, B, C, HW, HW), SEED_S, 0.5)


def rewards():
    return GG.rnd((T, 1, B), SEED_R, 0.3)


def rollout(P, weight_seed, torch_seed):
    """T sampled steps of a policy with synthetic weights: (memory, probs, hidden)."""
    pol = P.ActorCritic(C, C * HW * HW, A, H, True)
    GG.load_synth(pol, weight_seed)
    pol.train()
    mem = P.Memory()
    s = torch.from_numpy(states())
    probs, hidden = [], []
    torch.manual_seed(torch_seed)
    with torch.no_grad():
        for t in range(T):
            pol.act(s[t], mem, restart_batch=t == 0, training=True)
            hidden.append(mem.hidden[-1][0].clone())
            probs.append(pol.actor(mem.hidden[-1][0]))
    return mem, torch.stack(probs).numpy(), torch.stack(hidden).numpy()


def update(P, mem, old_seed, k_epochs, dtype):
    """PPO.update of the reference on a copy of `mem` in `dtype`, observed: {quantity: float64 array}."""
    torch.set_default_dtype(dtype)
    try:
        ppo = P.PPO(C, C * HW * HW, A, H, True, gpu=None, gamma=GAMMA, K_epochs=k_epochs, eps_clip=EPS_CLIP)
        GG.load_synth(ppo.policy, SEED_W)
        GG.load_synth(ppo.policy_old, old_seed)
        ppo = ppo.to(dtype)
        ppo.policy.train()
        ppo.policy_old.train()
        # (the optimizer was built on the fp32 parameters; .to(dtype) keeps the Parameter objects)
        m = P.Memory()
        m.states = [s.to(dtype) for s in mem.states]
        m.actions = list(mem.actions)
        m.logprobs = [v.to(dtype) for v in mem.logprobs]
        m.rewards = [torch.from_numpy(r).to(dtype) for r in rewards()]
        seen = {}
        evaluate, step, mse, backward = ppo.policy.evaluate, ppo.optimizer.step, ppo.MseLoss, torch.Tensor.backward

        def ev(*a, **k):
            out = evaluate(*a, **k)
            if "logprobs" not in seen:
                seen["logprobs"], seen["values"], seen["entropy"] = (o.detach().clone() for o in out)
            return out

        class Observed(torch.nn.Module):
            def forward(self, values, target):
                seen.setdefault("returns", target.detach().clone())
                return mse(values, target)

        def bw(self, *a, **k):
            seen.setdefault("loss", self.detach().clone().reshape(1))
            return backward(self, *a, **k)

        def st(*a, **k):
            if "grads" not in seen:
                seen["grads"] = {n: p.grad.detach().clone() for n, p in ppo.policy.named_parameters()}
            return step(*a, **k)

        ppo.policy.evaluate, ppo.optimizer.step, ppo.MseLoss, torch.Tensor.backward = ev, st, Observed(), bw
        try:
            ppo.update(m)
        finally:
            torch.Tensor.backward = backward
        for (n, p), (_, q) in zip(ppo.policy.named_parameters(), ppo.policy_old.named_parameters()):
            assert torch.equal(p, q), n
        out = {k: seen[k] for k in ("returns", "logprobs", "values", "entropy", "loss")}
        for n in FULL:
            out[n] = seen["grads"][n]
        for i, n in enumerate(PROJECTED):
            g = seen["grads"][n]
            out[n + "@v"] = g @ torch.from_numpy(GG.rnd((g.shape[1],), 174 + i)).to(dtype)
            out["u@" + n] = torch.from_numpy(GG.rnd((g.shape[0],), 184 + i)).to(dtype) @ g
        return {k: v.double().numpy() for k, v in out.items()}
    finally:
        torch.set_default_dtype(torch.float32)


def clip_classes(r, mem):
    """Ratios, advantages, the four clip classes' counts and the two decision margins of an observed update."""
    old = torch.stack(mem.logprobs).double().numpy()
    ratio = np.exp(r["logprobs"] - old)
    adv = r["returns"].reshape(T, B) - r["values"]
    lo, hi = 1 - EPS_CLIP, 1 + EPS_CLIP
    counts = [int(((ratio < lo) & (adv > 0)).sum()), int(((ratio < lo) & (adv < 0)).sum()),
              int(((ratio > hi) & (adv > 0)).sum()), int(((ratio > hi) & (adv < 0)).sum())]
    ratio_margin = min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min())
    surr1, surr2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    differ = surr1 != surr2
    surr_gap = np.abs(surr1 - surr2)[differ].min() if differ.any() else 0.0
    return ratio, adv, counts, float(ratio_margin), float(surr_gap)


def reward_cases(arrays):
    """main_dist.get_reward (ACT/main_dist.py:574-581): the driver module itself needs hydra and the data pipeline to import, so the one
    function is compiled from the reference's file as it stands (its syntax-tree node, nothing restated here)."""
    import ast
    path = os.path.join(GG.ACT, "main_dist.py")
    node = next(n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == "get_reward")
    ns = {}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    M = types.SimpleNamespace(get_reward=ns["get_reward"])
    conf, last, base = (np.abs(GG.rnd((1, B), 190 + i, 0.3)).clip(0, 1) for i in range(3))
    arrays["reward_conf"], arrays["reward_last"], arrays["reward_base"] = conf, last, base
    for kind in ("prev", "conf", "random"):
        r, carry = M.get_reward(GG.Args(reward=kind), torch.from_numpy(conf), torch.from_numpy(last), torch.from_numpy(base))
        arrays["reward_%s" % kind] = r.numpy()
        assert torch.equal(carry, torch.from_numpy(conf))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG._install_shims()
    GG._enter_tree(GG.ACT)
    import models.ppo as P
    arrays = {"dims": np.array([B, T, C, HW, A, H]), "eps_clip": np.array([EPS_CLIP]), "gamma": np.array([GAMMA]),
              "floors": np.array([PROB_FLOOR, RATIO_MARGIN_MIN, SURR_GAP_MIN])}

    # ---- roll-out: a torch seed whose every sampled action clears the probability floor
    for seed_t in range(100, 164):
        mem, probs, hidden = rollout(P, SEED_W, seed_t)
        act = torch.stack(mem.actions).numpy()
        p_act = np.take_along_axis(probs, act[..., None], 2)[..., 0]
        if p_act.min() >= PROB_FLOOR:
            break
    else:
        raise AssertionError("no torch seed clears the probability floor")
    assert np.abs(np.log(p_act) - torch.stack(mem.logprobs).numpy()).max() < 1e-5
    print("  rollout: torch seed %d, smallest sampled probability %.4f, largest probability %.4f" % (seed_t, p_act.min(), probs.max()))
    arrays.update(rollout_probs=probs, rollout_actions=act, rollout_logprobs=torch.stack(mem.logprobs).numpy(), rollout_hidden=hidden,
                  rollout_torch_seed=np.array([seed_t]))

    # ---- same: policy_old == policy (the roll-out above is policy_old's)
    cases = [("same", SEED_W, 1, mem)]
    # ---- clip: policy_old from a second weight seed, searched for the four classes and the margins
    for seed_old in range(2000, 2064):
        mem2, _, _ = rollout(P, seed_old, seed_t)
        r = update(P, mem2, seed_old, 2, torch.float32)
        ratio, adv, counts, ratio_margin, surr_gap = clip_classes(r, mem2)
        print("  clip candidate %d: classes %s, ratio margin %.2e, surrogate gap %.2e" % (seed_old, counts, ratio_margin, surr_gap))
        if min(counts) >= 1 and ratio_margin >= RATIO_MARGIN_MIN and surr_gap >= SURR_GAP_MIN:
            break
    else:
        raise AssertionError("no second weight seed gives the four clip classes with the margins")
    cases.append(("clip", seed_old, 2, mem2))
    arrays.update(clip_old_seed=np.array([seed_old]), clip_actions=torch.stack(mem2.actions).numpy(),
                  clip_old_logprobs=torch.stack(mem2.logprobs).numpy(), clip_classes=np.array(counts),
                  clip_margins=np.array([ratio_margin, surr_gap]), seeds=np.array([SEED_W, SEED_S, SEED_R, seed_t, seed_old]))
    assert min(counts) >= 1 and ratio_margin >= RATIO_MARGIN_MIN and surr_gap >= SURR_GAP_MIN

    for tag, seed_old, k, m in cases:
        r32 = update(P, m, seed_old, k, torch.float32)
        r64 = update(P, m, seed_old, k, torch.float64)
        if tag == "same":
            ratio = clip_classes(r32, m)[0]
            assert np.abs(ratio - 1).max() < 1e-4, np.abs(ratio - 1).max()
        for key in r32:
            arrays["%s_%s" % (tag, key)] = r32[key].astype(np.float32)
            spread = np.abs(r32[key] - r64[key]).max() / max(np.abs(r64[key]).max(), 1e-30)
            assert 0 < spread < 1e-5, (tag, key, spread)
            arrays["spread_%s_%s" % (tag, key)] = np.array([spread])
            print("  %-5s %-26s max %.3e  fp32-vs-fp64 %.2e" % (tag, key, np.abs(r64[key]).max(), spread))
    reward_cases(arrays)
    save_stable("g18_act_stage2", **arrays)


if __name__ == "__main__":
    main()
