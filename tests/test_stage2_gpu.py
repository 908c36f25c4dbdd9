"""Stage-2 training on the MI355X: the sampling roll-out, the returns, the PPO loss head and the HIP backward of the policy
(csrc/ppo_train.hip + csrc/gru_bptt.hip) against the reference (G18), against CPU autograd of a float64 restatement at full size, the
split-K weight gradient against the single-chain GEMM, and the stage-2 loop body end to end."""
import copy
import os
import types

import numpy as np
import pytest
import torch

from adafocus_amd import evaluate, hip_ops, synth, train
from adafocus_amd.gfv_net import GFV
from adafocus_amd.ppo import PARAM_NAMES, PPO, ActorCritic, Memory
from tests.helpers import manifest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g18_act_stage2.npz")
DEV = torch.device("cuda:0")
FULL = ("state_encoder.3.bias", "gru.bias_ih_l0", "gru.bias_hh_l0", "actor.0.bias", "critic.0.bias", "actor.0.weight", "critic.0.weight",
        "state_encoder.0.weight")
PROJECTED = ("state_encoder.3.weight", "gru.weight_ih_l0", "gru.weight_hh_l0")


def _rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64([seed, 0xBEEF]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def _load_synth(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()})
    return module


def _ppo(a=49, c=1280, hw=7, h=1024, seed=1818, old_seed=None, k_epochs=1):
    ppo = PPO(c, c * hw * hw, a, h, True, gamma=0.7, K_epochs=k_epochs, eps_clip=0.2)
    _load_synth(ppo.policy, seed)
    _load_synth(ppo.policy_old, seed if old_seed is None else old_seed)
    ppo.policy.train()
    ppo.policy_old.train()
    return ppo


# ---- 1. sampling ------------------------------------------------------------------------------------------------------------------------
def test_sampling_matches_the_reference_rollout_g18():
    """Every recorded step of the reference's policy_old.act(training=True): u = the midpoint of the recorded action's interval of the
    reference CDF (float64 running sums of the recorded probabilities).  Every row takes part: the generator's seed keeps every sampled
    probability above the recorded floor (1e-3 = 10x the 1e-4 the HIP logits may differ by), so the midpoint is >= 5e-4 from both edges.
    Log-probabilities and hidden states within 2e-5 (the stage-2 validation loop's tolerance for this policy's logits is 1e-4)."""
    g = np.load(GOLDEN)
    b, t, c, hw, a, h = (int(v) for v in g["dims"])
    floor = float(g["floors"][0])
    pol = _load_synth(ActorCritic(c, c * hw * hw, a, h, True), int(g["seeds"][0])).to(DEV).train()
    states = _rnd((t, b, c, hw, hw), int(g["seeds"][1]), 0.5).to(DEV)
    mem = Memory()
    probs = g["rollout_probs"].astype(np.float64)
    cdf = np.cumsum(probs, -1)
    for s in range(t):
        rec = g["rollout_actions"][s]
        p_rec = probs[s, np.arange(b), rec]
        assert (p_rec >= floor).all()
        u = torch.from_numpy((cdf[s, np.arange(b), rec] - 0.5 * p_rec).astype(np.float32)).to(DEV)
        action = pol.act(states[s], mem, restart_batch=s == 0, training=True, uniforms=u)
        assert action.dtype == torch.int64 and action.shape == (b,)
        assert np.array_equal(action.cpu().numpy(), rec), s
        assert np.abs(mem.logprobs[-1].cpu().numpy() - g["rollout_logprobs"][s]).max() < 2e-5
        assert np.abs(mem.hidden[-1][0].cpu().numpy() - g["rollout_hidden"][s]).max() < 2e-5
    assert len(mem.states) == len(mem.actions) == len(mem.logprobs) == t and len(mem.hidden) == t + 1
    assert all(torch.equal(m, states[i]) for i, m in enumerate(mem.states))


def test_sampling_distribution_chi_square():
    """200 000 draws from one fixed 49-way distribution with torch.rand uniforms (fixed seed): Pearson's chi-square against the kernel's own
    probabilities below the 99.9 % quantile for 48 degrees of freedom (84.04)."""
    a, n = 49, 200000
    logits = _rnd((1, a), 5, 1.0).to(DEV).expand(n, a).contiguous()
    torch.manual_seed(1234)
    u = torch.rand(n, device=DEV)
    action, logprob, probs = hip_ops.ppo_sample(logits, u, want_probs=True)
    p = torch.softmax(logits[0].double().cpu(), 0)
    assert (probs[0].double().cpu() - p).abs().max() < 1e-6
    want = torch.log(p)[action.cpu()]
    assert (logprob.double().cpu() - want).abs().max() < 1e-5
    counts = torch.bincount(action.cpu(), minlength=a).double()
    chi2 = (((counts - n * p) ** 2) / (n * p)).sum().item()
    print("chi-square %.2f (48 dof)" % chi2)
    assert chi2 < 84.04
    # the edges: u = 0 takes the first index with a positive probability, u -> 1 the last
    edge = hip_ops.ppo_sample(logits[:2], torch.tensor([0.0, 0.99999994], device=DEV))[0]
    assert edge.tolist() == [0, a - 1]
    # act() without uniforms draws them from torch's device generator: reproducible from torch.manual_seed
    pol = _load_synth(ActorCritic(1280, 1280 * 49, 49, 1024, True), 7).to(DEV).train()
    st = _rnd((8, 1280, 7, 7), 9, 0.5).to(DEV)
    out = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        out.append(pol.act(st, Memory(), restart_batch=True, training=True))
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])


# ---- 2. G18 ------------------------------------------------------------------------------------------------------------------------------
def _memory_from_g18(g, tag):
    b, t, c, hw, a, h = (int(v) for v in g["dims"])
    mem = Memory()
    states = _rnd((t, b, c, hw, hw), int(g["seeds"][1]), 0.5).to(DEV)
    acts = g["rollout_actions"] if tag == "same" else g["clip_actions"]
    lps = g["rollout_logprobs"] if tag == "same" else g["clip_old_logprobs"]
    rew = _rnd((t, 1, b), int(g["seeds"][2]), 0.3).to(DEV)
    for s in range(t):
        mem.states.append(states[s])
        mem.actions.append(torch.from_numpy(acts[s]).to(DEV))
        mem.logprobs.append(torch.from_numpy(lps[s]).to(DEV))
        mem.rewards.append(rew[s])
    return mem, states


@pytest.mark.parametrize("tag", ["same", "clip"])
def test_update_matches_reference_g18(tag):
    """G18: the reference's PPO.update, every recorded quantity of the first epoch.  Tolerance: 50x the fp32-vs-fp64 spread of that
    quantity recorded in the golden, relative to its largest entry (the rule of test_train_mode_matches_reference_g17).  No element is
    exempt.  Checked twice: gradients through evaluate's autograd function with the loss written in torch ops, and through the fused
    loss head that PPO.update uses."""
    g = np.load(GOLDEN)
    b, t, c, hw, a, h = (int(v) for v in g["dims"])
    old_seed = int(g["seeds"][0]) if tag == "same" else int(g["clip_old_seed"][0])
    ppo = _ppo(seed=int(g["seeds"][0]), old_seed=old_seed, k_epochs=1).to(DEV)
    mem, states = _memory_from_g18(g, tag)
    pol = ppo.policy
    rewards = torch.cat([r.reshape(1, -1) for r in mem.rewards], 0)
    returns = hip_ops.ppo_returns(rewards, ppo.gamma)
    actions, old = torch.stack(mem.actions), torch.stack(mem.logprobs)
    # evaluate (autograd Function) + the loss written with torch ops: gradients through the HIP backward of evaluate
    logprobs, values, entropy = pol.evaluate(states, actions)
    ratios = torch.exp(logprobs - old)
    adv = returns - values.detach()
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 0.8, 1.2) * adv) + 0.5 * torch.nn.functional.mse_loss(values, returns)
            - 0.01 * entropy).mean()
    pol.zero_grad(set_to_none=True)
    loss.backward()
    via_autograd = {n: p.grad.detach().clone() for n, p in pol.named_parameters()}
    # the fused loss head: the same numbers from one kernel
    fwd = pol._train_forward(pol._states_nhwc(states))
    lp2, v2, e2, loss2, dhead = hip_ops.ppo_loss_head(fwd["head"], actions, old, returns, ppo.eps_clip)
    fused = pol._train_backward(fwd, dhead)
    assert torch.equal(lp2, logprobs) and torch.equal(v2, values) and torch.equal(e2, entropy)
    for grads, loss_v in ((via_autograd, loss), (fused, loss2)):
        got = {"returns": returns, "logprobs": logprobs, "values": values, "entropy": entropy, "loss": loss_v.reshape(1)}
        for n in FULL:
            got[n] = grads[n]
        for i, n in enumerate(PROJECTED):
            gm = grads[n].double().cpu()
            got[n + "@v"] = gm @ _rnd((gm.shape[1],), 174 + i).double()
            got["u@" + n] = _rnd((gm.shape[0],), 184 + i).double() @ gm
        for k, v in got.items():
            ref = g["%s_%s" % (tag, k)].astype(np.float64)
            tol = 50 * float(g["spread_%s_%s" % (tag, k)][0])
            err = np.abs(v.detach().double().cpu().numpy().reshape(ref.shape) - ref).max() / np.abs(ref).max()
            print("%-5s %-26s err %.2e tol %.2e" % (tag, k, err, tol))
            assert err < tol, (tag, k, err, tol)


# ---- 3. PPO.update against a float64 restatement -------------------------------------------------------------------------------------------
def _ref_update(ppo, states, actions, old_logprobs, rewards, k_epochs):
    """ACT/models/ppo.py:147-178 restated in float64 on the CPU with torch autograd over a copy of the policy's nn modules.
    Returns (first-epoch gradients, per-epoch losses, final parameters)."""
    pol = copy.deepcopy(ppo.policy).cpu().double()
    opt = torch.optim.Adam(pol.parameters(), lr=ppo.lr, betas=ppo.betas)
    t, b = actions.shape
    states, old, rewards = states.double(), old_logprobs.double(), rewards.double()
    disc, run = [], torch.zeros(b, dtype=torch.float64)
    for r in reversed(rewards):
        run = r + ppo.gamma * run
        disc.insert(0, run)
    ret = torch.stack(disc)
    ret = (ret - ret.mean()) / (ret.std() + 1e-5)
    first, losses = None, []
    for _ in range(k_epochs):
        e = pol.state_encoder(states.reshape(t * b, *states.shape[2:])).view(t, b, -1)
        out, _ = pol.gru(e, torch.zeros(1, b, e.shape[2], dtype=torch.float64))
        s = out.reshape(t * b, -1)
        logp = torch.log_softmax(pol.actor[0](s), -1)
        lp = logp.gather(1, actions.reshape(-1, 1)).view(t, b)
        ent = -(logp.exp() * logp).sum(-1).view(t, b)
        val = pol.critic(s).view(t, b)
        ratios = torch.exp(lp - old)
        adv = ret - val.detach()
        loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - ppo.eps_clip, 1 + ppo.eps_clip) * adv)
                + 0.5 * torch.nn.functional.mse_loss(val, ret) - 0.01 * ent).mean()
        opt.zero_grad()
        loss.backward()
        if first is None:
            first = {n: p.grad.clone() for n, p in pol.named_parameters()}
        losses.append(loss.item())
        opt.step()
    return first, losses, {n: p.detach().clone() for n, p in pol.named_parameters()}, ret


def _rel(a, b):
    return ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("b,t,a,k", [(64, 16, 49, 2), (64, 16, 64, 1), (3, 5, 25, 1), (3, 5, 36, 1), (3, 5, 49, 1), (3, 5, 64, 2)])
def test_update_matches_float64_autograd(b, t, a, k):
    """PPO.update against CPU float64 autograd of the restatement above: policy_old differs from policy (ratios on both sides of the clip
    range), real dimensions.  First-epoch gradients: relative l2 error < 1e-4 each (fp32 sums in another order than fp64; the bound of the
    stage-3 gradient test).  After the update: the parameters' total step within 5e-2 of the restatement's in l2 -- the first Adam step is
    lr * sign(g) wherever |g| >> 1e-8, so only elements whose gradient is within fp32 noise (about 1e-8) of zero may land elsewhere, a
    fraction of about 1e-5 of them, each off by at most 2 lr: sqrt(4e-5) = 6e-3 relative -- and the last epoch's loss within 1e-4."""
    c, hw, h = 1280, 7, 1024
    ppo = _ppo(a=a, seed=300 + a, old_seed=400 + a, k_epochs=k)
    before = {n: p.detach().clone() for n, p in ppo.policy.named_parameters()}
    states = _rnd((t, b, c, hw, hw), 50 + b, 0.5)
    rewards = _rnd((t, b), 60 + b, 0.3)
    gen = np.random.Generator(np.random.PCG64(70 + b + a))
    actions = torch.from_numpy(gen.integers(0, a, size=(t, b)))
    # old log-probabilities: policy_old's own on the same states, in float64
    old_pol = copy.deepcopy(ppo.policy_old).double()
    with torch.no_grad():
        e = old_pol.state_encoder(states.double().reshape(t * b, c, hw, hw)).view(t, b, -1)
        out, _ = old_pol.gru(e, torch.zeros(1, b, h, dtype=torch.float64))
        old = torch.log_softmax(old_pol.actor[0](out.reshape(t * b, -1)), -1).gather(1, actions.reshape(-1, 1)).view(t, b).float()
    first, losses, final, ret = _ref_update(ppo, states, actions, old, rewards, k)
    ppo = ppo.to(DEV)
    mem = Memory()
    for s in range(t):
        mem.states.append(states[s].to(DEV))
        mem.actions.append(actions[s].to(DEV))
        mem.logprobs.append(old[s].to(DEV))
        mem.rewards.append(rewards[s].view(1, b).to(DEV))
    assert _rel(hip_ops.ppo_returns(rewards.to(DEV), ppo.gamma), ret) < 1e-5
    # first-epoch gradients through the same calls update() makes
    pol = ppo.policy
    fwd = pol._train_forward(pol._states_nhwc(torch.stack(mem.states)))
    _, _, _, loss0, dhead = hip_ops.ppo_loss_head(fwd["head"], actions.to(DEV), old.to(DEV), hip_ops.ppo_returns(rewards.to(DEV), ppo.gamma),
                                                  ppo.eps_clip)
    grads = pol._train_backward(fwd, dhead)
    assert abs(loss0.item() - losses[0]) < 1e-5 * max(1.0, abs(losses[0]))
    for n in PARAM_NAMES:
        assert first[n].abs().max() > 1e-7, n
        err = _rel(grads[n].reshape(first[n].shape), first[n])
        print("%-24s rel %.2e" % (n, err))
        assert err < 1e-4, (n, err)
    ppo.update(mem)
    assert abs(ppo.last_loss.item() - losses[-1]) < 1e-4 * max(1.0, abs(losses[-1]))
    for n, p in ppo.policy.named_parameters():
        step_ref = final[n] - before[n].double()
        step_got = p.detach().double().cpu() - before[n].double()
        assert step_ref.abs().max() > 0
        err = ((step_got - step_ref).norm() / step_ref.norm()).item()
        assert err < 5e-2, (n, err)


# ---- 4. the split-K weight gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,cin", [(64 * 16 * 49, 1280), (3 * 5 * 49, 1280), (1001, 384), (7, 128)])
def test_split_k_weight_gradient(npix, cin):
    """dW_enc by the split-K streaming kernel against the single-chain strided GEMM on the same inputs, and twice: torch.equal.
    The two sum the same products in different orders; the tolerance is measured in the test: 8x the distance of the single-chain fp32
    result from the float64 one (relative to the largest entry), i.e. the fp32 summation-order spread of this very product."""
    s = _rnd((npix, cin), 11, 0.5).to(DEV)
    de1 = _rnd((npix, 32), 12, 1e-3).to(DEV)
    e1 = torch.relu(_rnd((npix, 32), 13)).to(DEV)
    a = hip_ops.ppo_wenc_grad(s, de1, e1, split_k=True)
    b = hip_ops.ppo_wenc_grad(s, de1, e1, split_k=True)
    chain = hip_ops.ppo_wenc_grad(s, de1, e1, split_k=False)
    assert torch.equal(a, b)
    ref = (torch.where(e1 > 0, de1, torch.zeros_like(de1)).double().cpu().t() @ s.double().cpu())
    scale = ref.abs().max().item()
    spread = (chain.double().cpu() - ref).abs().max().item() / scale
    err_chain = (a - chain).abs().max().item() / scale
    err_ref = (a.double().cpu() - ref).abs().max().item() / scale
    print("npix %d cin %d: split-K vs chain %.2e, vs float64 %.2e, chain vs float64 %.2e" % (npix, cin, err_chain, err_ref, spread))
    assert scale > 0 and spread > 0
    assert err_chain < 8 * spread and err_ref < 8 * spread


# ---- 5. after the update ---------------------------------------------------------------------------------------------------------------------
def _act_args(**over):
    a = dict(num_segments=4, num_classes=200, reward="random", dataset="actnet", input_size=224, batch_size=2, patch_size=96,
             with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024, policy_conv=True,
             gpu=0, continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.0, consensus="gru", hidden_dim=1024,
             train_stage=2)
    a.update(over)
    return types.SimpleNamespace(**a)


def _model(**over):
    args = _act_args(**over)
    model = GFV(args)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(manifest()["ACT"], 1007).items()}
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval(), args


def test_update_moves_the_policy_and_the_next_act_sees_it():
    model, args = _model()
    model.policy_train_mode()
    ppo, mem = model.focuser.policy, model.focuser.memory
    b, t = 4, 3
    states = _rnd((t, b, 1280, 7, 7), 21, 0.5).to(DEV)
    u = torch.rand(t, b, generator=torch.Generator().manual_seed(1)).to(DEV)
    before = {n: p.detach().clone() for n, p in ppo.policy.named_parameters()}
    probe = Memory()
    a_before = ppo.policy_old.act(states[0], probe, restart_batch=True, training=True, uniforms=u[0])
    lp_before = probe.logprobs[0].clone()
    for s in range(t):
        ppo.policy_old.act(states[s], mem, restart_batch=s == 0, training=True, uniforms=u[s])
        mem.rewards.append(_rnd((1, b), 30 + s, 0.3).to(DEV))
    model.focuser.update()
    assert all(len(x) == 0 for x in (mem.actions, mem.states, mem.logprobs, mem.rewards, mem.is_terminals, mem.hidden))
    assert ppo.last_loss.shape == (1,) and torch.isfinite(ppo.last_loss).all()
    for (n, p), (n2, q) in zip(ppo.policy.named_parameters(), ppo.policy_old.named_parameters()):
        assert n == n2 and torch.equal(p, q), n
        assert not torch.equal(p, before[n]), n
        assert torch.isfinite(p).all(), n
    # the engine-layout weight views key on the parameter versions: the next step runs on the new weights
    probe = Memory()
    ppo.policy_old.act(states[0], probe, restart_batch=True, training=True, uniforms=u[0])
    assert not torch.equal(probe.logprobs[0], lp_before)
    ref = copy.deepcopy(ppo.policy_old).cpu().double()
    with torch.no_grad():
        e = ref.state_encoder(states[0].double().cpu())
        out, _ = ref.gru(e.view(1, b, -1), torch.zeros(1, b, 1024, dtype=torch.float64))
        logp = torch.log_softmax(ref.actor[0](out[0]), -1).gather(1, probe.actions[0].cpu().view(-1, 1)).view(-1)
    assert (probe.logprobs[0].double().cpu() - logp).abs().max() < 2e-5
    assert a_before.shape == (b,)


# ---- 6. the loop body end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward", ["random", "prev"])
def test_train_stage2_batch_end_to_end(reward):
    b, t = 2, 4
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=3)).to(DEV)
    target = torch.tensor([3, 150], device=DEV)
    runs = []
    for _ in range(2):
        model, args = _model(reward=reward)
        model.policy_train_mode()
        # observe the rewards the loop stores (the memory is cleared by the update)
        seen = []
        inner = model.focuser.update

        def spy(inner=inner, model=model, seen=seen):
            seen.extend(r.clone() for r in model.focuser.memory.rewards)
            seen.append(torch.stack(model.focuser.memory.actions).clone())
            return inner()
        model.focuser.update = spy
        # ... and every step's logits and baseline logits; for 'prev' / 'conf' / 'padding' the baseline feature is [glancer vector | zeros],
        # so the baseline is also recomputed here from the classifier's state BEFORE the step (it must not see the step's own update)
        steps = []
        step_inner = model.one_step_act

        def step_spy(img, fmap, fvec, restart_batch=False, training=True, step_inner=step_inner, model=model, steps=steps):
            hx = None if restart_batch else model.classifier.hx
            out = step_inner(img, fmap, fvec, restart_batch=restart_batch, training=training)
            want_base = None
            if model.rew != "random":
                feat = torch.cat([fvec, torch.zeros(fvec.shape[0], model.focuser.feature_dim, device=fvec.device)], 1)
                want_base = model.classifier._steps_from(feat.unsqueeze(1), hx)[0]
            steps.append((out[0].clone(), out[3].clone(), want_base))
            return out
        model.one_step_act = step_spy
        torch.manual_seed(11)
        np.random.seed(12)
        preds, loss = train.train_stage2_batch(model, images, target, args)
        assert preds.shape == (t, b, 200) and torch.isfinite(loss) and torch.isfinite(model.focuser.policy.last_loss).all()
        del model.one_step_act, model.focuser.update
        runs.append((preds, loss, seen, {n: p.detach().clone() for n, p in model.focuser.policy.policy.named_parameters()}, model, args, steps))
    (p0, l0, s0, w0, model, args, steps), (p1, l1, s1, w1, _, _, _) = runs
    assert torch.equal(p0, p1) and torch.equal(l0, l1)
    assert all(torch.equal(x, y) for x, y in zip(s0, s1)) and all(torch.equal(w0[n], w1[n]) for n in w0)
    # the stored rewards equal get_reward of the step's logits and baseline logits, for both kinds: 'random' is the confidence minus the
    # baseline's (a random crop's logits from the same classifier state), 'prev' the confidence's change from the previous step
    assert len(steps) == t
    conf_last = 0
    for s, (output, baseline, want_base) in enumerate(steps):
        assert torch.equal(output, p0[s])
        conf = torch.softmax(output, 1).gather(1, target.view(-1, 1)).view(1, -1)
        bconf = torch.softmax(baseline, 1).gather(1, target.view(-1, 1)).view(1, -1)
        want, conf_last = train.get_reward(args, conf, conf_last, bconf)
        assert s0[s].shape == (1, b) and torch.equal(s0[s], want), s
        if reward == "random":
            assert torch.equal(want, conf - bconf) and not torch.equal(baseline, output), s
        else:
            assert torch.equal(baseline, want_base), s
            assert torch.equal(want, conf - (0 if s == 0 else torch.softmax(p0[s - 1], 1).gather(1, target.view(-1, 1)).view(1, -1))), s
    assert s0[t].shape == (t, b)
    # the trained model validates through the stage-2 evaluation loop
    model.eval()
    args.train_stage = 2
    dataset = [(images[i].cpu(), torch.tensor([int(target[i])])) for i in range(b)]
    top1, top5, mean_ap, logs = evaluate.validate(dataset, model, torch.nn.CrossEntropyLoss(), args, quiet=True)
    assert 0 <= top1 <= 100 and 0 <= top5 <= 100 and len(logs) > 0


# ---- 7. the mode guard -------------------------------------------------------------------------------------------------------------------------
def test_one_step_act_training_needs_policy_train_mode():
    model, args = _model()
    b, t = 2, 4
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=5)).to(DEV)
    fmap, fvec = model.glance(images)
    img = images.view(b, t, 3, 224, 224)[:, 0]
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        model.one_step_act(img, fmap[:, 0], fvec[:, 0], restart_batch=True, training=True)
    model.policy_train_mode()
    out = model.one_step_act(img, fmap[:, 0], fvec[:, 0], restart_batch=True, training=True)
    assert len(out) == 4
    logits, last, sizes, baseline = out
    assert logits.shape == (b, 200) and last.shape == (b, 200) and sizes is None and baseline.shape == (b, 200)
    mem = model.focuser.memory
    assert len(mem.actions) == len(mem.logprobs) == len(mem.states) == 1 and mem.actions[0].shape == (b,)
    mem.clear_memory()


# ---- 8. one training core for both policies -------------------------------------------------------------------------------------------------
def test_evaluate_backward_equals_train_backward():
    """evaluate runs through the one autograd class both policies share (policy_train.PolicyEvaluateFn), and loss.backward() through it
    gives the gradients of _train_backward for the same d loss / d head: torch.equal for every parameter (B = 3, T = 5, A = 25; upstream
    gradients of all three outputs)."""
    from adafocus_amd import policy_train, ppo, ppo_continuous
    assert ppo.PolicyEvaluateFn is policy_train.PolicyEvaluateFn and ppo_continuous.PolicyEvaluateFn is policy_train.PolicyEvaluateFn
    b, t, a = 3, 5, 25
    pol = _ppo(a=a, seed=300 + a).policy.to(DEV)
    states = _rnd((t, b, 1280, 7, 7), 53, 0.5).to(DEV)
    actions = torch.from_numpy(np.random.Generator(np.random.PCG64(95)).integers(0, a, size=(t, b))).to(DEV)
    g = [_rnd((t, b), 90 + i).to(DEV) for i in range(3)]
    logprobs, values, entropy = pol.evaluate(states, actions)
    assert type(logprobs.grad_fn) is policy_train.PolicyEvaluateFn._backward_cls
    pol.zero_grad(set_to_none=True)
    ((logprobs * g[0]).sum() + (values * g[1]).sum() + (entropy * g[2]).sum()).backward()
    with torch.no_grad():
        fwd = pol._train_forward(pol._states_nhwc(states))
        want = pol._train_backward(fwd, hip_ops.ppo_head_backward(fwd["head"], actions, *g))
    assert tuple(n for n, _ in pol.named_parameters()) == PARAM_NAMES and set(want) == set(PARAM_NAMES)
    for n, p in pol.named_parameters():
        assert p.grad.abs().max() > 0 and torch.equal(p.grad, want[n].reshape(p.shape)), n
    # sum() hands the backward expanded (stride-0) upstream gradients: the head wrapper lays them out itself
    logprobs, values, entropy = pol.evaluate(states, actions)
    pol.zero_grad(set_to_none=True)
    (logprobs.sum() + 0.5 * values.sum()).backward()
    with torch.no_grad():
        dense = [torch.full((t, b), v, device=DEV) for v in (1.0, 0.5, 0.0)]
        want = pol._train_backward(fwd, hip_ops.ppo_head_backward(fwd["head"], actions, *dense))
        assert torch.equal(hip_ops.ppo_head_backward(fwd["head"], actions, dense[0].t().contiguous().t(), dense[1][:1].expand(t, b), None),
                           hip_ops.ppo_head_backward(fwd["head"], actions, dense[0], dense[1], None))
    for n, p in pol.named_parameters():
        assert torch.equal(p.grad, want[n].reshape(p.shape)), n


def test_encoder_backward_wrapper_equals_the_32_output_export():
    """hip_ops.ppo_encoder_backward (the general entry point, bn=None) at the discrete policy's 32 conv outputs against a direct call of
    adaf_ppo_encoder_backward_f32 on the same operands: torch.equal (T = 5, B = 3, 7 x 7 map, C = 128, H = 1024)."""
    import ctypes as C
    from adafocus_amd import _lib as L
    t, b, hw, cin, cmid, hid = 5, 3, 49, 128, 32, 1024
    states = _rnd((t * b, 7, 7, cin), 1010, 0.5).to(DEV)
    e1 = _rnd((t * b, hw * cmid), 1012).clamp(min=0).to(DEV)
    e_bt, dx = _rnd((b, t, hid), 1013).clamp(min=0).to(DEV), _rnd((b, t, hid), 1014, 0.1).to(DEV)
    w_lin = _rnd((hid, hw * cmid), 1015, 0.02).to(DEV)
    got = hip_ops.ppo_encoder_backward(states, e1, e_bt, dx, t, b, w_lin, bn=None)
    lib, h = L.load_library(), L.handle(DEV)
    need = lib.adaf_ppo_encoder_backward_workspace_bytes(t, b, hw, cin, cmid, hid)
    assert need == lib.adaf_ppo_encoder_bn_backward_workspace_bytes(t, b, hw, cin, cmid, hid, 0) and need > 0
    ws = torch.empty(need // 4, device=DEV)
    want = [torch.empty(s, device=DEV) for s in ((cmid, cin), (hid, cmid * hw), (hid,))]
    L.check(lib.adaf_ppo_encoder_backward_f32(h, L.ptr(states), L.ptr(e1), L.ptr(e_bt), L.ptr(dx), t, b, hw, cin, cmid, hid, L.ptr(w_lin),
                                              *(L.ptr(w) for w in want), L.ptr(ws), C.c_size_t(need), L.stream_ptr()), h)
    assert len(got) == 3
    for x, y in zip(got, want):
        assert x.shape == y.shape and y.abs().max() > 0 and torch.equal(x, y)
