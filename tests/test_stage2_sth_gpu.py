"""Stage-2 training of the Something-Something tree on the MI355X (csrc/ppo_train.hip): the Gaussian sampling kernel, BatchNorm
with batch statistics forward and backward, the 64-output split-K weight gradient, the roll-out and the PPO update against the reference
(G19) and against CPU autograd of a float64 restatement, and `train_stage2_batch_sth` end to end."""
import copy
import os

import numpy as np
import pytest
import torch

from adafocus_amd import hip_ops, synth, train
from adafocus_amd.ppo_continuous import PPO_Continuous, Memory
from tests import gauss_policy_model as M
from tests.helpers import synth_sd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g19_sth_stage2.npz")
DEV = torch.device("cuda:0")
FLOOR = 2.0 ** -22


def _rnd(shape, seed, scale=1.0):
    g = np.random.Generator(np.random.PCG64([seed, 0xBEEF]))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def _load_synth(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed).items()})
    return module


def _ppo(feature_dim, hw, h, with_bn, sigma, seed, old_seed=None, k_epochs=1, lr=0.0003):
    ppo = PPO_Continuous(feature_dim, feature_dim * hw * hw, h, True, lr=lr, gamma=0.7, K_epochs=k_epochs, eps_clip=0.2, action_std=sigma,
                         with_bn=with_bn)
    _load_synth(ppo.policy, seed)
    _load_synth(ppo.policy_old, seed if old_seed is None else old_seed)
    ppo.policy.train()
    ppo.policy_old.train()
    return ppo


# ---- 1. the sampling kernel ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampling_reference():
    """65 rows, sigma = 0.25: means in (0, 1), normals; the CPU expression's actions and the float64 log-probabilities.  The tolerance is
    the rule of ppo_rewards_kernel's test: 8x the largest distance of torch's own fp32 MultivariateNormal.log_prob from float64 over these
    rows, floor 2^-22.  Computed once; the cases take the first B rows."""
    sigma = 0.25
    g = torch.Generator().manual_seed(21)
    mean = torch.rand(65, 2, generator=g)
    noise = torch.randn(65, 2, generator=g)
    noise[0] = torch.tensor([-4.0, 4.0])                # row 0 (the B = 1 case) clamps at both ends
    action, _ = M.sample_action(mean, noise, sigma)
    assert (action == 0).any() and (action == 1).any() and ((action > 0) & (action < 1)).any()
    lp64 = M.logprob(action.double(), mean.double(), sigma)
    lp32 = torch.distributions.MultivariateNormal(mean, scale_tril=torch.diag(torch.full((2,), sigma))).log_prob(action)
    tol = max(8 * (lp32.double() - lp64).abs().max().item(), FLOOR)
    return sigma, mean, noise, action, lp64, tol


@pytest.mark.parametrize("b", [1, 3, 64, 65])
def test_gauss_sample_kernel(sampling_reference, b):
    sigma, mean, noise, action, lp64, tol = sampling_reference
    got_a, got_lp = hip_ops.ppo_gauss_sample(mean[:b].to(DEV), noise[:b].to(DEV), sigma)
    assert got_a.shape == (b, 2) and got_lp.shape == (b,)
    assert torch.equal(got_a.cpu(), action[:b])
    err = (got_lp.double().cpu() - lp64[:b]).abs().max().item()
    print("B %d: log-probability error %.2e, tolerance %.2e" % (b, err, tol))
    assert err <= tol


# ---- 2. BatchNorm with batch statistics, forward and backward ---------------------------------------------------------------------------------
def _bn_reference(x, gamma, beta, rmean, rvar, dy, dtype):
    x = x.to(dtype).requires_grad_()
    gamma, beta = gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    rmean, rvar = rmean.to(dtype).clone(), rvar.to(dtype).clone()
    y = torch.relu(torch.nn.functional.batch_norm(x, rmean, rvar, gamma, beta, training=True, momentum=0.1, eps=1e-5))
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rmean, running_var=rvar)


@pytest.mark.parametrize("rows,cols", [(2, 64), (3, 1024), (45, 64), (196, 64), (130, 1024), (6272, 64)])
def test_bn_train_forward_backward(rows, cols):
    """Outputs, dx, dgamma, dbeta and the running statistics against float64, each within 8x the distance of torch-CPU fp32 batch_norm +
    autograd from float64 on the same inputs (measured here), relative to the quantity's largest entry.  Two runs: equal bits."""
    x = _rnd((rows, cols), 31) * (1 + _rnd((cols,), 32).abs()) + _rnd((cols,), 33)
    gamma, beta = 1 + 0.1 * _rnd((cols,), 34), 0.1 * _rnd((cols,), 35)
    rmean, rvar = 0.1 * _rnd((cols,), 36), 1 + 0.1 * _rnd((cols,), 37).abs()
    dy = _rnd((rows, cols), 38)
    r64 = _bn_reference(x, gamma, beta, rmean, rvar, dy, torch.float64)
    r32 = _bn_reference(x, gamma, beta, rmean, rvar, dy, torch.float32)
    runs = []
    for _ in range(2):
        rm, rv = rmean.to(DEV), rvar.to(DEV)
        y, mean, invstd = hip_ops.bn_train_forward(x.to(DEV), gamma.to(DEV), beta.to(DEV), rm, rv)
        dx, dgamma, dbeta = hip_ops.bn_train_backward(x.to(DEV), y, dy.to(DEV), gamma.to(DEV), mean, invstd)
        runs.append(dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, running_mean=rm, running_var=rv))
    assert (r64["y"] == 0).any() and (r64["y"] > 0).any()
    for k, ref in r64.items():
        assert torch.equal(runs[0][k], runs[1][k]), k
        scale = ref.abs().max().item()
        tol = 8 * (r32[k].double() - ref).abs().max().item() / scale
        err = (runs[0][k].double().cpu() - ref).abs().max().item() / scale
        print("%5d x %4d %-12s err %.2e tol %.2e" % (rows, cols, k, err, tol))
        assert scale > 0
        assert err <= tol, (k, err, tol)       # (two rows: torch's sum of two values is exact, and so must this one be)


def test_bn_train_one_row_is_refused():
    one = torch.zeros(1, 64, device=DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hip_ops.bn_train_forward(one, torch.ones(64, device=DEV), torch.zeros(64, device=DEV))


# ---- 3. the 64-output split-K weight gradient --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("npix,cin", [(18, 128), (147, 384), (196, 2560), (3136, 1280)])
def test_split_k_weight_gradient_64_outputs(npix, cin, masked):
    """dW_enc [64, C] by the split-K streaming kernel against the single-chain strided GEMM on the same inputs, and twice: torch.equal.
    With the ReLU mask of the conv output (e1) and with a gradient whose mask is applied already (e1 = None).  Tolerance as for 32
    outputs: 8x the distance of the single-chain fp32 result from the float64 one, relative to the largest entry."""
    s = _rnd((npix, cin), 11, 0.5).to(DEV)
    de1 = _rnd((npix, 64), 12, 1e-3).to(DEV)
    e1 = torch.relu(_rnd((npix, 64), 13)).to(DEV) if masked else None
    a = hip_ops.ppo_wenc_grad(s, de1, e1, split_k=True)
    b = hip_ops.ppo_wenc_grad(s, de1, e1, split_k=True)
    chain = hip_ops.ppo_wenc_grad(s, de1, e1, split_k=False)
    assert a.shape == (64, cin) and torch.equal(a, b)
    g = torch.where(e1 > 0, de1, torch.zeros_like(de1)) if masked else de1
    ref = g.double().cpu().t() @ s.double().cpu()
    scale = ref.abs().max().item()
    spread = (chain.double().cpu() - ref).abs().max().item() / scale
    err_chain = (a - chain).abs().max().item() / scale
    err_ref = (a.double().cpu() - ref).abs().max().item() / scale
    print("npix %d cin %d masked %d: split-K vs chain %.2e, vs float64 %.2e, chain vs float64 %.2e" % (npix, cin, masked, err_chain, err_ref, spread))
    assert scale > 0 and spread > 0
    assert err_chain < 8 * spread and err_ref < 8 * spread


# ---- 4. G19: the reference's roll-out and update -------------------------------------------------------------------------------------------------
CASES = ("bn_vd1", "bn_vd2", "nobn_vd2", "clip")


def _case(g, tag):
    with_bn, t, tg, b, k, seed_old, seed_t = (int(v) for v in g["%s_case" % tag])
    c, hw, h = (int(v) for v in g["dims"])
    seed_w, seed_s, seed_r = (int(v) for v in g["seeds"])
    sigma = float(g["%s_action_std" % tag][0])
    states = [_rnd((b, tg * c, hw, hw), seed_s + s, 0.5).to(DEV) for s in range(t)]
    rewards = _rnd((t, 1, b), seed_r, 0.3).to(DEV)
    ppo = _ppo(tg * c, hw, h, bool(with_bn), sigma, seed_w, seed_old, k, float(g["lr"][0]))
    ppo.to(DEV)
    return ppo, states, rewards, (bool(with_bn), t, tg, b, k, sigma)


@pytest.mark.parametrize("tag", CASES)
def test_rollout_matches_reference_g19(tag):
    """Every recorded step of the reference's policy_old.act(training=True) with noise = (recorded sample - recorded mean) / sigma: the
    actions take the reference's clamp decisions (every raw sample is >= 1e-3 from 0 and 1 by the generator's search), interior actions,
    log-probabilities and hidden states within 2e-5, policy_old's BatchNorm buffers after every step within 2e-5 of their largest entry,
    num_batches_tracked exactly."""
    g = np.load(GOLDEN)
    ppo, states, _, (with_bn, t, tg, b, k, sigma) = _case(g, tag)
    pol, mem = ppo.policy_old, Memory()
    for s in range(t):
        mean_ref, raw_ref, act_ref = (g["%s_rollout_%s" % (tag, q)][s] for q in ("mean", "sample", "action"))
        noise = torch.from_numpy(((raw_ref.astype(np.float64) - mean_ref) / sigma).astype(np.float32)).to(DEV)
        action = pol.act(states[s], mem, restart_batch=s == 0, training=True, noise=noise)
        a = action.cpu().numpy()
        assert a.shape == (b, 2) and np.array_equal(a == 0, act_ref == 0) and np.array_equal(a == 1, act_ref == 1)
        errs = dict(action=np.abs(a - act_ref).max(), logprob=np.abs(mem.logprobs[-1].cpu().numpy() - g["%s_rollout_logprob" % tag][s]).max(),
                    hidden=np.abs(mem.hidden[-1][0].cpu().numpy() - g["%s_rollout_hidden" % tag][s]).max())
        print("%-8s step %d: %s" % (tag, s, "  ".join("%s %.2e" % kv for kv in errs.items())))
        assert max(errs.values()) < 2e-5, errs
        for key, v in pol.state_dict().items():
            if "running_" in key:
                ref = g["%s_rollout_old_%s" % (tag, key)][s]
                assert np.abs(v.cpu().numpy() - ref).max() < 2e-5 * np.abs(ref).max(), key
            elif "num_batches" in key:
                assert int(v) == int(g["%s_rollout_old_%s" % (tag, key)][s]) == s + 1
    assert len(mem.states) == len(mem.actions) == len(mem.logprobs) == t and len(mem.hidden) == t + 1
    assert all(torch.equal(m, states[i]) for i, m in enumerate(mem.states))


def _memory_from_g19(g, tag, states, rewards):
    mem = Memory()
    for s, st in enumerate(states):
        mem.states.append(st)
        mem.actions.append(torch.from_numpy(g["%s_rollout_action" % tag][s]).to(DEV))
        mem.logprobs.append(torch.from_numpy(g["%s_rollout_logprob" % tag][s]).to(DEV))
        mem.rewards.append(rewards[s])
    return mem


def _projections(grads, with_bn):
    lin = "state_encoder.%d.weight" % (4 if with_bn else 3)
    projected = sorted(("state_encoder.0.weight", "gru.weight_ih_l0", "gru.weight_hh_l0", lin))
    out = {}
    for i, n in enumerate(projected):
        gm = grads[n].double().cpu().flatten(1)
        out[n + "@v"] = gm @ _rnd((gm.shape[1],), 174 + i).double()
        out["u@" + n] = _rnd((gm.shape[0],), 184 + i).double() @ gm
    out.update({n: v for n, v in grads.items() if n not in projected})
    return out


def _check_against_g19(g, tag, got, with_bn):
    for key, v in got.items():
        ref = g["%s_%s" % (tag, key)].astype(np.float64)
        v = v.detach().double().cpu().numpy().reshape(ref.shape)
        if with_bn and key == "state_encoder.4.bias":
            # zero in real arithmetic (BatchNorm removes the bias): no entry above 50x the largest magnitude of the reference's fp32 run
            print("%-8s %-40s max %.2e, reference fp32 max %.2e" % (tag, key, np.abs(v).max(), np.abs(ref).max()))
            assert np.abs(v).max() <= 50 * np.abs(ref).max(), (tag, key)
            continue
        if not ref.any():
            assert not v.any(), (tag, key)
            continue
        tol = 50 * float(g["spread_%s_%s" % (tag, key)][0])
        err = np.abs(v - ref).max() / np.abs(ref).max()
        print("%-8s %-40s err %.2e tol %.2e" % (tag, key, err, tol))
        assert err < tol, (tag, key, err, tol)


@pytest.mark.parametrize("tag", CASES)
def test_update_matches_reference_g19(tag):
    """G19: the reference's PPO_Continuous.update, every recorded quantity of the first epoch within 50x its recorded fp32-vs-fp64 spread,
    relative to its largest entry (G17 / G18's rule); no element is exempt.  Checked twice: gradients through evaluate's autograd function
    with the loss written in torch ops, and through the fused Gaussian head.  Then the update itself: the policy's BatchNorm buffers
    afterwards by the same rule, num_batches_tracked exactly, policy_old equal to policy.  Under BatchNorm the gradient of the Linear bias
    in front of BatchNorm1d is zero in real arithmetic: it is held to an absolute bound (50x the largest magnitude of the reference's fp32
    run) and, Adam turning rounding noise into full steps, the parameter's change to lr per epoch."""
    g = np.load(GOLDEN)
    ppo, states, rewards, (with_bn, t, tg, b, k, sigma) = _case(g, tag)
    mem = _memory_from_g19(g, tag, states, rewards)
    fresh = copy.deepcopy(ppo.policy.state_dict())
    pol = ppo.policy
    returns = hip_ops.ppo_returns(torch.cat([r.reshape(1, -1) for r in mem.rewards], 0), ppo.gamma)
    actions, old = torch.stack(mem.actions), torch.stack(mem.logprobs)
    stacked = torch.stack(mem.states)
    logprobs, values, entropy = pol.evaluate(stacked, actions)
    ratios = torch.exp(logprobs - old)
    adv = returns - values.detach()
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 0.8, 1.2) * adv) + 0.5 * torch.nn.functional.mse_loss(values, returns)
            - 0.01 * entropy).mean()
    pol.zero_grad(set_to_none=True)
    loss.backward()
    via_autograd = {n: p.grad.detach().clone() for n, p in pol.named_parameters()}
    with torch.no_grad():
        fwd = pol._train_forward(pol._states_dense(stacked))
        lp2, v2, e2, loss2, dhead = hip_ops.ppo_gauss_loss_head(fwd["head"], actions, sigma, old, returns, ppo.eps_clip)
        fused = pol._train_backward(fwd, dhead)
    assert torch.equal(lp2, logprobs) and torch.equal(v2, values) and torch.equal(e2, entropy)
    assert set(fused) == set(via_autograd) == {n for n, _ in pol.named_parameters()}
    for grads, loss_v in ((via_autograd, loss), (fused, loss2)):
        got = {"returns": returns, "logprobs": logprobs, "values": values, "entropy": entropy, "loss": loss_v.reshape(1)}
        got.update(_projections(grads, with_bn))
        _check_against_g19(g, tag, got, with_bn)
    # the update itself, from the recorded starting point (the forwards above moved the BatchNorm buffers)
    pol.load_state_dict(fresh)
    pol.zero_grad(set_to_none=True)
    ppo.update(mem)
    after = pol.state_dict()
    _check_against_g19(g, tag, {"new_" + n: v for n, v in after.items() if "running_" in n}, with_bn)
    for n, v in after.items():
        if "num_batches" in n:
            assert int(v) == int(g["%s_new_%s" % (tag, n)]) == k
    for (n, p), (_, q) in zip(after.items(), ppo.policy_old.state_dict().items()):
        assert torch.equal(p, q), n
    if with_bn:
        moved = (after["state_encoder.4.bias"] - fresh["state_encoder.4.bias"]).abs().max().item()
        assert moved <= k * ppo.lr * (1 + 1e-6), moved


# ---- 5. the whole update against a float64 restatement -----------------------------------------------------------------------------------------
def _ref_update(ppo, states, actions, old_logprobs, rewards, k_epochs, dtype):
    """STH/models/ppo_continuous.py:111-139,165-196 restated on the CPU in `dtype` with torch autograd over a copy of the policy's nn
    modules.  Returns (first-epoch gradients, per-epoch losses, final state dict, returns)."""
    pol = copy.deepcopy(ppo.policy).cpu().to(dtype).train()
    opt = torch.optim.Adam(pol.parameters(), lr=ppo.lr, betas=ppo.betas)
    t, b = actions.shape[:2]
    sigma = pol.action_std
    states, actions, old, rewards = states.to(dtype), actions.to(dtype), old_logprobs.to(dtype), rewards.to(dtype)
    disc, run = [], torch.zeros(b, dtype=dtype)
    for r in reversed(rewards):
        run = r + ppo.gamma * run
        disc.insert(0, run)
    ret = torch.stack(disc)
    ret = (ret - ret.mean()) / (ret.std() + 1e-5)
    first, losses = None, []
    for _ in range(k_epochs):
        e = pol.state_encoder(states.reshape(t * b, *states.shape[2:])).view(t, b, -1)
        out, _ = pol.gru(e, torch.zeros(1, b, e.shape[2], dtype=dtype))
        s = out.reshape(t * b, -1)
        dist = torch.distributions.MultivariateNormal(pol.actor(s), scale_tril=torch.diag(torch.full((2,), sigma, dtype=dtype)))
        lp = dist.log_prob(actions.reshape(t * b, 2)).view(t, b)
        ent = dist.entropy().view(t, b)
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
    return first, losses, {n: p.detach().clone() for n, p in pol.state_dict().items()}, ret


def _rel(a, b):
    return ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("c,tg,hw,h,b,t,k,with_bn", [(128, 3, 3, 64, 5, 1, 2, True), (128, 3, 3, 64, 5, 3, 2, True), (128, 3, 3, 64, 5, 1, 2, False),
                                                     (128, 3, 3, 64, 5, 3, 2, False), (1280, 8, 7, 1024, 64, 1, 1, True)])
def test_update_matches_float64_autograd(c, tg, hw, h, b, t, k, with_bn):
    """PPO_Continuous.update against CPU float64 autograd of the restatement above: policy_old differs from policy (ratios on both sides
    of the clip range), actions clamped at both ends and interior.  The bounds are the discrete policy's
    (tests/test_stage2_gpu.py::test_update_matches_float64_autograd, where they are derived): first-epoch gradients within 1e-4 in
    relative l2, the parameters' total step within 5e-2 of the restatement's in l2, the last epoch's loss within 1e-4; BatchNorm's running
    statistics after the update within 1e-4 in relative l2.  A gradient that is identically zero in the restatement (weight_hh after one
    step from the zero state) must be identically zero here, and so must its step.  Under BatchNorm the Linear bias in front of
    BatchNorm1d has a zero gradient in real arithmetic: no entry above 50x the largest magnitude the same restatement in fp32 produces
    for it, and the parameter moves by at most lr per epoch."""
    sigma, feat = 0.25, c * tg
    ppo = _ppo(feat, hw, h, with_bn, sigma, 500 + t, 600 + t, k)
    before = copy.deepcopy(ppo.policy.state_dict())
    states = _rnd((t, b, feat, hw, hw), 50 + b, 0.5)
    rewards = _rnd((t, b), 60 + b, 0.3)
    # the roll-out's actions and old log-probabilities: policy_old's own on the same states, in float64, with seeded normals
    old_pol = copy.deepcopy(ppo.policy_old).double().train()
    with torch.no_grad():
        e = old_pol.state_encoder(states.double().reshape(t * b, feat, hw, hw)).view(t, b, -1)
        out, _ = old_pol.gru(e, torch.zeros(1, b, h, dtype=torch.float64))
        mu = old_pol.actor(out.reshape(t * b, -1))
        noise = _rnd((t * b, 2), 70 + b).double()
        noise[0] = torch.tensor([-8.0, 8.0])
        actions, _ = M.sample_action(mu, noise, sigma)
        old = M.logprob(actions, mu, sigma).view(t, b).float()
        actions = actions.float().view(t, b, 2)
    assert (actions == 0).any() and (actions == 1).any() and ((actions > 0) & (actions < 1)).any()
    first, losses, final, ret = _ref_update(ppo, states, actions, old, rewards, k, torch.float64)
    inert = "state_encoder.4.bias" if with_bn else None
    noise32 = _ref_update(ppo, states, actions, old, rewards, 1, torch.float32)[0][inert].abs().max().item() if inert else None
    ppo.to(DEV)
    mem = Memory()
    for s in range(t):
        mem.states.append(states[s].to(DEV))
        mem.actions.append(actions[s].to(DEV))
        mem.logprobs.append(old[s].to(DEV))
        mem.rewards.append(rewards[s].view(1, b).to(DEV))
    returns = hip_ops.ppo_returns(rewards.to(DEV), ppo.gamma)
    assert _rel(returns, ret) < 1e-5
    pol = ppo.policy
    with torch.no_grad():
        fwd = pol._train_forward(pol._states_dense(torch.stack(mem.states)))
        _, _, _, loss0, dhead = hip_ops.ppo_gauss_loss_head(fwd["head"], actions.to(DEV), sigma, old.to(DEV), returns, ppo.eps_clip)
        grads = pol._train_backward(fwd, dhead)
    assert abs(loss0.item() - losses[0]) < 1e-5 * max(1.0, abs(losses[0]))
    for n, ref in first.items():
        got = grads[n].reshape(ref.shape)
        if n == inert:
            print("%-24s max %.2e, fp32 restatement max %.2e" % (n, got.abs().max().item(), noise32))
            assert got.abs().max().item() <= 50 * noise32
        elif not ref.any():
            assert t == 1 and n == "gru.weight_hh_l0" and not got.any()
        else:
            err = _rel(got, ref)
            print("%-24s rel %.2e" % (n, err))
            assert err < 1e-4, (n, err)
    pol.load_state_dict(before)
    ppo.update(mem)
    assert abs(ppo.last_loss.item() - losses[-1]) < 1e-4 * max(1.0, abs(losses[-1]))
    params = {n for n, _ in pol.named_parameters()}
    for n, p in pol.state_dict().items():
        got = p.detach().double().cpu()
        if "num_batches" in n:
            assert int(p) == int(final[n]) == int(before[n]) + k
        elif n not in params:
            assert _rel(got, final[n]) < 1e-4, n
        elif n == inert:
            assert (got - before[n].double()).abs().max().item() <= k * ppo.lr * (1 + 1e-6)
        else:
            step_ref, step_got = final[n] - before[n].double(), got - before[n].double()
            if not step_ref.any():
                assert not step_got.any(), n
                continue
            err = ((step_got - step_ref).norm() / step_ref.norm()).item()
            assert err < 5e-2, (n, err)
    for (n, p), (_, q) in zip(pol.state_dict().items(), ppo.policy_old.state_dict().items()):
        assert torch.equal(p, q), n


# ---- 6. train_stage2_batch_sth end to end ------------------------------------------------------------------------------------------------------
def _sth_model(vd):
    from adafocus_amd.gfv_net_sth import GFV
    from tests.test_state_dict_compat import sth_args
    a = sth_args()
    a.gpu, a.video_div, a.num_segments_focuser, a.patch_size = 0, vd, 12, 144
    m = GFV(a).eval()
    m.focuser.net.base_model = torch.nn.Sequential(*list(m.focuser.net.base_model.children())[:-1])  # evaluate.py:83
    m.load_state_dict(synth_sd("STH", 1007), strict=True)
    pol = {k[len("policy."):]: v for k, v in synth_sd("STH_POLICY" if vd == 1 else "STH_POLICY_VD2", 1007).items()}
    m.focuser.policy.policy_old.load_state_dict(pol)
    m.focuser.policy.policy.load_state_dict(pol)
    m.focuser.policy.policy_old.eval()
    m.focuser.policy.policy.eval()
    return m.to(DEV), a


@pytest.mark.parametrize("vd", [1, 2])
def test_train_stage2_batch_sth(vd):
    """One batch through the loop body on a small model (B = 2, Tg = 8, Tf = 12, P = 144): the memory is cleared, the policy moved,
    policy_old equals policy (buffers included), the frozen parts are bit-identical, the rewards are the confidence differences of the
    returned logits, and two runs from the same seeds give the same bits."""
    b = 2
    gl = torch.from_numpy(synth.synth_frames(b, 8, 224, seed=3)).to(DEV)
    fo = torch.from_numpy(synth.synth_frames(b, 12, 224, seed=4)).to(DEV)
    target = torch.tensor([3, 100], device=DEV)
    runs = []
    for _ in range(2):
        model, args = _sth_model(vd)
        with pytest.raises(NotImplementedError, match="policy_train_mode"):
            model.action_stage2(fo.view(b, 12, 3, 224, 224), None, None, 0, args, training=True)
        model.policy_train_mode()
        ppo = model.focuser.policy
        assert not model.training and ppo.policy.training and ppo.policy_old.training
        frozen = {k: v.clone() for k, v in model.state_dict().items()}
        start = copy.deepcopy(ppo.policy.state_dict())
        seen = []
        stage2 = model.action_stage2

        def spy(*a, **kw):
            out = stage2(*a, **kw)
            seen.append((out[0].clone(), out[1].clone()))
            return out

        model.action_stage2 = spy
        torch.manual_seed(17)
        pred, loss, rewards = train.train_stage2_batch_sth(model, gl, fo, target, args)
        mem = model.focuser.memory
        assert not (mem.states or mem.actions or mem.logprobs or mem.rewards or mem.hidden)
        assert pred.shape == (b, args.num_classes) and len(rewards) == len(seen) == vd and torch.equal(pred, seen[-1][0])
        assert torch.equal(loss, torch.nn.functional.cross_entropy(pred, target))
        for r, (total, base) in zip(rewards, seen):
            conf = torch.softmax(total, 1).gather(1, target.view(-1, 1)).view(1, -1)
            bconf = torch.softmax(base, 1).gather(1, target.view(-1, 1)).view(1, -1)
            assert r.shape == (1, b) and torch.equal(r, conf - bconf)
        after = ppo.policy.state_dict()
        for n, p in ppo.policy.named_parameters():
            if not (vd == 1 and n == "gru.weight_hh_l0"):           # (one step from the zero state: no gradient reaches weight_hh)
                assert not torch.equal(p.detach(), start[n]), n
        assert all(int(after[n]) == int(start[n]) + 1 for n in after if "num_batches" in n)
        for (n, p), (_, q) in zip(after.items(), ppo.policy_old.state_dict().items()):
            assert torch.equal(p, q), n
        for k, v in model.state_dict().items():
            assert torch.equal(v, frozen[k]), k
        runs.append((pred, loss, torch.cat(rewards), {n: v.clone() for n, v in after.items()}))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    for n in runs[0][3]:
        assert torch.equal(runs[0][3][n], runs[1][3][n]), n


# ---- 7. one training core for both policies -------------------------------------------------------------------------------------------------
def test_evaluate_backward_equals_train_backward():
    """The continuous policy with BatchNorm (B = 3, T = 2) through the autograd class it shares with the discrete one
    (policy_train.PolicyEvaluateFn): loss.backward() on evaluate's outputs gives the gradients of _train_backward for the same
    d loss / d head, torch.equal for every parameter.  The entropy is a constant of the distribution: it takes no gradient."""
    from adafocus_amd import policy_train
    b, t, feat, hw, h, sigma = 3, 2, 1280, 7, 1024, 0.25
    pol = _ppo(feat, hw, h, True, sigma, 1919).policy.to(DEV)
    states = _rnd((t, b, feat, hw, hw), 53, 0.5).to(DEV)
    actions = torch.rand(t, b, 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    g = [_rnd((t, b), 95 + i).to(DEV) for i in range(2)]
    logprobs, values, entropy = pol.evaluate(states, actions)
    assert type(logprobs.grad_fn) is policy_train.PolicyEvaluateFn._backward_cls and not entropy.requires_grad
    pol.zero_grad(set_to_none=True)
    ((logprobs * g[0]).sum() + (values * g[1]).sum()).backward()
    with torch.no_grad():
        fwd = pol._train_forward(pol._states_dense(states))
        want = pol._train_backward(fwd, hip_ops.ppo_gauss_head_backward(fwd["head"], actions, sigma, *g))
    assert set(want) == {n for n, _ in pol.named_parameters()} and len(want) == 15
    for n, p in pol.named_parameters():
        assert torch.equal(p.grad, want[n].reshape(p.shape)), n
        assert p.grad.abs().max() > 0 or n == "state_encoder.4.bias", n       # (BatchNorm1d removes that bias: zero in real arithmetic)
    # sum() hands the backward expanded (stride-0) upstream gradients: the head wrapper lays them out itself
    logprobs, values, entropy = pol.evaluate(states, actions)
    pol.zero_grad(set_to_none=True)
    (logprobs.sum() + 0.5 * values.sum()).backward()
    with torch.no_grad():
        fwd = pol._train_forward(pol._states_dense(states))
        dense = [torch.full((t, b), v, device=DEV) for v in (1.0, 0.5)]
        want = pol._train_backward(fwd, hip_ops.ppo_gauss_head_backward(fwd["head"], actions, sigma, *dense))
    for n, p in pol.named_parameters():
        assert torch.equal(p.grad, want[n].reshape(p.shape)), n
