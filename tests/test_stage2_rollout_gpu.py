"""The batched stage-2 roll-out on the GPU: the sampling and rewards kernels, the classifier's baseline branch, GFV.rollout_act against the
loop of one_step_act(training=True) bit for bit, and train_stage2_batch_fused against train_stage2_batch."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adafocus_amd import _lib, evaluate, hip_ops, synth, train
from adafocus_amd.gfv_net import GFV, RecurrentClassifier
from tests.helpers import manifest

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = 2.0 ** -22


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


@functools.lru_cache(maxsize=None)
def _models():
    """Two identically built models in stage-2 mode with the policies' initial state.  The reward kind is an attribute (`rew`) that the
    cases set; the cases that run an update put the policies back with `_reset`."""
    pair = []
    for _ in range(2):
        model, _ = _model()
        model.policy_train_mode()
        ppo = model.focuser.policy
        init = tuple({k: v.clone() for k, v in p.state_dict().items()} for p in (ppo.policy, ppo.policy_old))
        pair.append((model, init))
    return pair


def _reset(model, init, reward):
    ppo = model.focuser.policy
    ppo.policy.load_state_dict(init[0])
    ppo.policy_old.load_state_dict(init[1])
    ppo.optimizer = torch.optim.Adam(ppo.policy.parameters(), lr=ppo.lr, betas=ppo.betas)
    for p in ppo.policy.parameters():
        p.grad = None
    model.focuser.memory.clear_memory()
    model.rew = reward
    model.policy_train_mode()


def _snapshot(mem):
    return {k: [x.clone() for x in getattr(mem, k)] for k in ("states", "actions", "logprobs", "hidden")}


def _step_loop(model, frames, fmap, fvec, uniforms=None):
    """The parent's roll-out: T calls of one_step_act(training=True); explicit uniforms go step by step through policy_old.act."""
    pol = model.focuser.policy.policy_old
    t = frames.shape[1]
    step = [0]
    if uniforms is not None:
        inner = pol.act

        def act(state, memory, restart_batch=False, training=True):
            return inner(state, memory, restart_batch, training, uniforms=uniforms[step[0]])
        pol.act = act
    try:
        outs = []
        for s in range(t):
            step[0] = s
            logits, _, _, base = model.one_step_act(frames[:, s], fmap[:, s], fvec[:, s], restart_batch=s == 0, training=True)
            outs.append((logits.clone(), base.clone()))
    finally:
        if uniforms is not None:
            del pol.act
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


@functools.lru_cache(maxsize=None)
def _rollout_case(b, t, reward, explicit):
    """One case run both ways, once: the loop on the first model, rollout_act on the second, from the same seeds."""
    (loop_model, init0), (fused_model, init1) = _models()
    _reset(loop_model, init0, reward)
    _reset(fused_model, init1, reward)
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=3)).to(DEV)
    frames = images.view(b, t, 3, 224, 224)
    u = torch.rand(t, b, generator=torch.Generator().manual_seed(5)).to(DEV) if explicit else None
    res = {}
    for name, model in (("loop", loop_model), ("fused", fused_model)):
        torch.manual_seed(11)
        np.random.seed(12)
        fmap, fvec = model.glance(images)
        if name == "loop":
            logits, base = _step_loop(model, frames, fmap, fvec, u)
        else:
            logits, base = model.rollout_act(frames, fmap, fvec, uniforms=u)
        res[name] = dict(logits=logits, base=base, mem=_snapshot(model.focuser.memory), hx=model.classifier.hx.clone())
        model.focuser.memory.clear_memory()
    return res


# ---- 1. the sampling kernel against the existing export ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t,a", [(3, 5, 25), (2, 4, 49), (64, 16, 64)])
def test_sample_actions_equals_stepwise_sampling(b, t, a):
    g = torch.Generator().manual_seed(100 + a)
    logits = (torch.randn(b * t, a, generator=g) * 2).to(DEV)
    u = torch.rand(t, b, generator=g)
    u[0::2, 0] = 0.0
    u[1::2, -1] = 1.0 - 2.0 ** -24
    assert float(u.max()) < 1.0
    u = u.to(DEV)
    side = int(round(a ** 0.5))
    table = torch.from_numpy(synth.grid_table(side)).to(DEV)
    actions, logprobs, coords = hip_ops.ppo_sample_actions(logits, u, table)
    assert actions.shape == (t, b) and actions.dtype == torch.int64 and logprobs.shape == (t, b) and coords.shape == (b * t, 2)
    rows = logits.view(b, t, a)
    for s in range(t):
        want_a, want_lp = hip_ops.ppo_sample(rows[:, s].contiguous(), u[s])
        assert torch.equal(actions[s], want_a) and torch.equal(logprobs[s], want_lp), s
    assert torch.equal(coords, table[actions.t().reshape(-1)])
    assert len(torch.unique(actions)) > 2 and (actions[0::2, 0] == 0).all()
    # a row stride larger than A, and the index-only form
    wide = torch.full((b * t, a + 7), float("nan"), device=DEV)
    wide[:, :a] = logits
    view = wide[:, :a]
    assert view.stride(0) == a + 7
    a2, lp2, c2 = hip_ops.ppo_sample_actions(view, u, table)
    assert torch.equal(a2, actions) and torch.equal(lp2, logprobs) and torch.equal(c2, coords)
    a3, lp3 = hip_ops.ppo_sample_actions(logits, u)
    assert torch.equal(a3, actions) and torch.equal(lp3, logprobs)


def test_sample_actions_argument_rules():
    lib, h = _lib.load_library(), _lib.handle(DEV)
    x = torch.zeros(8, device=DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    p, n, s = _lib.ptr, _lib.ptr(None), _lib.stream_ptr()
    assert lib.adaf_ppo_sample_actions_f32(h, p(x), 0, 0, 2, 4, p(x), n, p(idx), p(x), n, s) == -1
    assert lib.adaf_ppo_sample_actions_f32(h, p(x), 0, 1, 2, 0, p(x), n, p(idx), p(x), n, s) == -1
    assert lib.adaf_ppo_sample_actions_f32(h, p(x), 0, 1, 2, 4, p(x), p(x), p(idx), p(x), n, s) == -1      # a table without coords_out
    assert lib.adaf_ppo_sample_actions_f32(h, p(x), 3, 1, 2, 4, p(x), n, p(idx), p(x), n, s) == -1         # ld < A
    torch.cuda.synchronize()


# ---- 2. the classifier's baseline branch against the step form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("b,t", [(3, 5), (20, 16)])
def test_branch_forward_equals_the_step_form(b, t):
    """Rows B*T = 15 are one persistent scan.  320 rows in one call would take the scan's launch-per-step form (above 256 rows), whose
    W_hh h sums in another order than the persistent kernel the steps of batch 20 run on: branch_forward sends them as 256 + 64."""
    feat, classes = 3328, 200
    torch.manual_seed(7)
    cls = RecurrentClassifier(seq_len=t, input_dim=feat, batch_size=b, hidden_dim=1024, num_classes=classes, dropout=0.0).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(b, t, feat, generator=g).to(DEV)
    x_base = torch.randn(b, t, feat, generator=g).to(DEV)
    with torch.no_grad():
        base_steps, main_steps = [], []
        for s in range(t):
            base_steps.append(cls.test_single_forward(x_base[:, s:s + 1], reset=s == 0)[0])
            main_steps.append(cls.single_forward(x[:, s:s + 1], reset=s == 0)[0])
        hx_steps = cls.hx.clone()
        logits, last, hx, hs = cls._steps_from(x, None, want_hs=True)
        branch = cls.branch_forward(x_base, hs)
    assert logits.shape == (b * t, classes) and branch.shape == (b * t, classes) and hs.shape == (b, t, 1024)
    assert torch.equal(logits.view(b, t, classes), torch.stack(main_steps, 1))
    assert torch.equal(last, main_steps[-1]) and torch.equal(hx, hx_steps) and torch.equal(hx[0], hs[:, -1])
    assert torch.equal(branch.view(b, t, classes), torch.stack(base_steps, 1))
    assert not torch.equal(branch, logits)
    assert hip_ops.gru_scan_timeouts() == 0


# ---- 3. the roll-out against the loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["seeded", "uniforms"])
@pytest.mark.parametrize("reward", ["random", "prev"])
@pytest.mark.parametrize("b,t", [(2, 4), (3, 5)])
def test_rollout_act_equals_the_step_loop(b, t, reward, explicit):
    res = _rollout_case(b, t, reward, explicit)
    loop, fused = res["loop"], res["fused"]
    assert fused["logits"].shape == (t, b, 200) and fused["base"].shape == (t, b, 200)
    for s in range(t):
        assert torch.equal(fused["logits"][s], loop["logits"][s]), s
        assert torch.equal(fused["base"][s], loop["base"][s]), s
        if reward == "random":
            assert not torch.equal(fused["base"][s], fused["logits"][s]), s
    for key, n in (("states", t), ("actions", t), ("logprobs", t), ("hidden", t + 1)):
        assert len(fused["mem"][key]) == len(loop["mem"][key]) == n, key
        for s, (x, y) in enumerate(zip(fused["mem"][key], loop["mem"][key])):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (key, s)
    assert fused["mem"]["states"][0].shape == (b, 1280, 7, 7) and fused["mem"]["actions"][0].shape == (b,)
    assert fused["mem"]["hidden"][0].shape == (1, b, 1024) and not fused["mem"]["hidden"][0].any()
    assert torch.equal(fused["hx"], loop["hx"])
    assert len(torch.unique(torch.stack(fused["mem"]["actions"]))) > 1


# ---- 4. the rewards kernel ----------------------------------------------------------------------------------------------------------------------
def _reward_reference(logits_tb, base_tb, target, kind, dtype):
    """main_dist.py:511-516, 574-581 on (T, B, C) logits, step by step: (rewards (T, B), confidences (T, B), the last step's loss)."""
    args = types.SimpleNamespace(reward=kind)
    index = target.view(-1, 1)
    last, rewards, confs = 0, [], []
    for s in range(logits_tb.shape[0]):
        conf = torch.gather(F.softmax(logits_tb[s].to(dtype), 1), 1, index).view(1, -1)
        bconf = torch.gather(F.softmax(base_tb[s].to(dtype), 1), 1, index).view(1, -1)
        r, last = train.get_reward(args, conf, last, bconf)
        rewards.append(r)
        confs.append(conf)
    return torch.cat(rewards, 0), torch.cat(confs, 0), F.cross_entropy(logits_tb[-1].to(dtype), target)


def _tolerances(logits_tb, base_tb, target, kind):
    """8x the largest distance of torch's own fp32 softmax -> gather -> get_reward (the step loop's arithmetic) from the float64 result, with
    a floor of 2^-22; the same for the cross-entropy."""
    r64, c64, l64 = _reward_reference(logits_tb, base_tb, target, kind, torch.float64)
    r32, _, l32 = _reward_reference(logits_tb, base_tb, target, kind, torch.float32)
    tol_r = max(8 * (r32.double() - r64).abs().max().item(), FLOOR)
    tol_l = max(8 * abs(l32.double().item() - l64.item()), FLOOR)
    return r64, c64, l64, tol_r, tol_l


def _reward_inputs(which):
    if which == "synthetic":
        b, t, c = 3, 5, 200
        g = torch.Generator().manual_seed(31)
        logits = ((torch.rand(t, b, c, generator=g) * 2 - 1) * 15).to(DEV)
        base = ((torch.rand(t, b, c, generator=g) * 2 - 1) * 15).to(DEV)
        target = torch.tensor([3, 150, 199], device=DEV)
        # a confident clip and a wrong one beside the spread ones
        logits[:, 0, 3] = 15.0
        return logits, base, target
    res = _rollout_case(3, 5, which, True)["loop"]
    return res["logits"], res["base"], torch.tensor([3, 150, 77], device=DEV)


@pytest.mark.parametrize("kind", ["prev", "conf", "random"])
@pytest.mark.parametrize("which", ["synthetic", "random", "prev"], ids=["synthetic", "rollout-random", "rollout-prev"])
def test_rewards_kernel(which, kind):
    logits_tb, base_tb, target = _reward_inputs(which)
    t, b, c = logits_tb.shape
    rows = logits_tb.transpose(0, 1).reshape(b * t, c)
    base_rows = base_tb.transpose(0, 1).reshape(b * t, c)
    rewards, conf, ce = hip_ops.ppo_rewards(rows, base_rows, target, t, kind, want_conf=True, want_ce_last=True)
    assert rewards.shape == (t, b) and conf.shape == (t, b) and ce.shape == (1,)
    r64, c64, l64, tol_r, tol_l = _tolerances(logits_tb, base_tb, target, kind)
    err_r = (rewards.double() - r64).abs().max().item()
    err_c = (conf.double() - c64).abs().max().item()
    err_l = abs(ce.double().item() - l64.item())
    print("%s / %s: rewards vs float64 %.3e (tolerance %.3e), confidences %.3e, cross-entropy %.3e (tolerance %.3e)"
          % (which, kind, err_r, tol_r, err_c, err_l, tol_l))
    assert err_r <= tol_r and err_c <= tol_r and err_l <= tol_l
    assert r64.abs().max().item() > 0
    # run to run, and the outputs that were not asked for change nothing
    again = hip_ops.ppo_rewards(rows, base_rows, target, t, kind)
    assert torch.equal(again, rewards)
    if kind == "prev":
        assert torch.equal(rewards[0], conf[0])
        assert torch.equal(rewards[1:], conf[1:] - conf[:-1])
        assert torch.equal(hip_ops.ppo_rewards(rows, None, target, t, kind), rewards)
    elif kind == "conf":
        assert torch.equal(rewards, conf)
        assert torch.equal(hip_ops.ppo_rewards(rows, None, target, t, kind), rewards)
    else:
        bconf = hip_ops.ppo_rewards(base_rows, None, target, t, "conf")
        assert torch.equal(rewards, conf - bconf)
        with pytest.raises(_lib.AdafError, match="base_logits"):
            hip_ops.ppo_rewards(rows, None, target, t, kind)


def test_rewards_kernel_target_out_of_range():
    logits_tb, base_tb, target = _reward_inputs("synthetic")
    t, b, c = logits_tb.shape
    rows = logits_tb.transpose(0, 1).reshape(b * t, c)
    base_rows = base_tb.transpose(0, 1).reshape(b * t, c)
    for bad in (c, -1):
        off = target.clone()
        off[1] = bad
        for kind in ("prev", "conf", "random"):
            good = hip_ops.ppo_rewards(rows, base_rows, target, t, kind)
            rewards, ce = hip_ops.ppo_rewards(rows, base_rows, off, t, kind, want_ce_last=True)
            assert torch.isnan(rewards[:, 1]).all() and torch.isnan(ce).all()
            assert torch.equal(rewards[:, 0], good[:, 0]) and torch.equal(rewards[:, 2], good[:, 2])
    lib, h = _lib.load_library(), _lib.handle(DEV)
    p, n, s = _lib.ptr, _lib.ptr(None), _lib.stream_ptr()
    out = torch.empty(t, b, device=DEV)
    assert lib.adaf_ppo_rewards_f32(h, p(rows), n, p(target), t, b, c, 2, p(out), n, n, s) == -1
    assert lib.adaf_ppo_rewards_f32(h, p(rows), n, p(target), t, b, c, 3, p(out), n, n, s) == -1
    assert lib.adaf_ppo_rewards_f32(h, p(rows), n, p(target), 0, b, c, 0, p(out), n, n, s) == -1
    torch.cuda.synchronize()


# ---- 5. the whole body ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reward", ["random", "prev"])
def test_train_stage2_batch_fused_end_to_end(reward):
    b, t = 2, 4
    images = torch.from_numpy(synth.synth_frames(b, t, 224, seed=3)).to(DEV)
    target = torch.tensor([3, 150], device=DEV)
    model, init = _models()[0]
    args = _act_args(reward=reward)
    ppo = model.focuser.policy

    def run(body, swap_rewards=None):
        _reset(model, init, reward)
        seen, steps = [], []
        inner, step_inner = model.focuser.update, model.one_step_act

        def spy():
            seen.extend(r.clone() for r in model.focuser.memory.rewards)
            if swap_rewards is not None:
                model.focuser.memory.rewards[:] = [r.clone() for r in swap_rewards]
            return inner()

        def step_spy(*a, **k):
            out = step_inner(*a, **k)
            steps.append((out[0].clone(), out[3].clone()))
            return out
        model.focuser.update, model.one_step_act = spy, step_spy
        try:
            torch.manual_seed(11)
            np.random.seed(12)
            preds, loss = body(model, images, target, args)
        finally:
            del model.focuser.update, model.one_step_act
        params = {n: p.detach().clone() for n, p in ppo.policy.named_parameters()}
        return preds, loss, seen, params, steps

    p0, l0, s0, w0, _ = run(train.train_stage2_batch_fused)
    p1, l1, s1, w1, _ = run(train.train_stage2_batch_fused)
    assert p0.shape == (t, b, 200) and l0.dim() == 0 and torch.isfinite(l0) and torch.isfinite(ppo.last_loss).all()
    assert torch.equal(p0, p1) and torch.equal(l0, l1) and all(torch.equal(w0[n], w1[n]) for n in w0)
    assert len(s0) == t and all(r.shape == (1, b) for r in s0) and all(torch.equal(x, y) for x, y in zip(s0, s1))
    assert any(not torch.equal(w0[n], init[0][n]) for n in w0)
    # afterwards: the memory is empty, policy_old is the policy
    mem = model.focuser.memory
    assert all(len(x) == 0 for x in (mem.actions, mem.states, mem.logprobs, mem.rewards, mem.is_terminals, mem.hidden))
    for (n, p), (n2, q) in zip(ppo.policy.named_parameters(), ppo.policy_old.named_parameters()):
        assert n == n2 and torch.equal(p, q), n
    # the step loop from the same seeds, its update run on the fused body's rewards: the same predictions, the same policy
    pl, ll, sl, wl, steps = run(train.train_stage2_batch, swap_rewards=s0)
    assert torch.equal(pl, p0)
    assert len(sl) == t and len(steps) == t
    logits_tb, base_tb = torch.stack([s[0] for s in steps]), torch.stack([s[1] for s in steps])
    _, _, l64, tol_r, tol_l = _tolerances(logits_tb, base_tb, target, reward)
    err_r = (torch.cat(s0, 0) - torch.cat(sl, 0)).abs().max().item()
    err_l = abs(l0.item() - ll.item())
    print("%s: stored rewards fused vs loop %.3e (tolerance %.3e), loss %.3e (tolerance %.3e)" % (reward, err_r, tol_r, err_l, tol_l))
    # (the loss: the fused body's is held to tol_l of the float64 mean by test_rewards_kernel, the loop's is tol_l / 8 from it by construction)
    assert err_r <= tol_r and err_l <= tol_l + tol_l / 8
    assert all(torch.equal(wl[n], w0[n]) for n in w0)
    # the trained model validates through the stage-2 evaluation loop
    model.eval()
    args.train_stage = 2
    dataset = [(images[i].cpu(), torch.tensor([int(target[i])])) for i in range(b)]
    top1, top5, mean_ap, logs = evaluate.validate(dataset, model, torch.nn.CrossEntropyLoss(), args, quiet=True)
    assert 0 <= top1 <= 100 and 0 <= top5 <= 100 and len(logs) > 0
    _reset(model, init, "random")


# ---- 6. the mode guards ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_act_mode_guards():
    b, t = 2, 4
    frames = torch.zeros(b, t, 3, 224, 224)
    fmap, fvec = torch.zeros(b, t, 1280, 7, 7), torch.zeros(b, t, 1280)
    rnd = GFV(_act_args(random_patch=True))
    with pytest.raises(NotImplementedError) as one:
        rnd.one_step_act(frames[:, 0], fmap[:, 0], fvec[:, 0], restart_batch=True, training=True)
    with pytest.raises(NotImplementedError) as all_steps:
        rnd.rollout_act(frames, fmap, fvec)
    assert str(all_steps.value) == str(one.value) and "random-patch model" in str(one.value)
    model, init = _models()[0]
    model.eval()
    try:
        with pytest.raises(NotImplementedError) as one:
            model.one_step_act(frames[:, 0], fmap[:, 0], fvec[:, 0], restart_batch=True, training=True)
        with pytest.raises(NotImplementedError) as all_steps:
            model.rollout_act(frames, fmap, fvec)
        assert str(all_steps.value) == str(one.value) and "policy_train_mode" in str(one.value)
        assert len(model.focuser.memory.actions) == 0
    finally:
        model.policy_train_mode()
