"""Stage-2 training surface without a device: the new C-ABI exports and their workspace queries, the stage-2 mode switch, get_reward and
the G18 fixture (the reference roll-out and PPO update it pins)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from adafocus_amd import _lib, train
from adafocus_amd.gfv_net import GFV
from adafocus_amd.ppo import PPO, ActorCritic
from tests.helpers import manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g18_act_stage2.npz")
NEW = ("adaf_ppo_sample_f32", "adaf_ppo_returns_f32", "adaf_ppo_head_workspace_bytes", "adaf_ppo_head_f32", "adaf_ppo_rows_transpose_f32",
       "adaf_ppo_wenc_grad_workspace_bytes", "adaf_ppo_wenc_grad_f32", "adaf_ppo_encoder_backward_workspace_bytes",
       "adaf_ppo_encoder_backward_f32")


def _args(stage=2, **over):
    a = dict(num_segments=4, num_classes=200, reward="random", dataset="actnet", input_size=224, batch_size=2, patch_size=96,
             with_glancer=True, feature_map_channels=1280, glance_size=224, action_dim=49, hidden_state_dim=1024, policy_conv=True, gpu=0,
             continuous=False, gamma=0.7, policy_lr=0.0003, random_patch=False, dropout=0.5, consensus="gru", hidden_dim=1024,
             train_stage=stage)
    a.update(over)
    return types.SimpleNamespace(**a)


@pytest.fixture(scope="module")
def model():
    return GFV(_args())


def test_new_exports_declared_everywhere():
    with open(os.path.join(ROOT, "include", "adafocus.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SYMBOLS
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(_lib.load_library(), name)


def test_workspace_queries_without_a_device():
    lib = _lib.load_library()
    t, b, hw, c, cmid, h = 16, 64, 49, 1280, 32, 1024
    assert lib.adaf_ppo_head_workspace_bytes(t, b) == 2 * t * b * 4
    npix = t * b * hw
    # the larger of: one [32, C] partial per pixel slice (256 CUs / 5 chunks of 256 channels = 51 slices), the masked gradient [pixels, 32]
    wenc = max(51 * 32 * c, npix * cmid)
    assert lib.adaf_ppo_wenc_grad_workspace_bytes(npix, c, cmid) == wenc * 4
    assert lib.adaf_ppo_wenc_grad_workspace_bytes(100, 128, 32) == max(2 * 32 * 128, 100 * 32) * 4      # 64 pixels per slice at least
    rows, mid = t * b, hw * cmid
    floats = rows * h + rows * mid + h * mid + 32 * h + 51 * 32 * c        # (the encoder backward always takes the split-K form)
    assert lib.adaf_ppo_encoder_backward_workspace_bytes(t, b, hw, c, cmid, h) == floats * 4
    for bad in ((0, b), (t, 0), (-1, b)):
        assert lib.adaf_ppo_head_workspace_bytes(*bad) == 0
    for bad in ((0, c, cmid), (npix, 0, cmid), (npix, c, 0)):
        assert lib.adaf_ppo_wenc_grad_workspace_bytes(*bad) == 0
    for i in range(6):
        ext = [t, b, hw, c, cmid, h]
        ext[i] = 0
        assert lib.adaf_ppo_encoder_backward_workspace_bytes(*ext) == 0


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load_library()
    assert lib.adaf_ppo_sample_f32(None, None, 0, 1, 4, None, None, None, None, None) == -1
    assert lib.adaf_ppo_returns_f32(None, None, 1, 1, 0.7, None, None) == -1
    assert lib.adaf_ppo_head_f32(None, None, 1, 1, 1, 4, None, None, None, 0.2, *([None] * 9), 0, None) == -1
    assert lib.adaf_ppo_rows_transpose_f32(None, None, 1, 1, 1, None, None) == -1
    assert lib.adaf_ppo_wenc_grad_f32(None, None, None, None, 1, 128, 32, 1, None, None, 0, None) == -1
    assert lib.adaf_ppo_encoder_backward_f32(None, None, None, None, None, 1, 1, 49, 1280, 32, 1024, None, None, None, None, None, 0, None) == -1


def test_get_reward_matches_g18():
    g = np.load(GOLDEN)
    conf, last, base = (torch.from_numpy(g["reward_%s" % k]) for k in ("conf", "last", "base"))
    for kind in ("prev", "conf", "random"):
        reward, carry = train.get_reward(types.SimpleNamespace(reward=kind), conf, last, base)
        assert torch.equal(reward, torch.from_numpy(g["reward_%s" % kind])), kind
        assert carry is conf
    assert not np.array_equal(g["reward_prev"], g["reward_random"])
    with pytest.raises(NotImplementedError):
        train.get_reward(types.SimpleNamespace(reward="other"), conf, last, base)


def test_g18_fixture_is_self_consistent():
    g = np.load(GOLDEN)
    b, t, c, hw, a, h = (int(v) for v in g["dims"])
    assert (c, hw, a, h) == (1280, 7, 49, 1024)
    prob_floor, ratio_floor, surr_floor = (float(v) for v in g["floors"])
    eps = float(g["eps_clip"][0])
    # roll-out: probabilities sum to one, the recorded log-probability is the sampled action's, every sampled action clears the floor
    probs, act = g["rollout_probs"].astype(np.float64), g["rollout_actions"]
    assert probs.shape == (t, b, a) and act.shape == (t, b) and g["rollout_hidden"].shape == (t, b, h)
    assert np.abs(probs.sum(-1) - 1).max() < 1e-5
    p_act = np.take_along_axis(probs, act[..., None], 2)[..., 0]
    assert p_act.min() >= prob_floor
    assert np.abs(np.log(p_act) - g["rollout_logprobs"]).max() < 1e-5
    assert len(np.unique(act)) > 4
    for tag in ("same", "clip"):
        for k in ("returns", "logprobs", "values", "entropy"):
            assert g["%s_%s" % (tag, k)].size == t * b
        assert g["%s_loss" % tag].shape == (1,)
        assert g["%s_actor.0.weight" % tag].shape == (a, h) and g["%s_critic.0.weight" % tag].shape == (1, h)
        assert g["%s_state_encoder.0.weight" % tag].shape == (32, c, 1, 1)
        assert g["%s_state_encoder.3.weight@v" % tag].shape == (h,) and g["%s_u@state_encoder.3.weight" % tag].shape == (32 * hw * hw,)
        ret = g["%s_returns" % tag].astype(np.float64)
        assert abs(ret.mean()) < 1e-5 and abs(ret.std(ddof=1) - 1) < 1e-3
        # d loss / d actor bias sums (onehot - p) terms: zero
        assert abs(g["%s_actor.0.bias" % tag].sum()) < 1e-5
        spreads = [float(g[k][0]) for k in g.files if k.startswith("spread_%s_" % tag)]
        assert len(spreads) == 19 and 0 < min(spreads) and max(spreads) < 1e-5
    # same: ratios are one; clip: the four classes and the margins
    assert np.abs(np.exp(g["same_logprobs"].astype(np.float64) - g["rollout_logprobs"]) - 1).max() < 1e-4
    ratio = np.exp(g["clip_logprobs"].astype(np.float64) - g["clip_old_logprobs"])
    adv = g["clip_returns"].reshape(t, b).astype(np.float64) - g["clip_values"]
    lo, hi = 1 - eps, 1 + eps
    classes = [((ratio < lo) & (adv > 0)).sum(), ((ratio < lo) & (adv < 0)).sum(), ((ratio > hi) & (adv > 0)).sum(),
               ((ratio > hi) & (adv < 0)).sum()]
    assert min(classes) >= 1 and list(g["clip_classes"]) == [int(v) for v in classes]
    assert min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min()) >= ratio_floor
    assert float(g["clip_margins"][0]) >= ratio_floor and float(g["clip_margins"][1]) >= surr_floor
    surr1, surr2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    assert np.abs(surr1 - surr2)[(ratio < lo) | (ratio > hi)].min() >= surr_floor


def test_policy_train_mode_sets_the_stage2_modes(model):
    model.train()
    model.policy_train_mode()
    assert not model.training and not model.glancer.training and not model.focuser.training and not model.classifier.training
    assert not any(m.training for m in model.focuser.net.modules())
    for pol in (model.focuser.policy.policy, model.focuser.policy.policy_old):
        assert pol.training and all(m.training for m in pol.modules())
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        model.train_mode(_args(2))
    model.eval()
    assert not model.focuser.policy.policy_old.training


def test_one_step_act_training_needs_policy_train_mode(model):
    model.eval()
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(NotImplementedError, match="policy_train_mode"):
        model.one_step_act(x, torch.zeros(1, 1280, 7, 7), torch.zeros(1, 1280), restart_batch=True, training=True)


def test_ppo_keeps_the_manifest_state_dict_keys(model):
    keys = set(manifest()["ACT"])
    assert set(model.state_dict()) == keys
    ppo = model.focuser.policy
    assert isinstance(ppo.optimizer, torch.optim.Adam) and not any("optimizer" in k for k in ppo.state_dict())
    assert [id(p) for p in ppo.optimizer.param_groups[0]["params"]] == [id(p) for p in ppo.policy.parameters()]
    assert ppo.optimizer.param_groups[0]["lr"] == 0.0003 and tuple(ppo.optimizer.param_groups[0]["betas"]) == (0.9, 0.999)
    sd = ppo.state_dict()
    ppo.load_state_dict(sd, strict=True)
    assert set(sd) == {k[len("focuser.policy."):] for k in keys if k.startswith("focuser.policy.")}


def test_linear_encoder_has_no_backward():
    pol = ActorCritic(64, 64 * 4, 25, hidden_state_dim=32, policy_conv=False)
    with pytest.raises(NotImplementedError, match="policy_conv=False"):
        pol.evaluate(torch.zeros(2, 3, 64, 2, 2), torch.zeros(2, 3, dtype=torch.int64))
    ppo = PPO(64, 64 * 4, 25, 32, False)
    with pytest.raises(NotImplementedError, match="policy_conv=False"):
        ppo.update(types.SimpleNamespace(rewards=[], states=[], actions=[], logprobs=[]))
